"""The optimiser and latent kernels of csrc/elementwise.hip (svae_sumsq, svae_radam, svae_clip_grad,
svae_reparam_kl_fwd / _bwd, the embedding gather / scatter) at the sizes where their main loops run, against the
float64 restatements of tests/optim_ref.py. The bounds are optim_ref's: 4 x the f32-vs-f64 deviation of the same
formulas, measured on the CPU by test_optim_ref.py on these inputs. Every output buffer carries 64 guard elements."""
import math

import numpy as np
import pytest
import torch

import optim_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K

dev = 'cuda'
GUARD = 64
SENTINEL = -7777.0
NBLK = 1024                       # the partial count training passes (transformer_vae._norm_partials)


def guarded(src, dtype=torch.float32, shape=None):
    """-> (buffer, view): a copy of `src` (or an uninitialised-looking fill for shape) followed by GUARD sentinels."""
    n = src.numel() if src is not None else int(np.prod(shape))
    full = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    if src is not None:
        full[:n] = src.flatten().to(dtype)
        shape = src.shape
    return full, full[:n].view(shape)


def guard_intact(full):
    return bool((full[-GUARD:] == torch.tensor(SENTINEL, dtype=full.dtype)).all().item())


def max_ulps(a, b):
    """Largest distance in units in the last place between two f32 tensors whose elements agree in sign."""
    assert bool((torch.signbit(a) == torch.signbit(b)).all().item())
    return (a.view(torch.int32).long() - b.view(torch.int32).long()).abs().max().item()


# ================================================================================================ sumsq
def _sumsq_run(g_cpu, n, nblk, pad=8192):
    buf = torch.full((n + pad,), 1.0e4, device=dev)          # read past n and the count is off by 1e8
    buf[:n] = g_cpu.to(dev)
    part_full = torch.full((nblk + GUARD,), SENTINEL, device=dev)
    K.sumsq(buf, n, part_full[:nblk])
    torch.cuda.synchronize()
    assert guard_intact(part_full)
    return buf[:n], part_full[:nblk]


@pytest.mark.parametrize('n,nblk', [(1, 4), (4095, 4), (3 * 4096 + 3, 4), (3 * 4096 + 4, 4), (7 * 4096 + 2050, 4),
                                    (7 * 4096 + 2051, 4), (7 * 4096 + 2052, 4), (7 * 4096 + 2053, 4),
                                    (5_243_028, 1024)])
def test_sumsq_counts_every_element_once(n, nblk):
    """Integers in {-1, 0, 1}: every partial is an exact count, so part.sum() == (g != 0).sum() exactly, and each
    block's partial is the count of its own vectors. Thread t (0 .. 256 nblk - 1) starts at i = 4 t, stride S = 1024
    nblk; the unrolled loop runs while i + 3 S + 4 <= n, the vector remainder loop takes 16-B steps of S while
    i + 4 <= n, the scalar tail is the last n % 4 elements. With nblk = 4 (S = 4096):
      n = 1               t = 0: scalar tail (1 element); nobody else reads.
      n = 4095            below one stride. t <= 1022: one remainder vector; t = 1023: scalar tail (3 elements).
      n = 3 S + 3         the last n without the unrolled loop. every t: three remainder vectors; t = 0 then the
                          scalar tail (3 elements at 3 S).
      n = 3 S + 4         the first n with it. t = 0: one unrolled trip (4 vectors), nothing else; t >= 1: three
                          remainder vectors.
      n = 7 S + 2050 + r  every t: one unrolled trip. Second unrolled trip for i <= 2046 + r: t <= 511 (r = 0, 1),
                          t <= 512 (r = 2, 3); those are done after it. The others: three remainder vectors, and
                          r = 0, 1: t = 512 a scalar tail of 2 + r elements at 7 S + 2048;
                          r = 2:    no tail (n % 4 == 0, t = 512's second trip ends exactly at n);
                          r = 3:    t = 513 a scalar tail of 1 element at 7 S + 2052.
    With nblk = 1024 (S = 1 048 576, the training pair) and n = 5 S + 148: every t one unrolled trip and one
    remainder vector (at 4 S), t <= 36 a second one (at 5 S); no tail."""
    gen = torch.Generator().manual_seed(n)
    owner = (torch.arange(n, device=dev) // 4) % (nblk * 256) // 256
    # a random draw, and 1 on the even trips of the stride / 0 on the odd ones: a vector fetched from a neighbouring
    # trip (u * stride off by one) always changes the second count, whatever the draw does
    for name, g_cpu in (('random', torch.randint(-1, 2, (n,), generator=gen).float()),
                        ('trip parity', (torch.arange(n) // (1024 * nblk) % 2 == 0).float())):
        g, part = _sumsq_run(g_cpu, n, nblk)
        nz = (g != 0)
        per_block = torch.bincount(owner, weights=nz.double(), minlength=nblk)
        print(f'sumsq n={n} nblk={nblk} {name}: sum of partials {part.double().sum().item():.0f}, '
              f'non-zeros {nz.sum().item()}')
        assert part.double().sum().item() == nz.sum().item()
        assert torch.equal(part.double(), per_block)


def test_sumsq_randn_at_the_training_pair():
    n = 5_243_028
    g_cpu = torch.randn(n, generator=torch.Generator().manual_seed(11))
    g, part = _sumsq_run(g_cpu, n, NBLK)
    ref = R.sumsq(g).item()
    rel = abs(part.double().sum().item() - ref) / ref
    print(f'sumsq randn: relative error {rel:.3e}')
    assert rel < 1e-5


# ================================================================================================ radam
@pytest.mark.parametrize('rho_ok', [0, 1])
@pytest.mark.parametrize('clip_active', [True, False])
@pytest.mark.parametrize('n', R.RADAM_SIZES)
def test_radam_three_steps_elementwise(n, clip_active, rho_ok):
    """Three consecutive steps from non-zero moments; p, m and v elementwise against float64 after every step.
    n = 4, 1020, 10000: n / 4 <= 2048 * 256, every thread at most one vector, in the tail loop. n = 5 243 028
    (n / 4 = 2 * 524288 + 262181, 2048 blocks): every thread one trip of the 2-way unrolled main loop, threads
    below 262181 one tail trip more. The 1024 partials (a real svae_sumsq) take the partial-sum loop four trips."""
    p0, m0, v0, gs, scals = R.radam_case(n, clip_active, rho_ok, dev)
    max_norm = scals[0][8].item()
    bufs = {k: guarded(t) for k, t in (('p', p0), ('m', m0), ('v', v0), ('p2', p0), ('m2', m0), ('v2', v0))}
    pbf_full, pbf = guarded(None, torch.bfloat16, (n,))
    part_full = torch.full((NBLK + GUARD,), SENTINEL, device=dev)
    part = part_full[:NBLK]
    norm = torch.full((1,), float('nan'), device=dev)
    p, m, v, p2, m2, v2 = (bufs[k][1] for k in ('p', 'm', 'v', 'p2', 'm2', 'v2'))
    ref = (p0, m0, v0)
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0, 'norm': 0.0}
    for g, scal in zip(gs, scals):
        sc = scal.to(dev)
        K.sumsq(g, n, part)
        K.radam(p, pbf, g, m, v, n, part, sc, norm)
        K.radam(p2, None, g, m2, v2, n, part, sc, None)
        torch.cuda.synchronize()
        *ref, rnorm = R.radam_step(*ref, g, scal.double().tolist())
        assert (rnorm.item() > 2 * max_norm) if clip_active else (rnorm.item() < 0.5 * max_norm)
        for k, got, want in (('p', p, ref[0]), ('m', m, ref[1]), ('v', v, ref[2])):
            worst[k] = max(worst[k], R.deviation(got, want))
        worst['norm'] = max(worst['norm'], abs(norm.item() - rnorm.item()) / rnorm.item())
        assert torch.equal(pbf, p.bfloat16())                      # bit-equal over the whole range, every step
        assert torch.equal(p2, p) and torch.equal(m2, m) and torch.equal(v2, v)      # pbf = None: the same update
        assert all(guard_intact(full) for full, _ in bufs.values()) and guard_intact(pbf_full)
        assert guard_intact(part_full)
    print(f'radam n={n} clip={clip_active} rho_ok={rho_ok}: deviation p {worst["p"]:.3e} m {worst["m"]:.3e} '
          f'v {worst["v"]:.3e}, norm rel {worst["norm"]:.3e}')
    assert worst['p'] <= R.radam_bound(R.F32_DEV_P)
    assert worst['m'] <= R.radam_bound(R.F32_DEV_M)
    assert worst['v'] <= R.radam_bound(R.F32_DEV_V)
    assert worst['norm'] < 1e-5


# ================================================================================================ clip_grad
def _clip_input(n, scale):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n + int(scale * 10)))
    return g * (scale * math.sqrt(n) / g.double().norm().item())       # |g| = scale * max_norm, max_norm = sqrt(n)


CLIP_SIZES = [4, 1020, 2_097_152 + 4096]        # the last: past 2048 * 256 * 4, a second trip of the grid stride


@pytest.mark.parametrize('n', CLIP_SIZES)
def test_clip_grad_above_the_threshold(n):
    max_norm = math.sqrt(n)
    g_cpu = _clip_input(n, 3.0)
    full, g = guarded(g_cpu)
    full2, g2 = guarded(g_cpu)
    before = g.clone()
    part_full = torch.full((NBLK + GUARD,), SENTINEL, device=dev)
    norm = torch.full((1,), float('nan'), device=dev)
    K.sumsq(g, n, part_full[:NBLK])
    K.clip_grad(g, n, part_full[:NBLK], max_norm, norm)
    K.clip_grad(g2, n, part_full[:NBLK], max_norm, None)            # norm_out = None
    torch.cuda.synchronize()
    ref_norm = R.sumsq(before).sqrt().item()
    rel = abs(norm.item() - ref_norm) / ref_norm
    # the kernel's own coefficient, re-formed on the host in float32 from the norm it reported
    coef = min(np.float32(1.0), np.float32(max_norm) / (np.float32(norm.item()) + np.float32(1e-6)))
    assert coef.dtype == np.float32 and coef < 0.5
    ulps = max_ulps(g, before * float(coef))
    print(f'clip n={n}: norm rel {rel:.3e}, coef {coef}, max ulps {ulps}')
    assert rel < 1e-5
    assert ulps <= 2
    assert R.deviation(g, R.clip(before, max_norm)[0]) <= 1e-5        # and the float64 clip, the norm's bound
    assert torch.equal(g2, g)
    assert guard_intact(full) and guard_intact(full2) and guard_intact(part_full)


@pytest.mark.parametrize('n', CLIP_SIZES)
def test_clip_grad_below_the_threshold(n):
    max_norm = math.sqrt(n)
    full, g = guarded(_clip_input(n, 0.1))
    before = g.clone()
    part_full = torch.full((NBLK + GUARD,), SENTINEL, device=dev)
    norm = torch.full((1,), float('nan'), device=dev)
    K.sumsq(g, n, part_full[:NBLK])
    K.clip_grad(g, n, part_full[:NBLK], max_norm, norm)
    torch.cuda.synchronize()
    ref_norm = R.sumsq(before).sqrt().item()
    assert ref_norm < 0.5 * max_norm
    assert torch.equal(g.view(torch.int32), before.view(torch.int32))      # bit-identical: the early return
    assert abs(norm.item() - ref_norm) / ref_norm < 1e-5                   # and the norm is still written
    assert guard_intact(full) and guard_intact(part_full)


def test_accumulation_micro_step_clips_the_arena():
    """on_after_backward with require_backward_grad_sync = False (a gradient-accumulation micro-step) on the `tiny`
    golden: the arena becomes clip(arena, threshold), the logged grad_norm is the norm before the clip."""
    from golden_util import setup
    from oracle.params import TIED_ALIASES
    from sparse_vae import TransformerVAE, TransformerVAEHparams
    g, hp, params, ids = setup('tiny')
    threshold = 0.05
    mhp = TransformerVAEHparams(d_model=hp.d_model, num_heads=hp.num_heads, num_layers=hp.num_layers, latent_depth=64,
                                sparse_self_attention=False, kl_weight=float(g['kl_weight']),
                                grad_clip_threshold=threshold)
    model = TransformerVAE(mhp, device='cuda')
    sd = dict(params)
    for alias in TIED_ALIASES:
        sd[alias] = params['input_layer.0.weight']
    model.load_state_dict(sd, strict=True)
    model.train()
    batch = {'token_ids': ids, 'num_tokens': torch.from_numpy(g['lens'])}
    out = model.training_step(batch, 0, eps=torch.from_numpy(g['eps']).cuda(), dropout=0.0)
    model.require_backward_grad_sync = False
    out['loss'].backward()
    n = model._flat.n_live
    before = model._flat.grad[:n].clone()
    tail = model._flat.grad[n:].clone()
    model.on_after_backward()
    torch.cuda.synchronize()
    want, norm = R.clip(before, threshold)
    assert norm.item() > 2 * threshold                                     # the clip is active
    logged = float(model.logged['grad_norm'])
    d = R.deviation(model._flat.grad[:n], want)
    print(f'arena clip: n_live {n}, norm {norm.item():.5f}, logged {logged:.5f}, deviation {d:.3e}')
    assert abs(logged - norm.item()) / norm.item() < 1e-5
    assert d <= 1e-5                       # the coefficient carries the f32 norm's error (1e-5 relative at the most)
    assert abs(model._flat.grad[:n].double().norm().item() - threshold) < 1e-4 * threshold
    assert torch.equal(model._flat.grad[n:], tail)


# ================================================================================================ reparam + KL
def _kl_dev(got, want):
    return max(R.deviation(got[:1], want[:1]), R.deviation(got[1:], want[1:]))


@pytest.mark.parametrize('wide', [True, False], ids=['logvar-6..3', 'logvar-0.5randn'])
@pytest.mark.parametrize('B,Z', R.REPARAM_SHAPES)
def test_reparam_kl_forward_and_backward(B, Z, wide):
    """B > 64: the second b0 pass; B % 16 != 0: a ragged group of NB (b < B false inside it); Z < 64: idle lanes;
    Z = 96: a partial second lane trip; Z = 128, 256: whole further trips. ntok differs per row, from 1."""
    stats, eps, ntok, dz = R.reparam_case(B, Z, wide, dev)
    zr, rawr, klr = R.reparam_kl(stats, eps, ntok)
    outs = {k: guarded(None, dt, sh) for k, dt, sh in (('z', torch.float32, (B, Z)), ('zb', torch.bfloat16, (B, Z)),
                                                      ('eo', torch.float32, (B, Z)), ('raw', torch.float32, (B,)),
                                                      ('kl', torch.float32, (2,)), ('z2', torch.float32, (B, Z)),
                                                      ('raw2', torch.float32, (B,)), ('kl2', torch.float32, (2,)))}
    z, zb, eo, raw, kl, z2, raw2, kl2 = (outs[k][1] for k in ('z', 'zb', 'eo', 'raw', 'kl', 'z2', 'raw2', 'kl2'))
    K.reparam_fwd(stats, eps, 0, ntok, z, zb, eo, raw, kl, B, Z)
    K.reparam_fwd(stats, eps, 0, ntok, z2, None, None, raw2, kl2, B, Z)
    torch.cuda.synchronize()
    d = {'z': R.deviation(z, zr), 'raw_kl': R.deviation(raw, rawr), 'kl': _kl_dev(kl, klr)}
    print(f'reparam fwd B={B} Z={Z} wide={wide}: deviation z {d["z"]:.3e} raw_kl {d["raw_kl"]:.3e} kl {d["kl"]:.3e}')
    assert d['z'] <= R.reparam_bound(R.F32_DEV_Z)
    assert d['raw_kl'] <= R.reparam_bound(R.F32_DEV_RAW_KL)
    assert d['kl'] <= R.reparam_bound(R.F32_DEV_KL)                # both entries, each on its own scale
    assert torch.equal(zb, z.bfloat16())
    assert torch.equal(eo.view(torch.int32), eps.view(torch.int32))
    assert torch.equal(z2, z) and torch.equal(raw2, raw) and torch.equal(kl2, kl)
    assert all(guard_intact(full) for full, _ in outs.values())

    gkl = torch.tensor([0.7], device=dev)
    for dzi in (dz, None):                                         # None: the KL-only gradient
        ds_full, ds = guarded(None, torch.float32, (B, 2 * Z))
        K.reparam_bwd(stats, eps, dzi, ntok, gkl, ds, B, Z)
        torch.cuda.synchronize()
        db = R.deviation(ds, R.reparam_kl_bwd(stats, eps, ntok, dzi, 0.7), rows=True)
        print(f'reparam bwd B={B} Z={Z} wide={wide} dz={"given" if dzi is not None else None}: deviation {db:.3e}')
        assert db <= R.reparam_bound(R.F32_DEV_DSTATS)
        assert guard_intact(ds_full)


def _abs_corr_moments(n):
    """Mean and variance of |r| for the sample correlation r of two independent normal samples of length n:
    r has density (1 - r^2)^((n - 4) / 2) / B(1/2, (n - 2) / 2), so E|r| = 2 / ((n - 2) B(1/2, (n - 2) / 2)), and
    E r^2 = 1 / (n - 1)."""
    mean = 2.0 / ((n - 2) * math.sqrt(math.pi)) * math.exp(math.lgamma((n - 1) / 2) - math.lgamma((n - 2) / 2))
    return mean, 1.0 / (n - 1) - mean * mean


def _adjacent_corr(x):
    """Sample correlations of x[i] with x[i + 1] (rows of a 2-D float64 tensor)."""
    c = x - x.mean(-1, keepdim=True)
    c = c / c.norm(dim=-1, keepdim=True)
    return (c[:-1] * c[1:]).sum(-1)


def test_reparam_in_kernel_noise():
    B, Z = 130, 96
    stats, _, ntok, _ = R.reparam_case(B, Z, True, dev)

    def draw(seed):
        outs = [guarded(None, dt, sh) for dt, sh in ((torch.float32, (B, Z)), (torch.float32, (B, Z)),
                                                      (torch.float32, (B,)), (torch.float32, (2,)))]
        K.reparam_fwd(stats, None, seed, ntok, outs[0][1], None, outs[1][1], outs[2][1], outs[3][1], B, Z)
        torch.cuda.synchronize()
        assert all(guard_intact(full) for full, _ in outs)
        return outs[0][1], outs[1][1]

    z, e = draw(99)
    z_again, e_again = draw(99)
    _, e_other = draw(100)
    assert torch.equal(e.view(torch.int32), e_again.view(torch.int32)) and torch.equal(z, z_again)
    assert (e != e_other).float().mean().item() > 0.99
    assert bool(torch.isfinite(e).all().item())
    assert torch.unique(e, dim=0).shape[0] == B                    # no two rows equal
    assert torch.unique(e.t().contiguous(), dim=0).shape[0] == Z   # no two columns equal
    dz = R.deviation(z, R.reparam_kl(stats, e, ntok)[0])           # z = mu + eps_out * exp(0.5 logvar)
    assert dz <= R.reparam_bound(R.F32_DEV_Z)

    x = e.double().cpu()
    N = B * Z
    mean, var, m4 = x.mean().item(), (x * x).mean().item(), x.pow(4).mean().item()
    # standard errors of the sample moments of N(0, 1): Var x = 1, Var x^2 = 2, Var x^4 = E x^8 - 9 = 96
    se_mean, se_var, se_m4 = math.sqrt(1 / N), math.sqrt(2 / N), math.sqrt(96 / N)
    print(f'noise: mean {mean:.4f} (se {se_mean:.4f}), E x^2 {var:.4f} (se {se_var:.4f}), E x^4 {m4:.4f} '
          f'(se {se_m4:.4f}), z deviation {dz:.3e}')
    assert abs(mean) <= 5 * se_mean
    assert abs(var - 1) <= 5 * se_var
    assert abs(m4 - 3) <= 5 * se_m4
    for name, rows in (('rows', x), ('columns', x.t().contiguous())):
        r = _adjacent_corr(rows)
        k, n = r.numel(), rows.shape[1]
        mu_abs, var_abs = _abs_corr_moments(n)
        se_signed, se_abs = math.sqrt(1 / (n - 1) / k), math.sqrt(var_abs / k)
        print(f'noise, adjacent {name}: mean r {r.mean().item():.4f} (se {se_signed:.4f}), mean |r| '
              f'{r.abs().mean().item():.4f} (independent: {mu_abs:.4f}, se {se_abs:.4f})')
        assert abs(r.mean().item()) <= 5 * se_signed               # no common sign
        # mean |r| sits at the value independent rows give, which is itself below one standard error of a single r;
        # identical or strongly (anti)correlated neighbours push it towards 1
        assert abs(r.abs().mean().item() - mu_abs) <= 5 * se_abs
        assert r.abs().mean().item() <= 5 * math.sqrt(1 / (n - 1))


# ================================================================================================ embedding
def _half_zero_ids(T, V, seed):
    gen = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, V, (T,), generator=gen, dtype=torch.int32)
    ids[torch.randperm(T, generator=gen)[:T // 2]] = 0             # the padding id, as padded batches send it
    return ids


@pytest.mark.parametrize('D', [128, 200, 768])
def test_embedding_bwd_contended_padding_row(D):
    """Half of the 1027 rows (not a multiple of the block's 4) scatter into table row 0: ~513 atomic adds per
    element of one row. Quarter-integer gradients make every order of the f32 adds exact, so the whole table is
    compared bit for bit; N(0, 1) gradients are held to the worst-case bound of a k-term f32 sum in any order,
    (k - 1) 2^-24 sum |g|, per element, row 0 on its own."""
    T, V = 1027, 300
    ids = _half_zero_ids(T, V, D).to(dev)
    gen = torch.Generator().manual_seed(D + 1)
    for exact in (True, False):
        g = (torch.randint(-3, 4, (T, D), generator=gen) / 4.0 if exact else torch.randn(T, D, generator=gen)).to(dev)
        dt_full, dt = guarded(torch.zeros(V, D))
        K.embedding_bwd(ids, g, dt, T, D)
        torch.cuda.synchronize()
        ref = torch.zeros(V, D, device=dev, dtype=torch.float64).index_add_(0, ids.long(), g.double())
        assert guard_intact(dt_full)
        if exact:
            assert torch.equal(dt.double(), ref)
            continue
        mag = torch.zeros(V, D, device=dev, dtype=torch.float64).index_add_(0, ids.long(), g.double().abs())
        k = torch.bincount(ids.long(), minlength=V).double()[:, None]
        err, bound = (dt.double() - ref).abs(), (k - 1).clamp_min(0.5) * 2.0 ** -24 * mag
        print(f'embedding bwd D={D}: row 0 takes {int(k[0].item())} rows, max error {err[0].max().item():.3e} '
              f'(bound {bound[0].min().item():.3e}..), other rows {err[1:].max().item():.3e}')
        assert int(k[0].item()) == T // 2
        assert bool((err[0] <= bound[0]).all().item())             # the contended row on its own
        assert bool((err[1:] <= bound[1:]).all().item())


@pytest.mark.parametrize('D', [128, 200, 768])
def test_embedding_fwd_bf16_and_dual_outputs(D):
    T, V = 301, 300                                                # 301 rows: the last block has one live wave
    table = torch.randn(V, D, generator=torch.Generator().manual_seed(D)).to(dev)
    ids = _half_zero_ids(T, V, D + 2).to(dev)
    want = table[ids.long()]
    out_full, out = guarded(None, torch.float32, (T + 1, D))       # a guard row (and the 64 elements) after `out`
    bf_full, bf = guarded(None, torch.bfloat16, (T + 1, D))
    K.check(K.lib.svae_embedding_fwd(ids.data_ptr(), table.data_ptr(), out.data_ptr(), bf.data_ptr(), T, D,
                                     K.stream()), 'svae_embedding_fwd')
    a_full, a = guarded(None, torch.float32, (T + 1, D))
    b_full, b = guarded(None, torch.float32, (T + 1, D))
    K.embedding_fwd(ids, table, a, T, D, out2=b)
    torch.cuda.synchronize()
    assert torch.equal(out[:T], want) and torch.equal(bf[:T], want.bfloat16())
    assert torch.equal(a[:T], want) and torch.equal(b[:T], want)
    for full, view in ((out_full, out), (bf_full, bf), (a_full, a), (b_full, b)):
        assert bool((view[T] == torch.tensor(SENTINEL, dtype=view.dtype)).all().item()) and guard_intact(full)
