"""The four kernels behind svae_gemm (csrc/gemm.hip: gemm_skinny_kernel, gemm_kernel, gemm_glds_kernel, gemm256_kernel
with its persistent loop) one at a time, every epilogue per element against the float64 restatements of
tests/gemm_ref.py: at the smallest shapes at which each kernel's K loop, tile edges (ragged M, a last 4-column group:
N % 8 == 4), XCD remap with a remainder, persistent second tile, L2 grouping, batch strides and split-K slices are
live. Every case asserts the route it is named for (gemm_ref.route with the device's CU count): a dispatch change fails
there ("move the shape") instead of silently testing another kernel. The f32 bounds are gemm_ref.bound(): 4 x the
f32-vs-f64 deviation of the same formula on these inputs (measured on the CPU by test_gemm_ref.py, recorded in
tests/golden/gemm_bounds.json), never below 2^-21, on the error divided by the element's own scale
|alpha| |A| |B| + |bias| + |resid|; bf16 outputs carry 2^-8 |ref| on top. No element is excluded. Integer data is
bit-exact. Every output is a view into a sentinel-guarded buffer with a leading dimension above its column count, NaN
(or the known addend of an accumulating epilogue) before the launch.

DROPOUT_RESID, F32_ACC and F32_ATOMIC are given no bias and GELU_BWD none either: the 128-tile kernels do not add one
there while gemm256 and the skinny kernel do, and no caller passes one."""
import functools

import pytest
import torch

import gemm_ref as R
import sentinels as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae import _native as N
    from sparse_vae.engine import rotary_table

dev = 'cuda'
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
NAN = float('nan')
PAD = 1e30                         # what the padding of a strided input holds: a read of it shows in the output
ALPHA = 0.75                       # the real-valued epilogues' alpha (test_gemm_ref.py measures the bounds with it)


def n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def ld_of(n, route=None):
    """A leading dimension above n that validate_desc takes (% 8); the skinny cases write rows strided by 2 n."""
    return 2 * n if route == 'skinny' else (n + 7) // 8 * 8 + 8


def padded(t, ld):
    """-> (buffer [rows, ld] whose columns past t's hold PAD, its view of t's shape)."""
    buf = torch.full((t.shape[0], ld), PAD, dtype=t.dtype, device=dev)
    buf[:, :t.shape[1]] = t
    return buf, buf[:, :t.shape[1]]


@functools.lru_cache(maxsize=2)
def case(M, Nn, Kk, a_t=0, b_t=0, batch=1):
    """gemm_ref.inputs on the device (shared by the tests of one shape; nothing writes to it)."""
    c = R.inputs(M, Nn, Kk, a_t, b_t, batch)
    d = R.Case()
    d.M, d.N, d.K, d.a_t, d.b_t, d.batch = M, Nn, Kk, a_t, b_t, batch
    d.A, d.W, d.Ai, d.Wi = c.A.to(dev), c.W.to(dev), c.Ai.to(dev), c.Wi.to(dev)
    (d.As, d.Bs), (d.Asi, d.Bsi) = [[t.to(dev) for t in R.stored(c, i)] for i in (False, True)]
    d.bias, d.bias_mod, d.c0 = c.bias.to(dev), c.bias_mod.to(dev), c.c0.to(dev)
    d.ldr, d.ldgp = Nn + 4, ld_of(Nn)
    d.rbuf, d.resid = padded(c.resid.to(dev), d.ldr)
    d.gpbuf, d.gp = padded(c.gp.to(dev), d.ldgp)
    return d


def bits(t):
    return t.contiguous().view(torch.int16) if t.dtype == bf16 else t.contiguous().view(torch.int32)


def same_bits(a, b):
    return torch.equal(bits(a), bits(b))


def assert_route(name, c, epi, persistent=None, **kw):
    r = R.route(c.M, c.N, c.K, c.a_t, c.b_t, epi, batch=c.batch, n_cu=n_cu(), **kw)
    assert r[0] == name, ('the dispatch changed: move the shape', (c.M, c.N, c.K), epi, r)
    if persistent is not None:
        assert r[2] == persistent, ('the device has another CU count: move the shape', r, n_cu())
    return r


def gemm(c, C, ldc, epi, integer=False, **kw):
    As, Bs = (c.Asi, c.Bsi) if integer else (c.As, c.Bs)
    K.gemm(As, Bs, C, c.M, c.N, c.K, a_t=bool(c.a_t), b_t=bool(c.b_t), ldc=ldc, epi=getattr(N, 'EPI_' + epi), **kw)
    torch.cuda.synchronize()


def report(what, dev_at, limit):
    S.report(f'{what} (worst at {dev_at[1]})', dev_at[0], limit)


def ratio(what, exc_at):
    S.ratio(f'{what} (worst at {exc_at[1]})', exc_at[0])


def out(c, dtype, route=None, fill=NAN):
    ld = ld_of(c.N, route)
    full, view = S.matrix(c.M, c.N, ld, dtype, fill=fill)
    return full, view, ld


# ================================================================================================ real-valued epilogues
@pytest.mark.parametrize('route,M,Nn,Kk,a_t,b_t', R.REAL_CASES)
def test_epilogues_per_element(route, M, Nn, Kk, a_t, b_t):
    """BF16, F32 (plain, + bias + residual), GELU (both outputs), GELU_BWD, DROPOUT_RESID with its bf16 copy and F32
    with its dropout-masked bf16 copy, each element against float64. gemm256 at N = 1004 ends every row in a 4-column
    group: GELU_BWD there once multiplied it by zeros instead of the stored GELU' (columns 1000-1003)."""
    c = case(M, Nn, Kk, a_t, b_t)
    for epi in ('BF16', 'F32', 'GELU', 'GELU_BWD', 'DROPOUT_RESID'):
        r = assert_route(route, c, epi)
    if route == 'g256':
        assert r[1:] == R.route(M, Nn, Kk, n_cu=256)[1:], ('the device has another CU count: move the shape', r)
    tag = f'{route} {M}x{Nn}x{Kk} lay {a_t}{b_t}'
    ref, sc = R.gemm(c.A, c.W, ALPHA)

    Cf, C, ld = out(c, bf16, route)
    gemm(c, C, ld, 'BF16', bias=c.bias, alpha=ALPHA)
    assert S.intact(Cf, M, Nn)
    ratio(f'{tag} BF16', R.bf16_excess(C, R.epi_bf16(ref, c.bias), R.bound('f32'), sc + c.bias.abs()))

    Cf, C, ld = out(c, f32, route)
    gemm(c, C, ld, 'F32', alpha=ALPHA)
    assert S.intact(Cf, M, Nn)
    report(f'{tag} F32', R.deviation(C, ref, sc), R.bound('acc'))

    Cf, C, ld = out(c, f32, route)
    gemm(c, C, ld, 'F32', bias=c.bias, resid=c.rbuf, ldr=c.ldr, alpha=ALPHA)
    assert S.intact(Cf, M, Nn)
    report(f'{tag} F32 + bias + resid', R.deviation(C, R.epi_f32(ref, c.bias, c.resid), sc + c.bias.abs() + c.resid.abs()),
           R.bound('f32'))

    Cf, C, ld = out(c, bf16, route)
    Xf, X, ldx = out(c, bf16)
    gemm(c, C, ld, 'GELU', bias=c.bias_mod, aux=X, ldaux=ldx, alpha=ALPHA)
    assert S.intact(Cf, M, Nn) and S.intact(Xf, M, Nn)
    x = R.epi_f32(ref, c.bias_mod)
    g, gp = R.gelu_erf(x)
    sx = sc + c.bias_mod.abs()
    ratio(f'{tag} GELU g', R.bf16_excess(C, g, R.bound('gelu.g'), sx, extra=R.as_gap() * x.abs()))
    ratio(f"{tag} GELU g'", R.bf16_excess(X, gp, R.bound('gelu.gp'), sx + 1, extra=R.as_gap()))

    Cf, C, ld = out(c, bf16, route)
    gemm(c, C, ld, 'GELU_BWD', aux=c.gpbuf, ldaux=c.ldgp, alpha=ALPHA)
    assert S.intact(Cf, M, Nn)
    ratio(f'{tag} GELU_BWD', R.bf16_excess(C, R.epi_gelu_bwd(ref, c.gp), R.bound('gelu_bwd'), sc * c.gp.double().abs()))

    for p in R.DROP_P:
        keep = R.dropout_keep(M, Nn, p, R.SEED).to(dev)
        Cf, C, ld = out(c, f32, route)
        Xf, X, ldx = out(c, bf16)
        gemm(c, C, ld, 'DROPOUT_RESID', resid=c.rbuf, ldr=c.ldr, drop_p=p, seed=R.SEED, aux=X, ldaux=ldx, alpha=ALPHA)
        assert S.intact(Cf, M, Nn) and S.intact(Xf, M, Nn)
        assert same_bits(C[~keep], c.resid[~keep])                       # dropped: C - R is exactly 0
        report(f'{tag} DROPOUT_RESID p={p}',
               R.deviation(C, R.epi_dropout_resid(ref, c.resid, keep, p), sc * R.dropout_scale(p) * keep + c.resid.abs()),
               R.bound('dropout'))
        assert same_bits(X, C.to(bf16))

    for p in R.COPY_P:
        keep = R.dropout_keep(M, Nn, p, R.SEED).to(dev)
        Cf, C, ld = out(c, f32, route)
        Xf, X, ldx = out(c, bf16)
        gemm(c, C, ld, 'F32', bias=c.bias, aux=X, ldaux=ldx, drop_p=p, seed=R.SEED, alpha=ALPHA)
        assert S.intact(Cf, M, Nn) and S.intact(Xf, M, Nn)
        report(f'{tag} F32 + aux p={p}', R.deviation(C, R.epi_f32(ref, c.bias), sc + c.bias.abs()), R.bound('f32'))
        assert same_bits(X, R.epi_f32_copy(C, keep, p).to(bf16))


@pytest.mark.parametrize('rows,cols,p', [(37, 100, 0.25), (136, 132, 0.1), (12100, 1004, 0.25)])
def test_dropout_bwd_cast_draws_the_numpy_mask(rows, cols, p):
    """svae_dropout_bwd_cast (the backward's regeneration of the GEMM epilogues' mask) against the numpy generator, not
    against another kernel."""
    keep = R.dropout_keep(rows, cols, p, R.SEED).to(dev)
    gf, g = S.matrix(rows, cols, cols, bf16, fill=NAN)
    K.dropout_bwd_cast(torch.ones(rows, cols, device=dev), g, p, R.SEED, rows, cols)
    torch.cuda.synchronize()
    assert S.intact(gf, rows, cols)
    assert same_bits(g, R.epi_f32_copy(torch.ones(rows, cols, device=dev), keep, p).to(bf16))


# ================================================================================================ integers, bit-exact
@pytest.mark.parametrize('alpha', [-0.5, 2.0])
@pytest.mark.parametrize('route,M,Nn,Kk,a_t,b_t', R.INT_CASES)
def test_integer_alpha_and_accumulate_exact(route, M, Nn, Kk, a_t, b_t, alpha):
    """alpha != 1 (each kernel applies it in its own place) and F32_ACC onto a non-constant C, bit-exact on integer
    data; the 21-block grids run the XCD remap with remainder 5, where a tile left out shows as NaN and a tile taken
    twice as a doubled accumulate."""
    c = case(M, Nn, Kk, a_t, b_t)
    assert_route(route, c, 'F32')
    assert_route('glds' if route == 'skinny' else route, c, 'F32_ACC')
    want = (alpha * (c.Ai.double() @ c.Wi.double().t())).float()
    Cf, C, ld = out(c, f32, route)
    gemm(c, C, ld, 'F32', integer=True, alpha=alpha)
    assert S.intact(Cf, M, Nn)
    bad = (C != want).nonzero()
    assert bad.numel() == 0, (bad.shape[0], bad[:8].tolist())
    Cf, C, ld = out(c, f32, route)
    C.copy_(c.c0)
    gemm(c, C, ld, 'F32_ACC', integer=True, alpha=alpha)
    assert S.intact(Cf, M, Nn)
    bad = (C != R.epi_f32_acc(want, c.c0)).nonzero()
    assert bad.numel() == 0, (bad.shape[0], bad[:8].tolist())


@pytest.mark.parametrize('splits,slab', [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize('route,a_t,b_t', [('glds', 0, 1), ('g128', 1, 1)])
def test_split_k_atomic_and_slab_exact(route, a_t, b_t, splits, slab):
    """F32_ATOMIC at ragged M and N into a guarded C (and, in the dW layout, the fused a_rowsum into a guarded vector),
    by float atomics and by the slab form (the slab NaN before the launch: a slice that stored nothing shows). K = 200
    in 3 slices: 96 + 96 + 8 on the LDS-DMA kernel, 128 + 72 + an empty slice on the BK-64 kernel."""
    M, Nn, Kk = R.ATOMIC_SHAPE
    c = case(M, Nn, Kk, a_t, b_t)
    assert_route(route, c, 'F32_ATOMIC', splits=splits, slab=slab, a_rowsum=bool(a_t))
    Cf, C, ld = out(c, f32)
    C.copy_(c.c0)
    rf, rs = S.flat(M, fill=2.0)
    sf, sl = S.flat(splits * M * Nn, fill=NAN) if slab else (None, None)
    gemm(c, C, ld, 'F32_ATOMIC', integer=True, splits=splits, a_rowsum=rs if a_t else None, aux=sl)
    assert S.intact(Cf, M, Nn) and S.intact(rf) and (sf is None or S.intact(sf))
    want = R.epi_f32_atomic((c.Ai.double() @ c.Wi.double().t()).float(), c.c0)
    bad = (C != want).nonzero()
    assert bad.numel() == 0, (bad.shape[0], bad[:8].tolist())
    if a_t:
        assert torch.equal(rs, 2.0 + c.Ai.float().sum(-1))
    else:
        assert bool((rs == 2.0).all())


def test_split_k_slab_on_gemm256_exact():
    """The slab form where it reaches gemm256 (195 blocks; 13 slices of one K-tile, the last 56 deep), with the fused
    row sums of the first two column tiles."""
    M, Nn, Kk, splits = R.SLAB_G256
    c = case(M, Nn, Kk, 1, 1)
    assert_route('g256', c, 'F32_ATOMIC', persistent=False, splits=splits, slab=True, a_rowsum=True)
    Cf, C, ld = out(c, f32)
    C.copy_(c.c0)
    rf, rs = S.flat(M, fill=2.0)
    sf, sl = S.flat(splits * M * Nn, fill=NAN)
    gemm(c, C, ld, 'F32_ATOMIC', integer=True, splits=splits, a_rowsum=rs, aux=sl)
    assert S.intact(Cf, M, Nn) and S.intact(rf) and S.intact(sf)
    bad = (C != R.epi_f32_atomic((c.Ai.double() @ c.Wi.double().t()).float(), c.c0)).nonzero()
    assert bad.numel() == 0, (bad.shape[0], bad[:8].tolist())
    assert torch.equal(rs, 2.0 + c.Ai.float().sum(-1))


# ================================================================================================ batch
@pytest.mark.parametrize('route,M,Nn,Kk,batch', R.BATCH_CASES)
def test_batch_strides(route, M, Nn, Kk, batch):
    """batch > 1 with sA, sB, sC larger than the matrices (the gaps of A and B hold 1e30, the gaps between the batches
    of C sentinels): BF16 with bias and F32, per element; on gemm256 the batch is tile_coords' z of 192 tiles."""
    c = case(M, Nn, Kk, 0, 0, batch)
    for epi in ('BF16', 'F32'):
        r = assert_route(route, c, epi)
    if route == 'g256':
        assert r[1:] == (192, False)
    sA, sB = M * Kk + 64, Nn * Kk + 128
    A = torch.full((batch, sA), PAD, dtype=bf16, device=dev)
    B = torch.full((batch, sB), PAD, dtype=bf16, device=dev)
    A[:, :M * Kk] = c.A.reshape(batch, -1)
    B[:, :Nn * Kk] = c.W.reshape(batch, -1)
    ref, sc = R.gemm(c.A, c.W, ALPHA)
    ld, rows = ld_of(Nn), M + S.XROWS
    for epi, dt in (('BF16', bf16), ('F32', f32)):
        full, _ = S.matrix(batch * rows - S.XROWS, Nn, ld, dt, fill=NAN)
        full3 = full.view(batch, rows, ld)
        full3[:, M:] = S.SENTINEL                                        # the rows between two batches of C
        C = full3[:, :M, :Nn]
        K.gemm(A, B, C, M, Nn, Kk, ldc=ld, epi=getattr(N, 'EPI_' + epi), bias=c.bias if epi == 'BF16' else None,
               alpha=ALPHA, batch=batch, sA=sA, sB=sB, sC=rows * ld)
        torch.cuda.synchronize()
        s = torch.tensor(S.SENTINEL, dtype=dt)
        assert bool((full3[:, M:] == s).all()) and bool((full3[:, :, Nn:] == s).all())
        tag = f'{route} batch {batch} x {M}x{Nn}x{Kk} {epi}'
        if epi == 'BF16':
            ratio(tag, R.bf16_excess(C, R.epi_bf16(ref, c.bias), R.bound('f32'), sc + c.bias.abs()))
        else:
            report(tag, R.deviation(C, ref, sc), R.bound('acc'))


# ================================================================================================ rotary
@pytest.mark.parametrize('route,M,Nn,Kk,a_t,b_t,rot_d,rot_cols,rot_seq', R.ROTARY_CASES)
def test_rotary_per_element(route, M, Nn, Kk, a_t, b_t, rot_d, rot_cols, rot_seq):
    """ROTARY_BF16 per element from the table handed to the kernel: rot_d is no power of two, rot_seq = 40 starts tiles
    mid-sequence and wraps the position inside a fragment column, rot_seq = 5 is below gemm256's 16-row step; the
    columns past rot_cols pass unrotated."""
    c = case(M, Nn, Kk, a_t, b_t)
    assert_route(route, c, 'ROTARY_BF16', persistent=(M == 16420) if route == 'g256' else None)
    tab = rotary_table(rot_seq, rot_d).to(dev)
    Cf, C, ld = out(c, bf16)
    gemm(c, C, ld, 'ROTARY_BF16', bias=c.bias_mod, rot=tab, rot_cols=rot_cols, rot_d=rot_d, rot_seq=rot_seq)
    assert S.intact(Cf, M, Nn)
    ref, sc = R.gemm(c.A, c.W, 1.0, c.bias_mod)
    ref, sr = R.epi_rotary(R.epi_f32(ref, c.bias_mod), tab, rot_cols, rot_d, rot_seq, S=sc)
    ratio(f'{route} {M}x{Nn}x{Kk} lay {a_t}{b_t} ROTARY d {rot_d} seq {rot_seq}', R.bf16_excess(C, ref, R.bound('rotary'), sr))


# ================================================================================================ CE statistics
@pytest.mark.parametrize('route,T,V,Kk,tiles,persistent', R.CE_CASES)
def test_ce_stats_per_row(route, T, V, Kk, tiles, persistent):
    """CE_STATS at a vocabulary that is no multiple of 128 (V % 8 == 4): the logits per element, per row the
    logsumexp over the row's partials and the label's logit (labels in the last valid column, the last 4-column group,
    column 0 and on both sides of tile boundaries), the partials past T untouched, and the statistics-only run
    (C = None, gemm256's non-relaxed first wait) bit-equal to the run that stores the logits."""
    c = case(T, V, Kk)
    r = assert_route(route, c, 'CE_STATS', persistent=persistent if route == 'g256' else None)
    assert r[1] == tiles
    lab = R.ce_labels(T, V).to(dev)
    ntile = -(-V // 128)
    Cf, C, ld = out(c, bf16)
    pf, part = S.flat(T * ntile * 2, fill=NAN)
    lf, ll = S.flat(T, fill=NAN)
    gemm(c, C, ld, 'CE_STATS', bias=c.bias_mod, aux=part, labels=lab, label_logit=ll)
    assert S.intact(Cf, T, V) and S.intact(pf) and S.intact(lf)
    ref, sc = R.gemm(c.A, c.W, 1.0, c.bias_mod)
    logits = R.epi_f32(ref, c.bias_mod)
    lse, lref = R.ce_stats(logits, lab)
    tag = f'{route} CE_STATS {T}x{V}x{Kk}'
    ratio(f'{tag} logits', R.bf16_excess(C, logits, R.bound('ce.logit'), sc))
    report(f'{tag} logsumexp', R.deviation(R.ce_lse_from_partials(part.view(T, ntile, 2)), lse, sc.max(-1).values),
           R.bound('ce.lse'))
    report(f'{tag} label logit', R.deviation(ll, lref, sc.gather(-1, lab.long()[:, None])[:, 0]), R.bound('ce.logit'))
    pf2, part2 = S.flat(T * ntile * 2, fill=NAN)
    lf2, ll2 = S.flat(T, fill=NAN)
    gemm(c, None, ld, 'CE_STATS', bias=c.bias_mod, aux=part2, labels=lab, label_logit=ll2)
    assert S.intact(pf2) and S.intact(lf2)
    assert same_bits(part2, part) and same_bits(ll2, ll)


# ================================================================================================ BF16 + delta
@pytest.mark.parametrize('route,M,Nn,Kk,hd,seq', R.DELTA_CASES)
def test_bf16_delta_per_row_and_head(route, M, Nn, Kk, hd, seq):
    """svae_gemm's delta per (row, head) against float64 of the kernel's own bf16 C times o32 (ld_o32 > N): fused into
    gemm256's epilogue at hd 64 (a wave's columns are one head) and 96 (two), non-persistent and persistent; the
    separate delta kernel behind the skinny and the LDS-DMA kernel. C is bit-equal to the plain BF16 run."""
    c = case(M, Nn, Kk)
    assert_route(route, c, 'BF16', persistent=(M == 21780) if route == 'g256' else None)
    H = Nn // hd
    C0f, C0, ld = out(c, bf16, route)
    gemm(c, C0, ld, 'BF16', bias=c.bias_mod)
    Cf, C, ld = out(c, bf16, route)
    df, d = S.flat(M * H, fill=NAN)
    obuf, o32 = padded(c.resid, Nn + 8)
    gemm(c, C, ld, 'BF16', bias=c.bias_mod, delta=d, delta_o32=obuf, ld_o32=Nn + 8, delta_hd=hd, delta_seq=seq)
    assert S.intact(C0f, M, Nn) and S.intact(Cf, M, Nn) and S.intact(df)
    assert same_bits(C, C0)
    report(f'{route} delta {M}x{Nn} hd {hd}', R.deviation(d, R.delta(C, o32, hd, seq), R.delta(C, o32, hd, seq, absolute=True)),
           R.bound('delta'))
