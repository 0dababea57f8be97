"""The decode kernels (csrc/decode.hip), each called directly and compared with the float64 restatements of
tests/decode_ref.py at the shapes the production decoders use and at the edges of every tile, split and window:

* dec_linear: bit-exact on quarter-integer operands (every summation order gives the float64 result) over the
  m-tile, split-K and ragged-slice ladder, with the split count proved from the workspace; GELU and rotary
  epilogues, un-split and through the finalize kernel, to a few ulp of their own rounding;
* dec_attn: NaN-poisoned caches (a read of any invisible key shows), boundary keys carrying > 5 % of the softmax
  mass, against the float64 softmax over exactly the visible set, for hd 16 / 64 / 96 / 128, dense and windowed;
* dec_embed / dec_penalty / dec_advance;
* dec_sample: support and chi-square against the distribution the REFERENCE samples from
  (tests/golden/gen_sampler.npz through decode_ref.sample_distribution), greedy ties, live bookkeeping;
* sample() at d 512, batch 37: teacher-forced logits of every step against the float64 oracle, graph == eager.

Every bounded comparison prints its worst err / bound (run with -s to see them).
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import decode_ref as R  # noqa: E402
import oracle  # noqa: E402
from oracle.params import HParams, TIED_ALIASES, init_params  # noqa: E402
from golden_util import load  # noqa: E402

if torch.cuda.is_available():
    from sparse_vae import TransformerVAE, TransformerVAEHparams
    from sparse_vae import kernels as K
    from sparse_vae._native import EPI_F32, EPI_GELU, EPI_ROTARY_BF16
    from sparse_vae.core.generation import GenerationState
    from sparse_vae.decoding import KVDecoder
    from sparse_vae.engine import rotary_table

f32 = torch.float32
POISON = 0x7FC0BEEF          # a quiet NaN with a payload: untouched cells are recognised bit for bit


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device='cuda').view(f32)


def cur_tensor(c):
    return torch.tensor([c], dtype=torch.int32, device='cuda')


# ============================================================================================== dec_linear
def finite_slabs(part, M, N):
    """How many leading-dimension-M*N slabs of the NaN-filled workspace came back fully finite."""
    n = part.numel() // (M * N)
    return int(torch.isfinite(part[:n * M * N].view(n, M * N)).all(dim=1).sum().item())


def run_linear(M, N, Kd, *, seed, part_elems=None, epi=None, bias=True, resid=False, **kw):
    """Quarter-integer operands -> (Y f32 [M, N] on the host, float64 pre-activation + resid, finite slab count)."""
    X, W = R.quarter_ints((M, Kd), seed), R.quarter_ints((N, Kd), seed + 1)
    b = R.quarter_ints((N,), seed + 2) if bias else None
    r = R.quarter_ints((M, N), seed + 3) if resid else None
    Y = poisoned(M, N)
    part = None
    if part_elems:
        part = torch.full((part_elems,), float('nan'), device='cuda')
    K.dec_linear(dev(X), dev(W), Y, M, N, Kd, bias=None if b is None else dev(b), resid=None if r is None else dev(r),
                 epi=EPI_F32 if epi is None else epi, part=part, **kw)
    torch.cuda.synchronize()
    slabs = finite_slabs(part, M, N) if part is not None else 0
    return Y.cpu().numpy(), R.linear64(X, W, b, r), slabs


M_EDGES = [(m, 48, 128) for m in (15, 16, 17, 37, 63, 64, 65, 130)]
EXACT_SHAPES = [(1, 16, 4), (3, 40, 20), (5, 37, 68)] + M_EDGES + [
    (37, 128, 512), (37, 128, 1024), (64, 512, 2048), (37, 128, 4096),      # 2, 4, 8, 16 splits
    (37, 128, 520), (5, 136, 2056),                                          # ragged last K-slice
    (3, 32768, 128),                                                         # the vocabulary head: never splits
]
EXPECTED_SPLITS = {(37, 128, 512): 2, (37, 128, 1024): 4, (64, 512, 2048): 8, (37, 128, 4096): 16}


@pytest.mark.parametrize('shape', EXACT_SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_dec_linear_exact_on_quarter_integers(shape):
    M, N, Kd = shape
    part_elems = 16 * M * N
    splits = R.split_count(M, N, Kd, part_elems)
    if shape in EXPECTED_SPLITS:
        assert splits == EXPECTED_SPLITS[shape]
    Y, ref, slabs = run_linear(M, N, Kd, seed=sum(shape), part_elems=part_elems, resid=True)
    assert slabs == (splits if splits > 1 else 0), f'{slabs} finite partial slabs, the rule gives {splits} splits'
    assert np.array_equal(Y.astype(np.float64), ref)


def test_dec_linear_no_workspace_wide_output():
    Y, ref, _ = run_linear(64, 1536, 512, seed=11, resid=True)
    assert np.array_equal(Y.astype(np.float64), ref)


def test_dec_linear_workspace_fallbacks_agree():
    """(64, 512, 2048): 8 splits with room, 2 with a workspace of exactly 2 M N floats, none without one."""
    M, N, Kd = 64, 512, 2048
    out = []
    for elems, want in ((16 * M * N, 8), (2 * M * N, 2), (None, 1)):
        assert R.split_count(M, N, Kd, elems or 0) == want
        Y, ref, slabs = run_linear(M, N, Kd, seed=5, part_elems=elems, resid=True)
        assert slabs == (want if want > 1 else 0)
        assert np.array_equal(Y.astype(np.float64), ref)
        out.append(Y)
    assert np.array_equal(out[0].view(np.int32), out[1].view(np.int32))
    assert np.array_equal(out[0].view(np.int32), out[2].view(np.int32))


@pytest.mark.parametrize('shape,split', [((5, 37, 68), False), ((37, 130, 520), True)])
def test_dec_linear_leading_dimensions_and_padding(shape, split):
    M, N, Kd = shape
    ldx, ldw, ldy, ldr = Kd + 8, Kd + 4, N + 3, N + 7
    X, W = R.quarter_ints((M, Kd), 21), R.quarter_ints((N, Kd), 22)
    b, r = R.quarter_ints((N,), 23), R.quarter_ints((M, N), 24)
    Xp, Wp, rp, Y = poisoned(M, ldx), poisoned(N, ldw), poisoned(M, ldr), poisoned(M, ldy)
    Xp[:, :Kd], Wp[:, :Kd], rp[:, :N] = dev(X), dev(W), dev(r)
    part = torch.full((16 * M * N,), float('nan'), device='cuda') if split else None
    K.dec_linear(Xp, Wp, Y, M, N, Kd, bias=dev(b), resid=rp, ldx=ldx, ldw=ldw, ldy=ldy, ldr=ldr, part=part)
    torch.cuda.synchronize()
    if split:
        assert finite_slabs(part, M, N) == R.split_count(M, N, Kd, part.numel()) == 2
    assert np.array_equal(Y[:, :N].cpu().numpy().astype(np.float64), R.linear64(X, W, b, r))
    assert (Y[:, N:].contiguous().view(torch.int32) == POISON).all(), 'padding columns of Y were written'


EPI_SHAPES = [((37, 128, 512), None, 1), ((37, 128, 512), 16 * 37 * 128, 2),
              ((64, 1536, 512), None, 1), ((64, 1536, 512), 16 * 64 * 1536, 2)]
EPI_IDS = ['37x128x512-unsplit', '37x128x512-split2', '64x1536x512-unsplit', '64x1536x512-split2']


@pytest.mark.parametrize('shape,part_elems,want', EPI_SHAPES, ids=EPI_IDS)
def test_dec_linear_gelu_epilogue(shape, part_elems, want):
    """|y - gelu64(x)| <= 4 * 2^-24 * |x|: the pre-activation x is exact, erff is good to a couple of ulp of 1 and
    the factor is 0.5 |x| (which also covers the 1 + erf cancellation at negative x)."""
    M, N, Kd = shape
    assert R.split_count(M, N, Kd, part_elems or 0) == want
    Y, pre, slabs = run_linear(M, N, Kd, seed=31, part_elems=part_elems, epi=EPI_GELU)
    assert slabs == (want if want > 1 else 0)
    err, bound = np.abs(Y.astype(np.float64) - R.gelu64(pre)), 4 * R.EPS24 * np.abs(pre)
    assert np.isfinite(Y).all()
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f'gelu {shape} splits {want}: worst err / bound = {ratio:.3f}, |x| up to {np.abs(pre).max():.1f}')
    assert (err <= bound).all(), ratio


@pytest.mark.parametrize('cur', [1, 2, 100])
@pytest.mark.parametrize('shape,part_elems,want', EPI_SHAPES, ids=EPI_IDS)
def test_dec_linear_rotary_epilogue(shape, part_elems, want, cur):
    """Columns < rot_cols = 2 d are rotated pairwise by the f32 table row cur - 1, |err| <= 3 * 2^-24 * (|a cos| +
    |b sin|) (two products and a sum, or an fma and a product); columns >= rot_cols pass through exactly; cur = 1
    is the identity row (cos 1, sin 0)."""
    M, N, Kd = shape
    d = N // 3 // 2 * 2                      # q | k rotated, the rest (v, and the odd columns of N = 128) not
    rot = rotary_table(128, d)
    assert R.split_count(M, N, Kd, part_elems or 0) == want
    Y, pre, slabs = run_linear(M, N, Kd, seed=41, part_elems=part_elems, epi=EPI_ROTARY_BF16, rot=rot.cuda(),
                               rot_cols=2 * d, rot_d=d, cur=cur_tensor(cur))
    assert slabs == (want if want > 1 else 0)
    ref, mag = R.rotary64(pre, rot.numpy(), cur - 1, 2 * d, d)
    Y = Y.astype(np.float64)
    assert np.array_equal(Y[:, 2 * d:], pre[:, 2 * d:])
    if cur == 1:
        assert np.array_equal(Y, pre)
    err, bound = np.abs(Y - ref)[:, :2 * d], 3 * R.EPS24 * mag[:, :2 * d]
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f'rotary {shape} splits {want} cur {cur}: worst err / bound = {ratio:.3f}')
    assert (err <= bound).all(), ratio
    if cur > 1:
        assert np.abs(ref - pre)[:, :2 * d].max() > 1.0      # the rotation is not a no-op at this row


# ============================================================================================== dec_attn
ATTN_HEADS = {16: 5, 64: 3, 96: 2, 128: 4}       # hd -> H (d <= 512, H not a power of two where it can be)
DENSE_P = (0, 1, 31, 32, 63, 64, 1023, 1024, 1500)
WINDOW_P = (0, 31, 32, 95, 96, 97, 127, 128, 200, 1100)


def run_attn(B, H, hd, T, p, window, seed):
    """One dec_attn call on NaN-poisoned caches. Returns the worst err / bound over all outputs."""
    rng = np.random.default_rng(seed)
    d, scale = H * hd, hd ** -0.5
    vis = R.visible_keys(p, window)
    old = vis[vis < p]                                       # visible keys that live in the cache
    lo2 = max(32, (p // 32 - (window - 1)) * 32) if window > 0 else 0
    n1 = min(p + 1, 32) if window > 0 else p + 1
    boundary = sorted({j for j in (0, n1 - 1, lo2, p - 1, p) if 0 <= j <= p and j in set(vis.tolist())})
    q = rng.standard_normal((B, H, hd)).astype(np.float32)
    kc = np.full((B, H, T, hd), np.nan, dtype=np.float32)
    vc = np.full((B, H, T, hd), np.nan, dtype=np.float32)
    kc[:, :, old] = 0.5 * rng.standard_normal((B, H, old.size, hd)).astype(np.float32)
    vc[:, :, old] = rng.standard_normal((B, H, old.size, hd)).astype(np.float32)
    kp = 0.5 * rng.standard_normal((B, H, hd)).astype(np.float32)
    vp = rng.standard_normal((B, H, hd)).astype(np.float32)
    # boundary keys k = alpha q with score s_b = scale alpha |q|^2: the other keys' scores have std ~0.5, mass
    # ~1.13 each; exp(s_b) = an eighth of their total gives each of the <= 5 boundary keys >= 1/13 of the softmax
    s_b = max(1.0, math.log(max(vis.size, 1) * 1.13 / 8.0))
    alpha = (s_b / (scale * (q.astype(np.float64) ** 2).sum(-1))).astype(np.float32)[..., None]
    for j in boundary:
        if j == p:
            kp = alpha * q
        else:
            kc[:, :, j] = alpha * q
    qkv = np.concatenate([a.reshape(B, d) for a in (q, kp, vp)], axis=1)
    kc_d, vc_d, O = dev(kc), dev(vc), poisoned(B, d)
    kc0, vc0 = kc_d.clone(), vc_d.clone()
    K.dec_attn(dev(qkv), kc_d, vc_d, O, B, H, hd, T, cur_tensor(p + 1), window)
    torch.cuda.synchronize()
    # cache append: position p holds the k | v slices bit for bit, every other cell keeps its bit pattern
    assert torch.equal(kc_d[:, :, p].view(torch.int32), dev(kp).view(torch.int32))
    assert torch.equal(vc_d[:, :, p].view(torch.int32), dev(vp).view(torch.int32))
    keep = torch.ones(T, dtype=torch.bool, device='cuda')
    keep[p] = False
    assert torch.equal(kc_d[:, :, keep].view(torch.int32), kc0[:, :, keep].view(torch.int32))
    assert torch.equal(vc_d[:, :, keep].view(torch.int32), vc0[:, :, keep].view(torch.int32))
    kc[:, :, p], vc[:, :, p] = kp, vp
    got = O.cpu().numpy().reshape(B, H, hd).astype(np.float64)
    assert np.isfinite(got).all(), 'an invisible (NaN) key or value was read'
    worst, min_mass = 0.0, 1.0
    for b in range(B):
        for h in range(H):
            ref, A, S, spread = R.attn64(q[b, h], kc[b, h, vis], vc[b, h, vis], scale)
            assert spread <= 16.0, spread            # the bound's fast-exponential term assumes this
            s = scale * (kc[b, h, vis].astype(np.float64) @ q[b, h].astype(np.float64))
            pr = np.exp(s - s.max())
            pr /= pr.sum()
            min_mass = min(min_mass, min(pr[np.searchsorted(vis, j)] for j in boundary))
            worst = max(worst, float((np.abs(got[b, h] - ref) / R.attn_bound(A, S, vis.size, hd)).max()))
    assert min_mass >= 0.05, min_mass
    return worst


@pytest.mark.parametrize('window', [0, 1, 2, 4])
@pytest.mark.parametrize('hd', [16, 64, 96, 128])
def test_dec_attn_visible_set_and_bound(hd, window):
    H = ATTN_HEADS[hd]
    ratios = {}
    for p in (DENSE_P if window == 0 else WINDOW_P):
        ratios[p] = run_attn(3, H, hd, p + 3, p, window, seed=1000 * hd + 10 * window + p)
    print(f'dec_attn hd {hd} window {window}: err / bound per p = ' +
          ', '.join(f'{p}: {r:.3f}' for p, r in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios


def test_dec_attn_at_the_documented_length_limit():
    """T = 32768 (128 KiB of dynamic LDS), 20001 visible keys: twenty trips of the strided score loop."""
    r = run_attn(1, 1, 16, 32768, 20000, 0, seed=9)
    print(f'dec_attn T 32768 p 20000: err / bound = {r:.3f}')
    assert r <= 1.0, r


# ============================================================================================== embed / penalty
@pytest.mark.parametrize('cur', [1, 7])
@pytest.mark.parametrize('D', [128, 520])
@pytest.mark.parametrize('B', [1, 4, 5, 64])
def test_dec_embed_exact_gather(B, D, cur):
    g = torch.Generator().manual_seed(B * D + cur)
    V, T = 300, 9
    table = torch.randn(V, D, generator=g).cuda()
    ids = torch.randint(0, V, (B, T), generator=g).cuda()
    x = poisoned(B + 1, D)
    K.dec_embed(ids, T, cur_tensor(cur), table, x, B, D)
    torch.cuda.synchronize()
    assert torch.equal(x[:B], table[ids[:, cur - 1]])
    assert (x[B].view(torch.int32) == POISON).all()


def test_dec_penalty_window_moves_with_cur():
    """T 700, cur 600: the window is positions 88..599. The token at position t is 1000 + t (so each sits at one
    position only) except token 50 at positions 200 and 300. Logits rows map to sequences through row_map;
    sequence 3 is dead."""
    T, cur, V, B, pen = 700, 600, 2000, 6, 1.3
    g = torch.Generator().manual_seed(12)
    ids = (1000 + torch.arange(T)).repeat(B, 1)
    ids[:, 200] = ids[:, 300] = 50
    ids[:, cur:] = 1999                                   # not generated yet: never read
    row_map = torch.tensor([0, 2, 3, 5], dtype=torch.int32)
    live = torch.tensor([1, 1, 1, 0, 1, 1], dtype=torch.bool)
    logits = torch.randn(4, V, generator=g) * 3
    logits[0, 1087], logits[0, 1088], logits[0, 50] = 2.5, 2.5, -1.75         # both signs at each probe
    logits[1, 1087], logits[1, 1088], logits[1, 50] = -2.5, -2.5, 1.75
    ref = logits.clone()
    for r in (0, 1, 3):                                   # row 2 -> sequence 3 is dead
        prev = ids[row_map[r].long(), cur - 512:cur]
        pl = ref[r].gather(-1, prev)
        ref[r].scatter_(-1, prev, torch.where(pl < 0, pl * pen, pl / pen))
    out = logits.clone().cuda()
    K.dec_penalty(out, 4, row_map.cuda(), ids.cuda(), T, cur_tensor(cur), live.cuda(), pen)
    torch.cuda.synchronize()
    out = out.cpu()
    touched = torch.zeros(4, V, dtype=torch.bool)
    for r in (0, 1, 3):
        touched[r, ids[row_map[r].long(), 88:cur]] = True
    assert torch.equal(out[~touched].view(torch.int32), logits[~touched].view(torch.int32))
    assert torch.equal(out[2], logits[2])
    assert (out[touched] != logits[touched]).all()
    torch.testing.assert_close(out, ref, rtol=2.0 ** -23, atol=0.0)
    pen = float(np.float32(pen))                          # the factor as the kernel and torch see it
    for r, sign in ((0, 1.0), (1, -1.0)):
        assert out[r, 1087] == logits[r, 1087]                                    # position 87: outside
        assert abs(out[r, 1088] - 2.5 * sign / (pen ** sign)) <= 2.0 ** -23 * 2.5 * pen   # position 88: inside
        once = logits[r, 50] * pen if logits[r, 50] < 0 else logits[r, 50] / pen  # twice inside: penalised once
        assert abs(out[r, 50] - once) <= 2.0 ** -23 * abs(once)


def test_dec_advance():
    c = cur_tensor(41)
    K.dec_advance(c)
    K.dec_advance(c)
    assert c.item() == 43


# ============================================================================================== dec_sample
RANK_CONFIG = 3
N_ROWS, N_LAUNCH = 4096, 4


@functools.lru_cache(maxsize=None)
def sampler_fixture():
    g = load('gen_sampler')
    return g, [(int(k), float(p), float(t)) for k, p, t in g['configs']]


def sample_rows(row, top_k, top_p, temperature, seed, rows=N_ROWS):
    """`rows` copies of one logits row through one dec_sample launch -> the emitted ids."""
    V = row.size
    logits = dev(row).repeat(rows, 1)
    T = 4
    out = torch.full((rows, T), -7, dtype=torch.int64, device='cuda')
    K.dec_sample(logits, V, rows, None, out, T, cur_tensor(1), None, -1, temperature, top_k, top_p, seed)
    torch.cuda.synchronize()
    assert (out[:, [0, 2, 3]] == -7).all()
    return out[:, 1].cpu().numpy()


@functools.lru_cache(maxsize=None)
def fixture_draws(c, key, r):
    g, cfgs = sampler_fixture()
    row = g['logits_wide' if key == 'w' else 'logits'][r]
    return np.concatenate([sample_rows(row, *cfgs[c], seed=7919 * (s + 1) + 31 * c + r) for s in range(N_LAUNCH)])


def reference_support(c, key, r):
    """The ids the REFERENCE can emit for this row. The (40, 0.7, 0.8) rows at V 2000 are matched by rank (the
    forced column): what the reference's torch build emitted there is its topk's nth_element order (see
    test_decode_ref.test_rank_emission_at_v2000_matches_reference_by_rank)."""
    g, _ = sampler_fixture()
    o = g[f'offsets{c}{key}']
    which = 'cols' if (c == RANK_CONFIG and key == '') else 'ids'
    return np.sort(g[f'{which}{c}{key}'][int(o[r]):int(o[r + 1])].astype(np.int64))


SAMPLER_CASES = [(c, '', r) for c in range(5) for r in range(4)] + [(RANK_CONFIG, 'w', r) for r in range(2)]
SAMPLER_IDS = [f'cfg{c}{k}-row{r}' for c, k, r in SAMPLER_CASES]


@pytest.mark.parametrize('c,key,r', SAMPLER_CASES, ids=SAMPLER_IDS)
def test_dec_sample_support_is_the_references(c, key, r):
    draws = fixture_draws(c, key, r)
    support = reference_support(c, key, r)
    assert np.isin(draws, support).all(), np.setdiff1d(draws, support)[:8]


def check_chi2(logits_row, cfg, draws, tag):
    ids, p = R.sample_distribution(logits_row, *cfg)
    chi2, nu = R.chi2_binned(ids, p, draws)
    if nu == 0:
        print(f'dec_sample {tag}: one bin, chi2 {chi2}')
        assert chi2 == 0.0
        return
    thr = R.chi2_threshold(nu)
    print(f'dec_sample {tag}: chi2 {chi2:.1f} with {nu} degrees of freedom, threshold {thr:.1f}')
    assert chi2 <= thr, (chi2, nu, thr)


@pytest.mark.parametrize('c,key,r', SAMPLER_CASES, ids=SAMPLER_IDS)
def test_dec_sample_distribution_chi2(c, key, r):
    g, cfgs = sampler_fixture()
    row = g['logits_wide' if key == 'w' else 'logits'][r]
    check_chi2(row, cfgs[c], fixture_draws(c, key, r), f'cfg {cfgs[c]} V {row.size} row {r}')


@pytest.mark.parametrize('V', [1000, 5000])
def test_dec_sample_vocabulary_tails(V):
    """V not a multiple of 1024: the partial last column of the sampler's (column, thread) layout."""
    cfg = (0, 0.9, 0.8)
    row = (2.0 * np.random.default_rng(V).standard_normal(V)).astype(np.float32)
    assert R.nucleus_margin(row, *cfg) > 1e-6
    draws = np.concatenate([sample_rows(row, *cfg, seed=104729 * (s + 1) + V) for s in range(N_LAUNCH)])
    ids, _ = R.sample_distribution(row, *cfg)
    assert np.isin(draws, ids).all()
    check_chi2(row, cfg, draws, f'cfg {cfg} V {V}')


@pytest.mark.parametrize('temperature,top_k', [(0.0, 0), (0.8, 1)])
@pytest.mark.parametrize('V', [1000, 5000, 32768])
def test_dec_sample_greedy_edges(V, temperature, top_k):
    rng = np.random.default_rng(V)
    logits = rng.standard_normal((4, V)).astype(np.float32)
    logits[0, 0] = 9.0                                   # maximum at index 0
    logits[1, V - 1] = 9.0                               # ... at V - 1
    logits[2, [V // 3, V - 2]] = 9.0                     # duplicated: the lower index wins
    logits[3, [V - 1, 1025 % V]] = 9.0                   # duplicated across columns of the layout
    want = [0, V - 1, V // 3, min(V - 1, 1025 % V)]
    out = torch.full((4, 3), -7, dtype=torch.int64, device='cuda')
    K.dec_sample(dev(logits), V, 4, None, out, 3, cur_tensor(1), None, -1, temperature, top_k, 0.9, 5)
    assert out[:, 1].tolist() == want


def test_dec_sample_live_bookkeeping():
    """Rows map to sequences; a row that emits end_token, or writes the last position, clears its live flag and
    takes one off live_count; a dead sequence is skipped and its output_ids stay as they were."""
    B, T, V, end = 8, 6, 1000, 17
    row_map = torch.tensor([1, 2, 4, 6, 7], dtype=torch.int32, device='cuda')
    logits = torch.full((5, V), -5.0)
    for r, tok in enumerate((3, end, 5, 8, end)):
        logits[r, tok] = 4.0
    live = torch.ones(B, dtype=torch.bool, device='cuda')
    live[4] = False
    count = torch.tensor([7], dtype=torch.int32, device='cuda')
    out = torch.full((B, T), -7, dtype=torch.int64, device='cuda')
    K.dec_sample(logits.cuda(), V, 5, row_map, out, T, cur_tensor(2), live, end, 0.0, 0, 0.9, 1, count)
    assert out[:, 2].tolist() == [-7, 3, end, -7, -7, -7, 8, end]
    assert (out[:, [0, 1, 3, 4, 5]] == -7).all()
    assert live.tolist() == [True, True, False, True, False, True, True, False]
    assert count.item() == 5
    # the last position: cur + 1 >= T stops every live row
    K.dec_sample(logits.cuda(), V, 5, row_map, out, T, cur_tensor(T - 1), live, end, 0.0, 0, 0.9, 1, count)
    assert out[:, T - 1].tolist() == [-7, 3, -7, -7, -7, -7, 8, -7]
    assert live.tolist() == [True, False, False, True, False, True, False, False]
    assert count.item() == 3


# ============================================================================================== sample()
MODEL = dict(d_model=512, num_heads=8, num_layers=4)
MODEL_SEED = 77


@functools.lru_cache(maxsize=None)
def model_params():
    return init_params(HParams(latent_depth=64, kl_weight=1.0, **MODEL), MODEL_SEED)


@functools.lru_cache(maxsize=None)
def model(window):
    mhp = TransformerVAEHparams(latent_depth=64, sparse_self_attention=bool(window), attn_window_size=window or 4,
                                kl_weight=1.0, **MODEL)
    m = TransformerVAE(mhp, device='cuda')
    params = model_params()
    sd = dict(params)
    for alias in TIED_ALIASES:
        sd[alias] = params['input_layer.0.weight']
    m.load_state_dict(sd, strict=True)
    m.eval()
    m.start_token, m.end_token = 1, -1
    return m


def latent(B):
    g = torch.Generator().manual_seed(B)
    return torch.randn(B, 1, 64, generator=g)


@pytest.mark.parametrize('window,B,T', [(0, 37, 40), (2, 17, 140)], ids=['dense-B37-T40', 'window2-B17-T140'])
def test_decode_step_logits_match_float64_oracle(window, B, T):
    """Eager KVDecoder steps, the logits of every step kept; then one causal float64 pass of the oracle over the
    ids the GPU produced (teacher forcing) gives every step's reference logits. e_ref = max |f32 pass - f64 pass|
    is the reference's own f32 noise; the GPU must stay within 8 e_ref at every step (16 waves x up to 16 splits
    against BLAS blocking: another summation order, not another precision)."""
    m, z = model(window), latent(B)
    st = GenerationState(T, B, 1, -1, device='cuda', temperature=0.0, repetition_penalty=1.0)
    dec = KVDecoder(m._require_engine(), st, z.cuda(), use_graph=False)
    steps = []
    dec._step(first=True)
    st.step_done()
    steps.append(dec.logits.clone())
    while st.current_index < T - 1:
        dec._step(first=False)
        st.step_done()
        steps.append(dec.logits.clone())
    torch.cuda.synchronize()
    n = len(steps)
    assert n == T - 2
    ids = st.output_ids.cpu()
    assert (ids[:, 1:n + 1] >= 0).all() and (ids[:, n + 1:] == 0).all()
    hp = HParams(latent_depth=64, kl_weight=1.0, attn_window=window, **MODEL)
    p32 = model_params()
    p64 = {k: v.double() for k, v in p32.items()}
    worst_gpu, e_ref = np.zeros(n), 0.0
    for b0 in range(0, B, 8):                      # a few sequences at a time: [8, T, 32768] float64 logits
        sl = slice(b0, min(B, b0 + 8))
        with torch.no_grad():
            x32 = torch.nn.functional.embedding(ids[sl, :n], p32['input_layer.0.weight'])
            l32 = oracle.reconstruct(p32, x32, z[sl], None, hp)
            l64 = oracle.reconstruct(p64, x32.double(), z[sl].double(), None, hp)
        e_ref = max(e_ref, float((l32.double() - l64).abs().max()))
        gpu = torch.stack([s[sl] for s in steps], dim=1).cpu().double()          # [rows, steps, V]
        worst_gpu = np.maximum(worst_gpu, (gpu - l64).abs().amax(dim=(0, 2)).numpy())
        # the ids the GPU chose are the float64 argmax wherever the top-2 margin exceeds the allowed error
        top2 = l64.topk(2, dim=-1)
        clear = (top2.values[..., 0] - top2.values[..., 1]) > 16 * e_ref
        assert torch.equal(ids[sl, 1:n + 1][clear], top2.indices[..., 0][clear])
    ratio = worst_gpu / e_ref
    print(f'sample() window {window} B {B} T {T}: e_ref {e_ref:.3e}, worst gpu / e_ref {ratio.max():.3f} '
          f'(step {int(ratio.argmax()) + 1}), median {np.median(ratio):.3f}')
    assert (worst_gpu <= 8 * e_ref).all(), (ratio.max(), int(ratio.argmax()) + 1)


@pytest.mark.parametrize('kw', [dict(temperature=0.0), dict(temperature=0.8, top_p=0.9)], ids=['greedy', 'nucleus'])
@pytest.mark.parametrize('window,B,T', [(0, 37, 40), (2, 17, 140)], ids=['dense-B37-T40', 'window2-B17-T140'])
def test_sample_graph_replay_equals_eager_steps(window, B, T, kw):
    """No atomics in the decode arithmetic: the replayed graph and the eager steps give identical ids."""
    m, z = model(window), latent(B).cuda()
    out = []
    for use_graph in (True, False):
        torch.manual_seed(1234)
        out.append(m.sample(T, B, z=z.clone(), use_graph=use_graph, repetition_penalty=1.0, **kw))
    torch.cuda.synchronize()
    assert out[0].shape == (B, T - 1)
    assert torch.equal(out[0], out[1])
    if kw['temperature'] > 0:
        assert out[0][:, :-1].unique().numel() > B        # sampling did not collapse to one id
