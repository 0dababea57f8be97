"""The MMD kernels (csrc/mmd.hip), the three estimators of sparse_vae.core.math_utils, LatentIndex.stats / .mmd and
latent_stats.py on the device, against the float64 restatement of tests/mmd_ref.py computed from the same f32 inputs and
against the reference's recorded f64 values (tests/golden/mmd.npz).

EPS24 = 2^-24 is the unit roundoff of f32 (an instruction accurate to 1 ulp counts as two such roundings). Every bound
counts roundings in that unit from the arithmetic and the summation order written in the header of csrc/mmd.hip:

  pairsum   d2: (Z + 3) roundings relative to d2 (Z_ROUNDINGS below: 2 from squaring the rounded difference, at most
            Z / 2 + 1 on the partial sums of the two fmaf chains and their final addition; all terms are non-negative).
            v = d2 + offset: 1, relative to |v|. A term's relative error from those is the count times its
            sensitivity: a d2 and a |v| for exp(-a v); d2 / (s + v) and |v| / (s + v) for s / (s + v).
            RBF: the exponent fl(-a log2 e) * v adds 2 relative to a |v| (so 3 with v's own); v_exp_f32 is 1 ulp: 2
            relative to the term. IMQ: the sum s + v 1, v_rcp_f32 1 ulp = 2, the product 1: 4 relative to the term.
            A term is then added in f32 within one tile of 32 columns: at most 31 additions, each one rounding relative
            to a partial sum of non-negative terms: 31 relative to the sum of the terms. Everything after that is
            f64, chains of at most a few thousand additions: under 1 more in all.
            -> RBF_EXTRA = (3, 2 + 31 + 1), IMQ_EXTRA = (1, 4 + 31 + 1).
  rowterm, colstats, draw: beside their tests (mmd_ref.rowterm_bound holds the first)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mmd_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS24 = 2.0 ** -24
EPS53 = 2.0 ** -53
RBF_EXTRA = (3, 2 + 31 + 1)
IMQ_EXTRA = (1, 4 + 31 + 1)
TILE = 32                     # SVAE_PAIRSUM_TILE_COLS


def z_roundings(Z):
    return Z + 3


def rows_per_block(Z):
    return 512 if Z <= 64 else 256


def dev():
    return torch.device('cuda', 0)


def gpu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- the sizes, from the kernel's own constants -----------------------------------------------------------------------
# 33: one column more than a tile. rows_per_block + 1: one row more than a workgroup owns (513 for Z <= 64, 257 above).
# 2 * rows_per_block + 1: the smallest N with three block rows of the triangular enumeration (1025 / 513).
# 2049: the smallest N at which a workgroup goes round its column-tile loop twice (65 tiles, at most 64 slices, so a
# slice is two tiles). test_geometry_of_the_cases checks all of this against the library.
N_LOOP = 2049


def tri_sizes(Z):
    rb = rows_per_block(Z)
    return [2, 3, 63, 64, 65, TILE + 1, rb + 1, 2 * rb + 1, N_LOOP]


RECT_M = [1, 1000, TILE + 1]


@pytest.mark.parametrize('Z', [4, 64, 68, 128, 256])
def test_geometry_of_the_cases(Z):
    from sparse_vae import _native, kernels as K
    assert _native.PAIRSUM_TILE_COLS == TILE
    rb = rows_per_block(Z)
    for n in tri_sizes(Z):
        g_rb, row_blocks, slices, slice_cols, tile = K.pairsum_geometry(n, n, Z, True)
        assert (g_rb, tile) == (rb, TILE) and row_blocks == -(-n // rb) and slice_cols % TILE == 0
        assert slices * slice_cols >= n > (slices - 1) * slice_cols
    assert K.pairsum_geometry(rb + 1, rb + 1, Z, True)[1] == 2 and K.pairsum_geometry(rb, rb, Z, True)[1] == 1
    assert K.pairsum_geometry(2 * rb + 1, 2 * rb + 1, Z, True)[1] == 3 and K.pairsum_geometry(2 * rb, 2 * rb, Z, True)[1] == 2
    assert K.pairsum_geometry(N_LOOP, N_LOOP, Z, True)[3] == 2 * TILE        # two tiles per slice ...
    assert K.pairsum_geometry(N_LOOP - 1, N_LOOP - 1, Z, True)[3] == TILE     # ... and one just below
    assert K.pairsum_geometry(65, N_LOOP, Z, False)[3] == 2 * TILE
    assert K.pairsum_geometry(N_LOOP, 1000, Z, False)[3] == TILE and K.pairsum_geometry(N_LOOP, TILE + 1, Z, False)[2] == 2


# ---- exact counts ----------------------------------------------------------------------------------------------------
def two_sites(n, Z, seed):
    """Rows on one of two sites at squared distance exactly 1."""
    site = np.random.default_rng(seed).integers(0, 2, n)
    x = np.zeros((n, Z), np.float32)
    x[:, Z - 1] = site
    return x, site


@pytest.mark.parametrize('Z', [4, 64, 68, 128, 256])
def test_exact_counts_triangular(Z):
    """RBF with all rows identical: every term is exp(0) = 1 and the sum is N (N - 1) / 2. IMQ with s = 1 and every
    row on one of two sites with d2 = 1 = s: the terms are 1 (same site) or 1/2, every f32 partial (at most 32 terms)
    and every f64 sum is exact, so the result is the pair counts. A dropped, doubled or self pair changes an integer."""
    from sparse_vae import kernels as K
    for n in tri_sizes(Z):
        same = gpu(np.full((n, Z), 0.375, np.float32))
        got = K.pairsum(same, kind='rbf', params=[0.25, 3.0])
        assert f64(got).tolist() == [n * (n - 1) / 2] * 2, (n, f64(got))
        x, site = two_sites(n, Z, n)
        n1 = int(site.sum())
        n0 = n - n1
        want = n0 * (n0 - 1) / 2 + n1 * (n1 - 1) / 2 + n0 * n1 / 2
        xt = gpu(x)
        got = K.pairsum(xt, kind='imq', params=[1.0])
        assert f64(got).tolist() == [want], (n, f64(got), want)
        if n == N_LOOP:
            assert torch.equal(got, K.pairsum(xt, kind='imq', params=[1.0]))
            assert torch.equal(K.pairsum(same, kind='rbf', params=[0.25, 3.0]), K.pairsum(same, kind='rbf', params=[0.25, 3.0]))


@pytest.mark.parametrize('Z', [4, 64, 68, 128, 256])
def test_exact_counts_rectangular(Z):
    from sparse_vae import kernels as K
    for n in tri_sizes(Z):
        for m in RECT_M:
            a = gpu(np.full((n, Z), -1.5, np.float32))
            b = gpu(np.full((m, Z), -1.5, np.float32))
            got = K.pairsum(a, b, kind='rbf', params=[0.5])
            assert f64(got).tolist() == [float(n * m)], (n, m)
            x, sx = two_sites(n, Z, n + m)
            y, sy = two_sites(m, Z, n + m + 1)
            same = int(sx.sum()) * int(sy.sum()) + int((1 - sx).sum()) * int((1 - sy).sum())
            want = same + (n * m - same) / 2
            xt, yt = gpu(x), gpu(y)
            got = K.pairsum(xt, yt, kind='imq', params=[1.0])
            assert f64(got).tolist() == [want], (n, m)
            if n == N_LOOP:
                assert torch.equal(got, K.pairsum(xt, yt, kind='imq', params=[1.0]))
    # 65 rows against 2,049 columns: the rectangular grid's slices are two tiles too (checked in the geometry test)
    x, sx = two_sites(65, Z, 1)
    y, sy = two_sites(N_LOOP, Z, 2)
    same = int(sx.sum()) * int(sy.sum()) + int((1 - sx).sum()) * int((1 - sy).sum())
    got = K.pairsum(gpu(x), gpu(y), kind='imq', params=[1.0])
    assert f64(got).tolist() == [same + (65 * N_LOOP - same) / 2]
    assert torch.equal(got, K.pairsum(gpu(x), gpu(y), kind='imq', params=[1.0]))


# ---- random data against the f64 restatement --------------------------------------------------------------------------
def rbf_params(Z):
    return [float(np.float32(4.0 / Z)), float(np.float32(0.5 / Z))]


def check_pairsum(tag, got, want, bound):
    ratio = np.abs(f64(got) - want) / bound
    print(f'{tag}: max err / bound {ratio.max():.4f}')
    assert np.isfinite(f64(got)).all() and ratio.max() <= 1.0, (tag, ratio)


@pytest.mark.parametrize('shift', [0.0, 30.0])
@pytest.mark.parametrize('Z', [4, 16, 64, 68, 256])
def test_random_triangular(Z, shift):
    """N(0, 1) rows, and the same rows + 30 in every coordinate under the SAME bound: distances do not change, and a
    d2 formed from direct differences does not notice (a Gram form |x|^2 + |y|^2 - 2 x.y without centring loses
    (30^2 Z / 2Z) ~ 450 times the precision here and fails)."""
    from sparse_vae import kernels as K
    for n in tri_sizes(Z):
        rng = np.random.default_rng(1000 * Z + n)
        x = (rng.standard_normal((n, Z)) + shift).astype(np.float32)
        xt = gpu(x)
        d2 = R.sqdist(x, x)
        for kind, params, extra in (('rbf', rbf_params(Z), RBF_EXTRA), ('imq', R.imq_scales(Z), IMQ_EXTRA)):
            want, bound = R.pairsum64(x, None, kind, params, None, z_roundings(Z), extra, d2=d2)
            got = K.pairsum(xt, kind=kind, params=params)
            check_pairsum(f'tri {kind} Z {Z} N {n} shift {shift}', got, want, bound)
            assert torch.equal(got, K.pairsum(xt, kind=kind, params=params))


@pytest.mark.parametrize('shift', [0.0, 30.0])
@pytest.mark.parametrize('Z', [4, 16, 64, 68, 256])
def test_random_rectangular(Z, shift):
    """All pairs of two sets, with and without a column offset (uniform in +-0.1 Z: s + v stays above 0.1 Z)."""
    from sparse_vae import kernels as K
    for n in tri_sizes(Z):
        for m in RECT_M:
            rng = np.random.default_rng(1000 * Z + n + 7 * m)
            x = (rng.standard_normal((n, Z)) + shift).astype(np.float32)
            y = (rng.standard_normal((m, Z)) + shift).astype(np.float32)
            off = ((rng.random(m) - 0.5) * 0.2 * Z).astype(np.float32)
            xt, yt, ot = gpu(x), gpu(y), gpu(off)
            d2 = R.sqdist(x, y)
            for kind, params, extra in (('rbf', rbf_params(Z), RBF_EXTRA), ('imq', R.imq_scales(Z), IMQ_EXTRA)):
                for o_np, o_t in ((None, None), (off, ot)):
                    want, bound = R.pairsum64(x, y, kind, params, o_np, z_roundings(Z), extra, d2=d2)
                    got = K.pairsum(xt, yt, kind=kind, params=params, col_off=o_t)
                    check_pairsum(f'rect {kind} Z {Z} N {n} M {m} shift {shift} offset {o_np is not None}', got, want,
                                  bound)


# ---- rowterm, colstats, draw -----------------------------------------------------------------------------------------
# 17: one row more than a workgroup's 16 (one per 16 lanes); 4097: one more than the 256 workgroups x 16 rows of one pass
ROW_N = [1, 16 + 1, 63, 65, 1000, 16 * 256 + 1]


@pytest.mark.parametrize('Z', [4, 64, 256])
@pytest.mark.parametrize('n', ROW_N)
def test_rowterm(n, Z):
    from sparse_vae import _native, kernels as K
    assert _native.MMD_REDUCE_BLOCKS == 256
    rng = np.random.default_rng(n + Z)
    for shift in (0.0, 30.0):
        x = (rng.standard_normal((n, Z)) + shift).astype(np.float32)
        w = (1.0 / (0.125 * Z + rng.random(Z) * 2.0)).astype(np.float32)
        m = (shift + 0.1 * rng.standard_normal(Z)).astype(np.float32)
        for m_np in ((None, m) if shift == 0.0 else (m,)):
            got = K.mmd_rowterm(gpu(x), gpu(w), None if m_np is None else gpu(m_np))
            want, q = R.rowterm64(x, w, m_np)
            bound = R.rowterm_bound(q, Z)
            err = abs(float(got.item()) - want)
            print(f'rowterm N {n} Z {Z} shift {shift} mean {m_np is not None}: err / bound {err / bound:.4f}')
            assert err <= bound
            assert torch.equal(got, K.mmd_rowterm(gpu(x), gpu(w), None if m_np is None else gpu(m_np)))


@pytest.mark.parametrize('Z', [4, 64, 256])
@pytest.mark.parametrize('n', [1, 'block + 1', 63, 65, 1000, 256 * 64 + 1])
def test_colstats(n, Z):
    """'block + 1': one row more than the 256 / (Z / 4) row groups of one workgroup (257, 17 and 5 rows at Z = 4, 64,
    256). All f64 on the device, so the bounds are in 2^-53: at most N additions per sum in any order, each a rounding
    relative to the sum of the absolute values of the terms, plus 8 for the few operations on each term (a 1-ulp log
    among them) and the final algebra. The sums are taken of loc - loc[0]: the variance's terms are (x - x_0)^2 and
    S1^2 / N, the mean's are |x_0| and |x - x_0| / N. (16,385 rows: one more than the 256 workgroups x 64 row groups
    of one pass at Z = 4.)"""
    from sparse_vae import kernels as K
    if n == 'block + 1':
        n = 256 // (Z // 4) + 1
    rng = np.random.default_rng(3 * n + Z)
    loc = (rng.standard_normal((n, Z)) * 0.7 + 30.0 * (np.arange(Z) % 2)).astype(np.float32)
    scale = np.exp(rng.standard_normal((n, Z))).astype(np.float32)
    mean, var, kl = (f64(t) for t in K.latent_colstats(gpu(loc), gpu(scale)))
    w_mean, w_var, w_kl = R.colstats64(loc, scale)
    l64, s64 = loc.astype(np.float64), scale.astype(np.float64)
    d = l64 - l64[0]
    u = (n + 8) * EPS53
    b_mean = u * (np.abs(l64[0]) + np.abs(d).sum(0) / n) + 1e-300
    b_kl = u * (0.5 * (l64 ** 2 + s64 ** 2 + 1.0 + np.abs(np.log(s64 ** 2)))).sum(0) / n
    r_mean, r_kl = np.abs(mean - w_mean) / b_mean, np.abs(kl - w_kl) / b_kl
    print(f'colstats N {n} Z {Z}: err / bound mean {r_mean.max():.4f} kl {r_kl.max():.4f}', end='')
    assert r_mean.max() <= 1.0 and r_kl.max() <= 1.0
    if n == 1:
        assert np.isnan(var).all()
        print()
    else:
        # numpy's own two-pass variance is good to about (n + 8) 2^-53 of the same terms: twice the bound covers both
        b_var = 2 * u * ((d * d).sum(0) + np.abs(d).sum(0) ** 2 / n) / (n - 1)
        r_var = np.abs(var - w_var) / b_var
        print(f' var {r_var.max():.4f}')
        assert r_var.max() <= 1.0


@pytest.mark.parametrize('Z', [4, 64, 256])
@pytest.mark.parametrize('n', [1, 63, 65, 1000, 2049])
def test_draw_with_injected_eps(n, Z):
    """z = fmaf(scale, eps, loc): one rounding of the exact value (2,049 x 256 elements: one more than the 2,048
    workgroups of 256 threads, so the grid-stride loop repeats)."""
    from sparse_vae import kernels as K
    rng = np.random.default_rng(n * Z)
    loc, eps = (rng.standard_normal((n, Z)).astype(np.float32) for _ in range(2))
    scale = np.exp(rng.standard_normal((n, Z))).astype(np.float32)
    z = f64(K.latent_draw(gpu(loc), gpu(scale), eps=gpu(eps)))
    exact = loc.astype(np.float64) + scale.astype(np.float64) * eps.astype(np.float64)   # the product is exact in f64
    assert (np.abs(z - exact) <= EPS24 * np.abs(exact) * (1 + 1e-6) + 2.0 ** -149).all()


def test_draw_with_a_seed():
    """Reproducible per seed, different across seeds, and the 65,536 x 64 draws have mean and variance within five
    standard errors of N(0, 1)'s (1 / sqrt(n) and sqrt(2 / n))."""
    from sparse_vae import kernels as K
    n, Z = 65536, 64
    loc, scale = torch.zeros(n, Z, device=dev()), torch.ones(n, Z, device=dev())
    a, b, c = K.latent_draw(loc, scale, seed=5), K.latent_draw(loc, scale, seed=5), K.latent_draw(loc, scale, seed=6)
    assert torch.equal(a, b) and not torch.equal(a, c)
    e = f64(a)
    cnt = e.size
    assert np.isfinite(e).all()
    print(f'seeded draws: mean {e.mean():.3e} (5 sigma {5 / np.sqrt(cnt):.3e}) var - 1 {e.var() - 1:.3e} '
          f'(5 sigma {5 * np.sqrt(2 / cnt):.3e})')
    assert abs(e.mean()) <= 5 / np.sqrt(cnt) and abs(e.var() - 1.0) <= 5 * np.sqrt(2.0 / cnt)
    # keyed by (row, column): the first rows of a larger draw are the smaller draw
    small = K.latent_draw(loc[:100], scale[:100], seed=5)
    assert torch.equal(small, a[:100])
    shifted = K.latent_draw(loc + 2.0, scale * 0.5, seed=5)
    assert torch.equal(shifted, torch.addcmul(loc + 2.0, scale * 0.5, a))


# ---- the public functions against the reference's recorded values -----------------------------------------------------
@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(ROOT, 'tests', 'golden', 'mmd.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


NAMES = ['a', 'a_shrunk', 'a_shift', 'b', 'b_shrunk', 'b_shift']


def rbf_bounds(x, w, m):
    """(pair-sum bound, row-sum bound) of the two device sums behind an RBF estimator. Against the counts above: the
    wrapper rounds a = 0.5 / kernel_var and the weights 1 / (kernel_var + var) to f32: one more rounding relative to
    the exponent (RBF_EXTRA[0] + 1) and one relative to q."""
    n, d = x.shape
    a = 0.5 / (0.125 * d)
    _, b_pair = R.pairsum64(x, None, 'rbf', [a], None, z_roundings(d), (RBF_EXTRA[0] + 1, RBF_EXTRA[1]))
    _, q = R.rowterm64(x, w, m)
    return b_pair[0], R.rowterm_bound(q, d, w_roundings=1)


@pytest.mark.parametrize('name', NAMES)
def test_rbf_estimators_against_the_reference(golden, name):
    """Unstandardised: |error| <= 2 normalizer (row bound) / N + (pair bound) / (N (N - 1) / 2); standardised: the same
    over the null standard error. The host algebra is f64 (1e-12, tests/test_mmd_ref.py): 1e-12 of the three terms'
    magnitudes is added for it."""
    import sparse_vae
    from sparse_vae.core import math_utils as MU
    x = golden[name]
    n, d = x.shape
    kv = 0.125 * d
    xt = gpu(x)
    mean, var = golden[f'{name}/mean'], golden[f'{name}/var']
    cases = [('analytic', lambda s: sparse_vae.analytic_gaussian_rbf_mmd_sq(xt, s), MU.rbf_analytic_algebra(n, d),
              np.full(d, 1.0 / (1.0 + kv)), None),
             ('custom', lambda s: sparse_vae.custom_gaussian_rbf_mmd_sq(xt, gpu(mean), gpu(var), s),
              MU.rbf_custom_algebra(n, [float(v) for v in var]), 1.0 / (kv + var.astype(np.float64)), mean)]
    for tag, fn, (normalizer, first, variance), w, m in cases:
        b_pair, b_row = rbf_bounds(x, w, m)
        bound = 2 * normalizer * b_row / n + b_pair / (n * (n - 1) / 2) + 1e-12 * (first + 2 * normalizer + 1.0)
        for std, key in ((False, 'raw'), (True, 'std')):
            got = fn(std)
            assert got.dtype == torch.float64 and got.dim() == 0 and got.is_cuda
            want = float(golden[f'{name}/{tag}_{key}'])
            b = bound / variance ** 0.5 if std else bound
            err = abs(got.item() - want)
            f32_err = abs(float(golden[f'{name}/{tag}_{key}_f32']) - want)
            print(f'{name} {tag} {key}: got {got.item():.9g} reference {want:.9g} err / bound {err / b:.4f} '
                  f'(the reference in f32: {f32_err / b:.2f} bounds)')
            assert err <= b, (name, tag, key)


def test_rbf_statistic_separates_a_shrunk_posterior(golden):
    """The standardised statistic on N(0, I) input is of order 1; on the same rows shrunk by half it is above 10^3."""
    import sparse_vae
    for name in ('a', 'b'):
        same = sparse_vae.analytic_gaussian_rbf_mmd_sq(gpu(golden[name])).item()
        shrunk = sparse_vae.analytic_gaussian_rbf_mmd_sq(gpu(golden[name + '_shrunk'])).item()
        assert abs(float(golden[f'{name}/analytic_std'])) < 10 and float(golden[f'{name}_shrunk/analytic_std']) > 1e3
        assert abs(same) < 10 and shrunk > 1e3


@pytest.mark.parametrize('name', ['a', 'a_shrunk', 'a_shift'])
def test_imq_estimator_against_the_reference(golden, name):
    """The three sums' bounds over their counts (7 scales x pairs), the cross term twice. The wrapper rounds the
    column offset Z - |p|^2 to f32: one more rounding, relative to the offset (off_roundings). Given the recorded
    samples. By seed the library draws the same two sets itself; its standardisation runs in f32 on the host, whose
    last bits may differ from one CPU to another, so that path is held to the explicit call on the library's own draws
    (bit for bit) and to 1e-6 of the value above (every term is at most 1 and moves by a few 2^-24)."""
    import sparse_vae
    from sparse_vae.core import math_utils as MU
    x, prior, pair = golden[name], golden['prior16'], golden['prior16_pair']
    n, d = x.shape
    s = R.imq_scales(d)
    zr = z_roundings(d)
    _, b_x = R.pairsum64(x, None, 'imq', s, None, zr, IMQ_EXTRA)
    _, b_c = R.pairsum64(x, prior, 'imq', s, R.imq_offsets(prior).astype(np.float32), zr, IMQ_EXTRA, off_roundings=1)
    _, b_p = R.pairsum64(pair, None, 'imq', s, None, zr, IMQ_EXTRA)
    k, npri = len(s), len(prior)
    bound = (b_x.sum() / (k * n * (n - 1) / 2) + 2 * b_c.sum() / (k * n * npri) + b_p.sum() / (k * npri * (npri - 1) / 2)
             + 4e-12)
    want = float(golden[f'{name}/imq'])
    given = sparse_vae.gaussian_imq_mmd_sq(gpu(x), prior_samples=(gpu(prior), gpu(pair)))
    seeded = sparse_vae.gaussian_imq_mmd_sq(gpu(x), seed=int(golden['prior_seed']))
    assert given.dtype == torch.float64 and given.dim() == 0 and given.is_cuda
    own = MU.imq_prior_samples(d, int(golden['prior_seed']))
    assert seeded.item() == sparse_vae.gaussian_imq_mmd_sq(gpu(x), prior_samples=own).item()
    assert abs(seeded.item() - given.item()) <= 1e-6
    err = abs(given.item() - want)
    print(f'{name} imq: got {given.item():.9g} reference {want:.9g} err / bound {err / bound:.4f} (the reference in f32: '
          f'{abs(float(golden[f"{name}/imq_f32"]) - want) / bound:.2f} bounds)')
    assert err <= bound
    # one set of samples in both prior terms
    _, b_p1 = R.pairsum64(prior, None, 'imq', s, None, zr, IMQ_EXTRA)
    one_set = sparse_vae.gaussian_imq_mmd_sq(gpu(x), prior_samples=gpu(prior))
    assert abs(one_set.item() - R.imq(x, prior)) <= bound + (b_p1.sum() - b_p.sum()) / (k * npri * (npri - 1) / 2)


# ---- LatentIndex and the script --------------------------------------------------------------------------------------
def synthetic_index_arrays(n=1000, Z=32, dead=6):
    rng = np.random.default_rng(77)
    loc = rng.standard_normal((n, Z)).astype(np.float32) * 0.8
    scale = (0.3 + 0.5 * rng.random((n, Z))).astype(np.float32)
    loc[:, Z - dead:] = 0.0                                   # collapsed dimensions: the posterior is the prior
    scale[:, Z - dead:] = 1.0
    return loc, scale


def test_index_stats_and_mmd():
    from sparse_vae import LatentIndex, kernels as K
    import sparse_vae
    loc, scale = synthetic_index_arrays()
    n, Z = loc.shape
    index = LatentIndex(Z).add(gpu(loc), gpu(scale))
    st = index.stats()
    assert st['active_units'] == Z - 6
    assert (f64(st['var_loc'])[Z - 6:] == 0).all() and (f64(st['mean_kl'])[Z - 6:] == 0).all()
    assert (f64(st['mean_loc'])[Z - 6:] == 0).all()
    w_mean, w_var, w_kl = R.colstats64(loc, scale)
    assert np.allclose(f64(st['mean_kl']), w_kl, rtol=1e-12, atol=0) and np.allclose(f64(st['var_loc']), w_var, rtol=1e-12)
    assert st['kl'] == float(st['mean_kl'].sum().item()) and abs(st['kl'] - w_kl.sum()) <= 1e-12 * w_kl.sum()
    assert index.stats(threshold=10.0)['active_units'] == 0
    # mmd: the documented compositions of the library calls, bit for bit
    z = K.latent_draw(index.loc, index.scale, seed=3)
    assert index.mmd('rbf', 'sample', seed=3).item() == sparse_vae.analytic_gaussian_rbf_mmd_sq(z).item()
    assert index.mmd('rbf', 'mean', standardize=False).item() == \
        sparse_vae.analytic_gaussian_rbf_mmd_sq(index.loc, False).item()
    assert index.mmd('imq', 'sample', seed=3).item() == sparse_vae.gaussian_imq_mmd_sq(z, seed=3).item()
    m, v, _ = K.latent_colstats(z, index.scale)
    assert index.mmd('rbf_fitted', 'sample', seed=3).item() == sparse_vae.custom_gaussian_rbf_mmd_sq(z, m, v).item()
    assert np.isfinite(index.mmd('rbf_fitted', 'mean').item())
    assert index.mmd('rbf', 'sample', seed=3).item() != index.mmd('rbf', 'sample', seed=4).item()
    with pytest.raises(ValueError):
        index.mmd('linear')
    with pytest.raises(ValueError):
        index.mmd('rbf', 'median')


def test_latent_stats_script(tmp_path):
    """latent_stats.py in a fresh process on a 1,000-row index file: the JSON holds the library's numbers."""
    from sparse_vae import LatentIndex
    loc, scale = synthetic_index_arrays()
    n, Z = loc.shape
    src, out = str(tmp_path / 'latents.npz'), str(tmp_path / 'stats.json')
    LatentIndex(Z).add(torch.from_numpy(loc), torch.from_numpy(scale)).save(src)
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'latent_stats.py'), src, '--seed', '3', '--json', out],
                          capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    assert f'active units (Var[mu_d] > 0.01): {Z - 6} of {Z}' in done.stdout
    with open(out) as f:
        r = json.load(f)
    index = LatentIndex.load(src, dev())
    st = index.stats()
    assert r['rows'] == n and r['latent_depth'] == Z and r['active_units'] == Z - 6 == st['active_units']
    assert r['kl'] == st['kl'] and r['mean_kl'] == st['mean_kl'].tolist() and r['var_loc'] == st['var_loc'].tolist()
    assert r['mean_kl'][Z - 6:] == [0.0] * 6 and r['var_loc'][Z - 6:] == [0.0] * 6
    assert sorted(r['mmd']) == sorted(f'{k}/{s}' for k in ('rbf', 'rbf_fitted', 'imq') for s in ('sample', 'mean'))
    for key, val in r['mmd'].items():
        kind, source = key.split('/')
        assert val == index.mmd(kind, source, seed=3).item(), key
