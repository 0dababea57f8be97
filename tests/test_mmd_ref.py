"""The MMD estimators without a device: the float64 restatement of tests/mmd_ref.py against the reference's recorded
values (tests/golden/mmd.npz, written by tests/golden/make_golden_mmd.py), the host algebra of sparse_vae's functions
against the restatement, and the argument checks of the new entry points (which return before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import mmd_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ['a', 'a_shrunk', 'a_shift', 'b', 'b_shrunk', 'b_shift']


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'mmd.npz'), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def rel(got, want):
    return abs(got - want) / abs(want)


@pytest.mark.parametrize('name', NAMES)
def test_restatement_reproduces_the_reference(golden, name):
    """Same f64 arithmetic in another operation order: 1e-10 relative. (The reference's own f32 run is 1e-3 to 1e-7
    away from its f64 run on these inputs, so this tells the two apart.)"""
    x = golden[name]
    mean, var = golden[f'{name}/mean'], golden[f'{name}/var']
    got = {'analytic_std': R.analytic_rbf(x, True), 'analytic_raw': R.analytic_rbf(x, False),
           'custom_std': R.custom_rbf(x, mean, var, True), 'custom_raw': R.custom_rbf(x, mean, var, False)}
    if x.shape[1] == 16:
        got['imq'] = R.imq(x, golden['prior16'], golden['prior16_pair'])
        assert R.imq_min_denominator(x, golden['prior16']) >= 1.0
        assert float(golden[f'{name}/imq_min_denominator']) >= 1.0
    for k, v in got.items():
        want = float(golden[f'{name}/{k}'])
        print(f'{name}/{k}: restatement {v!r} reference {want!r} rel {rel(v, want):.2e} '
              f'(reference f32 run: rel {rel(float(golden[f"{name}/{k}_f32"]), want):.2e})')
        assert rel(v, want) <= 1e-10, (name, k)


def test_the_f32_reference_is_not_the_f64_one(golden):
    """What the 1e-10 above separates: somewhere on these inputs the reference in f32 is off in the fourth digit."""
    worst = max(rel(float(golden[k + '_f32']), float(golden[k])) for k in golden
                if k + '_f32' in golden)
    assert worst > 1e-4


def test_prior_samples_are_the_reference_draws(golden):
    """imq_prior_samples(Z, seed) is the reference's pair of draws after torch.manual_seed(seed): the same numbers up to
    the last bits of the f32 standardisation (torch's CPU reductions and normal transform may round differently from
    one CPU to another; on the machine that wrote the fixture they are bit-identical)."""
    from sparse_vae.core import math_utils as MU
    p, p_pair = MU.imq_prior_samples(16, int(golden['prior_seed']))
    assert p.dtype == torch.float32 and p.shape == (1000, 16) and p_pair.shape == (1000, 16)
    for got, want in ((p, golden['prior16']), (p_pair, golden['prior16_pair'])):
        assert (np.abs(got.numpy().astype(np.float64) - want) <= 8 * 2.0 ** -24 * (1.0 + np.abs(want))).all()
    assert abs(float(p.double().mean())) < 1e-7 and abs(float(p.double().var()) - 1.0) < 1e-6      # f32 roundings


@pytest.mark.parametrize('n,d', [(2, 4), (300, 64), (513, 16), (100000, 256)])
def test_host_algebra_analytic(n, d):
    from sparse_vae.core import math_utils as MU
    got, want = MU.rbf_analytic_algebra(n, d), R.analytic_algebra(n, d)
    for g, w in zip(got, want):
        assert rel(g, w) <= 1e-12
    assert MU.rbf_kernel_var(d) == 0.125 * d


@pytest.mark.parametrize('n,d', [(2, 4), (300, 64), (513, 16), (100000, 256)])
def test_host_algebra_custom(n, d):
    from sparse_vae.core import math_utils as MU
    var = np.random.default_rng(d).random(d) * 3.0 + 0.01
    got, want = MU.rbf_custom_algebra(n, [float(v) for v in var]), R.custom_algebra(n, var)
    for g, w in zip(got, want):
        assert rel(g, w) <= 1e-12
    # var = 1 in every dimension is the analytic form
    for g, w in zip(MU.rbf_custom_algebra(n, [1.0] * d), R.analytic_algebra(n, d)):
        assert rel(g, w) <= 1e-12


def test_host_algebra_combine(golden):
    """rbf_combine / imq_combine on the restatement's sums give the restatement's (= the reference's) values."""
    from sparse_vae.core import math_utils as MU
    for name in NAMES:
        x = golden[name]
        n, d = x.shape
        kv = 0.125 * d
        pair = R.pairsum64(x, None, 'rbf', [0.5 / kv])[0]
        row = R.rowterm64(x, np.full(d, 1.0 / (1.0 + kv)))[0]
        for std in (True, False):
            got = MU.rbf_combine(n, *MU.rbf_analytic_algebra(n, d), row, pair, std)
            assert rel(got, R.analytic_rbf(x, std)) <= 1e-12
        var = golden[f'{name}/var'].astype(np.float64)
        row = R.rowterm64(x, 1.0 / (kv + var), golden[f'{name}/mean'])[0]
        got = MU.rbf_combine(n, *MU.rbf_custom_algebra(n, [float(v) for v in var]), row, pair, True)
        assert rel(got, float(golden[f'{name}/custom_std'])) <= 1e-10
        if d == 16:
            prior = golden['prior16']
            assert MU.imq_scales(d) == R.imq_scales(d)
            s = MU.imq_scales(d)
            sums = [R.pairsum64(x, None, 'imq', s).sum(),
                    R.pairsum64(x, prior, 'imq', s, R.imq_offsets(prior)).sum(),
                    R.pairsum64(golden['prior16_pair'], None, 'imq', s).sum()]
            got = MU.imq_combine(n, len(prior), len(prior), *sums)
            assert rel(got, float(golden[f'{name}/imq'])) <= 1e-10


def test_the_two_distance_forms_agree():
    """The centred product form the restatement uses above 2^25 element operations against the direct differences,
    on rows at +30 (where an uncentred Gram form would lose nine bits) and on two sets: 1e-12 of d2."""
    rng = np.random.default_rng(5)
    for z in (4, 68, 256):
        x = (rng.standard_normal((300, z)) + 30.0).astype(np.float32)
        y = (rng.standard_normal((200, z)) + 30.0).astype(np.float32)
        for a, b in ((x, x), (x, y)):
            direct, centred = R.sqdist_direct(a, b), R.sqdist_centred(a, b)
            off = direct > 0
            assert (np.abs(centred - direct)[off] <= 1e-12 * direct[off]).all()
            assert (centred[~off] <= 1e-10).all()
    assert R.sqdist(x, y) is not None and 300 * 200 * 256 <= R.DIRECT_LIMIT < 2049 * 2049 * 16


# ---- argument checks (no launch, so no GPU) --------------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_launch():
    from sparse_vae import _native
    lib = _native.lib
    prm = (ctypes.c_float * 8)(*([1.0] * 8))
    pp = ctypes.addressof(prm)
    A, W, O = 4096, 8192, 16384          # non-null, aligned addresses that are never dereferenced: every call below fails

    def pairsum(x=A, n=100, y=A + 64, m=50, z=16, tri=0, kind=0, params=pp, p=1, off=None, ws=W, wsb=1 << 30, out=O):
        return lib.svae_pairsum(x, n, y, m, z, tri, kind, params, p, off, ws, wsb, out, None)

    for bad in (dict(x=None), dict(y=None), dict(params=None), dict(out=None), dict(ws=None), dict(z=6), dict(z=260),
                dict(z=0), dict(p=9), dict(p=0), dict(kind=2), dict(n=0), dict(m=0), dict(n=(1 << 24) + 1),
                dict(wsb=8), dict(x=A + 4), dict(tri=1, y=None, n=1, m=1), dict(tri=1, y=None, n=100, m=100, off=A),
                dict(tri=1, y=None, n=100, m=50), dict(tri=1, y=A + 64, n=100, m=100)):
        assert pairsum(**bad) == 1, bad
    prm[0] = -1.0
    assert pairsum() == 1 and pairsum(kind=1) == 1
    prm[0] = float('nan')
    assert pairsum() == 1 and pairsum(kind=1) == 1
    geom = (ctypes.c_int32 * 5)()
    assert lib.svae_pairsum_geometry(100, 50, 16, 0, None) == 1
    for n, m, z, tri in ((100, 50, 6, 0), (100, 50, 260, 0), (1, 1, 16, 1), (0, 5, 16, 0), (100, 50, 16, 1)):
        assert lib.svae_pairsum_geometry(n, m, z, tri, ctypes.addressof(geom)) == 1
        assert lib.svae_pairsum_ws_bytes(n, m, z, tri) == 0

    def rowterm(x=A, m=None, w=A, n=10, z=16, ws=W, wsb=1 << 20, out=O):
        return lib.svae_mmd_rowterm(x, m, w, n, z, ws, wsb, out, None)

    for bad in (dict(x=None), dict(w=None), dict(out=None), dict(ws=None), dict(z=6), dict(z=260), dict(n=0),
                dict(wsb=0), dict(m=A + 4)):
        assert rowterm(**bad) == 1, bad

    def colstats(loc=A, scale=A, n=10, z=16, ws=W, wsb=1 << 30, a=O, b=O, c=O):
        return lib.svae_latent_colstats(loc, scale, n, z, ws, wsb, a, b, c, None)

    for bad in (dict(loc=None), dict(scale=None), dict(a=None), dict(b=None), dict(c=None), dict(ws=None), dict(z=6),
                dict(z=260), dict(n=0), dict(wsb=8)):
        assert colstats(**bad) == 1, bad
    assert lib.svae_latent_colstats_ws_bytes(10, 6) == 0 and lib.svae_mmd_rowterm_ws_bytes(0) == 0

    def draw(loc=A, scale=A, eps=None, n=10, z=16, out=O):
        return lib.svae_latent_draw(loc, scale, eps, 1, n, z, out, None)

    for bad in (dict(loc=None), dict(scale=None), dict(out=None), dict(z=6), dict(z=260), dict(n=0)):
        assert draw(**bad) == 1, bad


def test_workspace_and_geometry_formulas():
    """The documented geometry (include/svae.h): rows per workgroup 512 for Z <= 64 else 256; slices = as many column
    slices of whole 32-column tiles as bring the grid to about 2048 workgroups, at most 64 and at most one per tile;
    workspace = row_blocks * slices * 8 parameters * 8 bytes."""
    from sparse_vae import _native, kernels as K
    lib = _native.lib
    assert (_native.PAIRSUM_TILE_COLS, _native.PAIRSUM_MAX_P, _native.MMD_REDUCE_BLOCKS) == (32, 8, 256)
    hdr = open(os.path.join(os.path.dirname(HERE), 'include', 'svae.h')).read()
    for line in ('#define SVAE_PAIRSUM_TILE_COLS 32', '#define SVAE_PAIRSUM_MAX_P 8', '#define SVAE_MMD_REDUCE_BLOCKS 256',
                 '#define SVAE_PAIR_RBF 0', '#define SVAE_PAIR_IMQ 1'):
        assert line in hdr

    def ceil(a, b):
        return -(-a // b)

    for n, m, z, tri in [(2, 2, 4, 1), (513, 513, 16, 1), (513, 1000, 64, 0), (2049, 2049, 64, 1), (2049, 1, 68, 0),
                         (1025, 1025, 256, 1), (65536, 65536, 64, 1), (1 << 20, 1000, 64, 0), (1 << 24, 1 << 24, 128, 1)]:
        rb = 512 if z <= 64 else 256
        row_blocks, tiles = ceil(n, rb), ceil(m, 32)
        s = min(ceil(2048, row_blocks), tiles, 64)
        per = ceil(tiles, s)
        want = (rb, row_blocks, ceil(tiles, per), per * 32, 32)
        assert K.pairsum_geometry(n, m, z, tri) == want, (n, m, z, tri)
        assert lib.svae_pairsum_ws_bytes(n, m, z, tri) == want[1] * want[2] * 8 * 8
    for n in (1, 16, 17, 4096, 4097, 1 << 24):
        assert lib.svae_mmd_rowterm_ws_bytes(n) == min(ceil(n, 16), 256) * 8
    for n, z in ((1, 4), (63, 4), (64, 4), (65, 64), (1 << 20, 64), (1000, 256), (7, 12)):
        rows_per_pass = 256 // (z // 4)
        assert lib.svae_latent_colstats_ws_bytes(n, z) == min(ceil(n, rows_per_pass), 256) * 3 * z * 8


# ---- no CPU fallback -------------------------------------------------------------------------------------------------
def test_cpu_tensors_are_refused():
    import sparse_vae
    from sparse_vae import LatentIndex
    x = torch.randn(10, 16)
    for call in (lambda: sparse_vae.analytic_gaussian_rbf_mmd_sq(x),
                 lambda: sparse_vae.custom_gaussian_rbf_mmd_sq(x, torch.zeros(16), torch.ones(16)),
                 lambda: sparse_vae.gaussian_imq_mmd_sq(x)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
    index = LatentIndex(16).add(x, torch.ones_like(x))
    for call in (lambda: index.stats(), lambda: index.mmd(), lambda: index.mmd('imq', 'mean')):
        with pytest.raises(RuntimeError, match='no CPU fallback|There is no CPU fallback'):
            call()
    with pytest.raises(ValueError, match='one per row'):          # the reference's [N, Z] variance form stays out
        sparse_vae.custom_gaussian_rbf_mmd_sq(x, 0.0, torch.ones(10, 16))
