"""The float64 restatement of the aggregate-posterior kernels (tests/aggpost_ref.py) against the definitions, the
identities the decomposition must satisfy, and the parts of the new surface that need no device: the entry points'
argument checks and geometry, the Python surface, and the CPU index's refusal."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import aggpost_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ('svae_aggpost_geometry', 'svae_aggpost_ws_bytes', 'svae_aggpost_logq', 'svae_aggpost_decompose')


def small(seed=0, M=5, N=7, Z=4):
    rng = np.random.default_rng(seed)
    loc = rng.standard_normal((N, Z)).astype(np.float32)
    scale = rng.uniform(0.1, 1.5, (N, Z)).astype(np.float32)
    src = rng.integers(0, N, M).astype(np.int32)
    z = R.draw(loc[src], scale[src], rng.standard_normal((M, Z)).astype(np.float32))
    return z, src, loc, scale


@pytest.mark.parametrize('loo', [False, True])
def test_reference_equals_the_double_loop(loo):
    z, src, loc, scale = small()
    skip = src if loo else None
    want_q, want_d = R.brute_logq(z, loc, scale, skip)
    got = R.logq(z, loc, scale, skip, per_dim=True)
    assert np.allclose(got['logq'], want_q, rtol=0, atol=1e-12)
    assert np.allclose(got['logq_dim'], want_d, rtol=0, atol=1e-12)
    assert (got['logq_err'] > 0).all() and (got['logq_err'] < 1e-3).all()
    assert (got['logq_dim_err'] > 0).all() and (got['logq_dim_err'] < 1e-3).all()
    if loo:           # leaving the own component out lowers the density estimate at the point
        inc = R.logq(z, loc, scale, None)['logq']
        assert (want_q + math.log(6) < inc + math.log(7)).all()


def test_skip_outside_the_rows_leaves_none_out():
    z, src, loc, scale = small(1)
    a = R.logq(z, loc, scale, None, per_dim=True)
    b = R.logq(z, loc, scale, np.full(len(z), -1, np.int32), per_dim=True)
    assert np.array_equal(a['logq'], b['logq']) and np.array_equal(a['logq_dim'], b['logq_dim'])


@pytest.mark.parametrize('kind', ['vae', 'extreme'])
def test_marginal_kl_is_tc_plus_the_dimension_kls(kind):
    z, src, loc, scale = R.case(33, 40, 8, kind)
    r = R.surgery(loc, scale, src, z)
    out = r['out']
    scale_ = np.abs(out[1]) + np.abs(out[2]) + np.abs(out[4:]).sum() + np.abs(r['logq']).mean()
    assert abs(out[1] - (out[2] + out[4:].sum())) <= 64 * 2.0 ** -52 * scale_
    assert out[3] == out[0] + out[1]


def test_separated_rows_give_exactly_the_cap():
    """loc_j0 = 64 j, scale 1, |eps| <= 4: a foreign term is below exp(-1800) of the own one, which f64 flushes to 0,
    so the reference's inclusive estimate is log N to rounding, whatever the draws."""
    N = 24
    z, src, loc, scale = R.case(N, N, 4, 'separated')
    r = R.surgery(loc, scale, src, z)
    assert abs(r['out'][0] - math.log(N)) <= 1e-13 and r['mi_cap'] == math.log(N)
    assert np.isfinite(r['out']).all()


def test_one_row_has_no_mutual_information():
    z, src, loc, scale = R.case(9, 1, 4, 'vae')
    r = R.surgery(loc, scale, src, z)
    assert abs(r['out'][0]) <= 1e-13 and r['mi_cap'] == 0.0


def test_inclusive_and_leave_one_out_bracket():
    z, src, loc, scale = R.case(48, 48, 4, 'vae')
    inc = R.surgery(loc, scale, src, z)
    loo = R.surgery(loc, scale, src, z, leave_one_out=True)
    assert inc['out'][0] < loo['out'][0] and inc['out'][1] > loo['out'][1]
    assert abs(inc['out'][3] - loo['out'][3]) <= 1e-12 * (1 + abs(inc['out'][3]))      # log q(z) cancels in kl_mc
    assert inc['out'][0] <= inc['mi_cap']


def test_geometry_restated():
    from sparse_vae import _native, kernels as K
    assert (_native.AGGPOST_POINTS_PER_BLOCK, _native.AGGPOST_TILE_ROWS, _native.AGGPOST_PASS_DIMS) == \
        (R.POINTS_PER_BLOCK, R.TILE_ROWS, R.PASS_DIMS)
    hdr = open(os.path.join(ROOT, 'include', 'svae.h')).read()
    for name, v in (('POINTS_PER_BLOCK', R.POINTS_PER_BLOCK), ('TILE_ROWS', R.TILE_ROWS), ('PASS_DIMS', R.PASS_DIMS)):
        assert f'#define SVAE_AGGPOST_{name} {v}\n' in hdr
    for M, N, Z in R.shapes() + [(16384, 131072, 64), (131072, 131072, 64), (16384, 1 << 20, 64), (1 << 24, 1 << 24, 256),
                                 (300000, 1000, 8), (1, 1 << 24, 4)]:
        for per_dim in (False, True):
            assert K.aggpost_geometry(M, N, Z, per_dim) == R.geometry(M, N, Z, per_dim), (M, N, Z, per_dim)
            assert _native.lib.svae_aggpost_ws_bytes(M, N, Z, int(per_dim)) == R.ws_bytes(M, N, Z, per_dim)
    g = R.geometry(65, R.MIN_SLICE_ROWS + 1, 64, True)
    assert g[2] == 2 and g[3] == R.MIN_SLICE_ROWS                  # the last slice holds one row
    assert R.geometry(65, 2 * R.MIN_SLICE_ROWS + 1, 64, True)[2] == 3
    assert R.geometry(1, 1 << 20, 64, False)[2] == 1024 and R.geometry(1 << 20, 1 << 20, 64, False)[2] == 1


def test_bad_arguments_are_refused_without_a_launch():
    from sparse_vae import _native
    lib = _native.lib
    A, W = 4096, 1 << 30            # aligned non-NULL addresses that are never dereferenced: every call must return first
    geom = (ctypes.c_int32 * 6)()
    G = ctypes.addressof(geom)
    for bad in ((0, 8, 8), (8, 0, 8), (8, 8, 0), (8, 8, 6), (8, 8, 260), ((1 << 24) + 1, 8, 8), (8, (1 << 24) + 1, 8)):
        assert lib.svae_aggpost_geometry(*bad, 0, G) == 1, bad
        assert lib.svae_aggpost_ws_bytes(*bad, 1) == 0, bad
    assert lib.svae_aggpost_geometry(8, 8, 8, 0, None) == 1
    assert lib.svae_aggpost_decompose_ws_bytes(0, 8) == 0 and lib.svae_aggpost_decompose_ws_bytes(8, 6) == 0
    assert lib.svae_aggpost_decompose_ws_bytes(257, 8) == 2 * 11 * 8

    def logq(z=A, M=8, loc=A, scale=A, N=8, Z=8, skip=None, out=A, out_dim=None, ws=A, ws_bytes=W):
        return lib.svae_aggpost_logq(z, M, loc, scale, N, Z, skip, out, out_dim, ws, ws_bytes, None)

    for bad in (dict(z=None), dict(loc=None), dict(scale=None), dict(out=None), dict(ws=None), dict(z=A + 4),
                dict(loc=A + 8), dict(ws=A + 8), dict(out=A + 2), dict(M=0), dict(N=0), dict(Z=6), dict(Z=260),
                dict(Z=0), dict(M=(1 << 24) + 1), dict(N=(1 << 24) + 1), dict(ws_bytes=8 * 16 - 1),
                dict(out_dim=A, ws_bytes=8 * 9 * 16 - 1), dict(skip=A, N=1), dict(skip=A + 2)):
        assert logq(**bad) == 1, bad

    def dec(z=A, src=A, loc=A, scale=A, lq=A, lqd=A, M=8, Z=8, ws=A, ws_bytes=W, out=A):
        return lib.svae_aggpost_decompose(z, src, loc, scale, lq, lqd, M, Z, ws, ws_bytes, out, None)

    for bad in (dict(z=None), dict(src=None), dict(loc=None), dict(scale=None), dict(lq=None), dict(lqd=None),
                dict(out=None), dict(ws=None), dict(M=0), dict(Z=6), dict(Z=260), dict(out=A + 4),
                dict(ws_bytes=11 * 8 - 1)):
        assert dec(**bad) == 1, bad


def test_header_declares_the_entry_points_as_native_calls_them():
    from sparse_vae import _native
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'svae.h')).read(), flags=re.S)
    for name in ENTRY_POINTS + ('svae_aggpost_decompose_ws_bytes',):
        m = re.search(r'^\s*(int|int64_t)\s+%s\s*\(([^)]*)\)\s*;' % name, src, flags=re.M)
        assert m, name
        assert len(m.group(2).split(',')) == len(_native._SIGS[name]), name
        assert (m.group(1) == 'int64_t') == name.endswith('ws_bytes')
        assert getattr(_native.lib, name).restype is (ctypes.c_int64 if name.endswith('ws_bytes') else ctypes.c_int)


def test_python_surface():
    import sparse_vae
    from sparse_vae import ElboSurgery, LatentIndex, kernels as K
    from sparse_vae.surgery import sample_rows
    assert sparse_vae.ElboSurgery is ElboSurgery
    for f in ('mutual_info', 'marginal_kl', 'total_correlation', 'dim_kl', 'kl_mc', 'kl_analytic', 'mi_cap', 'rows',
              'samples', 'seed', 'leave_one_out'):
        assert f in ElboSurgery.__dataclass_fields__, f
    assert callable(LatentIndex.log_density) and callable(LatentIndex.elbo_surgery)
    assert callable(K.aggpost_geometry) and callable(K.aggpost_logq) and callable(K.aggpost_decompose)
    doc = ElboSurgery.__doc__
    assert 'LOW' in doc and 'HIGH' in doc and 'bracket' in doc
    rows = sample_rows(1000, 100, seed=3)
    assert rows.dtype == torch.int64 and rows.numel() == 100 and bool((rows[1:] > rows[:-1]).all())
    assert torch.equal(rows, sample_rows(1000, 100, seed=3)) and not torch.equal(rows, sample_rows(1000, 100, seed=4))
    assert torch.equal(sample_rows(10, None), torch.arange(10)) and torch.equal(sample_rows(10, 10), torch.arange(10))
    assert torch.equal(sample_rows(10, 50), torch.arange(10))
    s = ElboSurgery(3.0, 1.0, 0.5, torch.zeros(4, dtype=torch.float64), 4.0, 4.0, math.log(20), torch.arange(20), 20, 0,
                    False)
    assert s.saturated and s.to_dict()['saturated'] is True and s.to_dict()['rows'] == 20
    s.mutual_info = 2.0
    assert not s.saturated


def test_cpu_index_refuses():
    from sparse_vae import LatentIndex
    index = LatentIndex(4, device='cpu').add(torch.zeros(3, 4), torch.ones(3, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        index.log_density(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        index.elbo_surgery()
    with pytest.raises(ValueError, match='empty'):
        LatentIndex(4, device='cpu').elbo_surgery()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        from sparse_vae import kernels as K
        K.aggpost_logq(torch.zeros(2, 4), torch.zeros(3, 4), torch.ones(3, 4))


def test_script_parser():
    import importlib.util
    spec = importlib.util.spec_from_file_location('elbo_surgery_script', os.path.join(ROOT, 'elbo_surgery.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    a = mod.build_parser().parse_args(['x.npz', '--samples', '7', '--leave-one-out', '--json', 'o.json'])
    assert (a.index, a.samples, a.seed, a.leave_one_out, a.json, a.device) == ('x.npz', 7, 0, True, 'o.json', 'cuda')
