"""The Gaussian-mixture prior without a device: the float64 restatement of tests/gmm_ref.py against brute-force loops,
the monotonicity of EM on the bound, the tie / NaN / zero-weight / empty-component rules, the collapsed-dimension case
that fixes the default source, the condition under which the GPU tests may demand identical labels for every row of the
blob cases, the argument checks of the svae_gmm_* entry points (which return before any launch), and the Python and
command-line surface."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gmm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_a(x, s2, w, m, v):
    n, Z = x.shape
    out = np.empty((n, len(w)))
    for i in range(n):
        for k in range(len(w)):
            if w[k] == 0:
                out[i, k] = -math.inf
                continue
            acc = math.log(float(w[k]))
            for d in range(Z):
                vv = float(v[k, d])
                ss = 0.0 if s2 is None else float(s2[i, d])
                acc -= 0.5 * (math.log(2 * math.pi * vv) + ((float(x[i, d]) - float(m[k, d])) ** 2 + ss) / vv)
            out[i, k] = acc
    return out


def small_case(seed, n=19, K=4, Z=8, has_s2=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, Z)).astype(np.float32)
    s2 = rng.uniform(0.1, 1.0, (n, Z)).astype(np.float32) if has_s2 else None
    w = rng.dirichlet(np.ones(K)).astype(np.float32)
    m = rng.standard_normal((K, Z)).astype(np.float32)
    v = rng.uniform(0.5, 2.0, (K, Z)).astype(np.float32)
    return x, s2, w, m, v


@pytest.mark.parametrize('has_s2', [False, True])
def test_estep_matches_a_triple_loop(has_s2):
    x, s2, w, m, v = small_case(0, has_s2=has_s2)
    e = R.estep(x, s2, w, m, v)
    want = brute_a(x, s2, w, m, v)
    assert np.allclose(e['a'], want, rtol=1e-12, atol=1e-12)
    lse = np.array([math.log(sum(math.exp(t - max(row)) for t in row)) + max(row) for row in want])
    assert np.allclose(e['lse'], lse, rtol=1e-12) and abs(e['bound'] - lse.sum()) <= 1e-10
    assert (e['label'] == want.argmax(axis=1)).all()
    assert np.allclose(e['resp'].sum(axis=1), 1.0, atol=1e-12)
    assert (e['err'] > 0).all() and (e['lse_err'] > 0).all() and (e['resp_err'] > 0).all()


@pytest.mark.parametrize('has_s2', [False, True])
def test_mstep_matches_a_loop(has_s2):
    x, s2, w, m, v = small_case(1, has_s2=has_s2)
    e = R.estep(x, s2, w, m, v)
    reg = 1e-3
    for hard in (False, True):
        out = R.mstep(x, s2, w, m, v, reg, label=e['label']) if hard else R.mstep(x, s2, w, m, v, reg, lse=e['lse'])
        r = np.eye(len(w))[e['label']] if hard else e['resp']
        for k in range(len(w)):
            nk = sum(r[i, k] for i in range(len(x)))
            assert abs(out['nk'][k] - nk) <= 1e-12 * max(nk, 1)
            if nk == 0:                               # a hard step may leave a component empty: it keeps its row
                assert np.array_equal(out['mean'][k], m[k]) and out['weight'][k] == 0
                continue
            for d in range(x.shape[1]):
                mu = sum(r[i, k] * float(x[i, d]) for i in range(len(x))) / nk
                ss = [0.0 if s2 is None else float(s2[i, d]) for i in range(len(x))]
                var = sum(r[i, k] * ((float(x[i, d]) - mu) ** 2 + ss[i]) for i in range(len(x))) / nk + float(np.float32(reg))
                assert abs(out['mean'][k, d] - mu) <= 2e-7 * max(abs(mu), 1.0)
                assert abs(out['var'][k, d] - var) <= 2e-7 * max(var, 1.0)
            assert abs(out['weight'][k] - nk / len(x)) <= 1e-7
        assert out['mean'].dtype == np.float32 and out['var'].dtype == np.float32
        if not hard:
            assert (out['mean_err'] > 0).all() and (out['var_err'] > 0).all() and (out['nk_err'] > 0).all()


@pytest.mark.parametrize('case', R.BLOBS)
def test_em_is_monotone_and_runs_several_iterations(case):
    """EM ascends the bound, with and without s2, and the blobs overlap enough that it keeps moving: a case that
    converged in one iteration would test nothing."""
    x, s2, w0, m0, v0 = R.blob_case(*case)
    b = R.fit(x, s2, w0, m0, v0, R.REG, 12, round32=False)['bounds']          # EM proper: parameters kept in f64
    assert all(b[i + 1] >= b[i] - 1e-12 * abs(b[i]) for i in range(len(b) - 1)), b
    out = R.blob_fit(*case)
    b = out['bounds']
    assert len(b) == R.BLOB_ITERS
    assert all(b[i + 1] - b[i] > 1e-3 for i in range(3)), b          # sklearn's tol would not stop it here
    assert (out['nk'] > 0).all()


@pytest.mark.parametrize('case', R.BLOBS)
def test_blob_cases_leave_no_row_near_a_tie(case):
    """The condition under which test_gmm_gpu.py exempts no row from its label comparison: in every iteration of the
    reference, every row's gap between its largest and second-largest a_ik exceeds the sum of the two entries' derived
    rounding bounds by GAP_FACTOR (whose derivation is in gmm_ref.py)."""
    out = R.blob_fit(*case)
    assert min(out['gaps']) > R.GAP_FACTOR, out['gaps']
    assert len(R.blob_case(*case)[0]) == 2 * R.ROWS_PER_BLOCK + 1


def test_tie_nan_zero_weight_and_empty_component_rules():
    x = np.array([[0, 0, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    m = np.array([[2, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    v = np.ones((4, 4), np.float32)
    w = np.full(4, 0.25, np.float32)
    e = R.estep(x, None, w, m, v)
    assert e['label'].tolist() == [1, 0, 0]                              # duplicates and the midpoint: lower index
    m2 = m.copy()
    m2[0] = np.nan
    e = R.estep(x, None, w, m2, v)
    assert e['label'].tolist() == [1, 2, 1] and np.isnan(e['lse']).all()  # NaN loses; a NaN a_ik makes lse NaN
    e = R.estep(x, None, w, np.full((4, 4), np.nan, np.float32), v)
    assert e['label'].tolist() == [0, 0, 0] and np.isnan(e['lse']).all() and np.isnan(e['bound'])
    a = np.array([[np.nan, -np.inf, 3.0], [np.nan, -np.inf, -np.inf], [-np.inf, np.nan, -np.inf]])
    assert R.winners(a).tolist() == [2, 1, 0]
    # a zero-weight component contributes exactly 0: the result is the mixture without it
    w0 = np.array([0.5, 0.0, 0.5, 0.0], np.float32)
    e0 = R.estep(x, None, w0, m, v)
    keep = [0, 2]
    e1 = R.estep(x, None, w0[keep], m[keep], v[keep])
    assert np.array_equal(e0['lse'], e1['lse']) and (e0['resp'][:, [1, 3]] == 0).all()
    assert (e0['err'][:, [1, 3]] == 0).all() and set(e0['label'].tolist()) <= {0, 2}
    # ... also when its q is NaN, and an all-zero-weight mixture gives -inf
    m3 = m.copy()
    m3[1] = np.nan
    assert np.array_equal(R.estep(x, None, w0, m3, v)['lse'], e1['lse'])
    assert np.isneginf(R.estep(x, None, np.zeros(4, np.float32), m, v)['lse']).all()
    # an empty component keeps its mean and variance and gets weight 0; labels outside 0..K-1 are ignored
    out = R.mstep(x, None, w, m, v * 3, 1e-6, label=np.array([0, 7, -1]))
    assert out['nk'].tolist() == [1, 0, 0, 0] and out['weight'].tolist() == [1, 0, 0, 0]
    assert np.array_equal(out['mean'][1:], m[1:]) and np.array_equal(out['var'][1:], (v * 3)[1:])
    assert np.array_equal(out['mean'][0], x[0]) and np.allclose(out['var'][0], 1e-6)
    # a component that loses all mass in a soft step
    far = m.copy()
    far[3] = 1e4
    out = R.mstep(x, None, w, far, v, 1e-6, lse=R.estep(x, None, w, far, v)['lse'])
    assert out['nk'][3] == 0 and out['weight'][3] == 0 and np.array_equal(out['mean'][3], far[3])


def test_sample_rules():
    w = np.array([0.25, 0.0, 0.5, 0.25, 0.0], np.float32)
    m = np.arange(20, dtype=np.float32).reshape(5, 4)
    v = np.full((5, 4), 4.0, np.float32)
    below = np.nextafter(np.float32(0.25), np.float32(0))
    u = np.array([0.0, below, 0.25, 0.5, 0.75 - 2.0 ** -24, 0.75, 1 - 2.0 ** -24, 1.0], np.float32)
    eps = np.tile(np.array([[0.5, -1.0, 0.0, 2.0]], np.float32), (len(u), 1))
    comp, z, exact = R.sample(w, m, v, u, eps)
    assert comp.tolist() == [0, 0, 2, 2, 2, 3, 3, 3]                     # weight 0 is never drawn; u >= 1 clamps
    assert exact.all() and np.array_equal(z[2], m[2] + 2.0 * eps[2])


def test_fitting_the_means_collapses_what_fitting_the_posteriors_keeps():
    """Why the default source is 'posterior': on 16 active and 48 collapsed dimensions (mu ~ 0, s2 ~ 0.98), a mixture of
    the means drives the collapsed variances to the scale of the jitter and reg_covar, where the decoder never saw z;
    a mixture of the posteriors keeps them at the posterior variance."""
    mu, s2 = R.collapsed_case()
    K, Z = 2, mu.shape[1]
    w0 = np.full(K, 0.5, np.float32)
    m0 = np.zeros((K, Z), np.float32)
    m0[0, :16], m0[1, :16] = -1.0, 1.0
    v0 = np.ones((K, Z), np.float32)
    as_points = R.fit(mu, None, w0, m0, v0, 1e-6, 20)
    as_posteriors = R.fit(mu, s2, w0, m0, v0, 1e-6, 20)
    assert as_points['var'][:, 16:].max() < 1e-3                        # (0.02)^2 = 4e-4 and reg_covar
    assert 0.9 < as_posteriors['var'][:, 16:].min() and as_posteriors['var'][:, 16:].max() < 1.1
    assert np.abs(np.abs(as_posteriors['mean'][:, :16]) - 1.5).max() < 0.2   # both find the two clusters
    assert np.abs(np.abs(as_points['mean'][:, :16]) - 1.5).max() < 0.2


def test_rounding_bound_is_the_one_the_kernel_states():
    assert [R.q_roundings(Z) for Z in R.ZS] == [7, 37, 39, 133]
    src = open(os.path.join(ROOT, 'sparse-vae_amd', 'csrc', 'gmm.hip')).read()
    assert '((Z / 2 + 5) q / 2 + |logc| + |a|) 2^-24' in src
    for n, K, Z, has_s2 in R.exact_shapes():
        x, s2, w, m, v, label = R.exact_case(n, K, Z, has_s2)
        assert x.shape == (n, Z) and m.shape == (K, Z) and (s2 is None) == (not has_s2)
        assert np.abs(x).max() <= 7 and np.abs(m).max() <= 7 and n * (14 * 14 + 3) < 2 ** 53


# ---- argument checks (no launch, so no GPU) --------------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_launch():
    from sparse_vae import _native
    lib = _native.lib
    A, B, P, W, O = 4096, 8192, 1 << 18, 1 << 20, 1 << 16     # non-null, aligned addresses that are never dereferenced
    MAXK = _native.GMM_MAX_K
    assert MAXK >= 256
    shapes_bad = (dict(z=6), dict(z=0), dict(z=260), dict(k=0), dict(k=MAXK + 1), dict(n=0), dict(n=(1 << 24) + 1))

    def estep(x=A, s2=B, n=1000, params=P, k=10, z=16, lse=O, label=O + 4096, resp=None, bound=O + 8192, ws=W,
              wsb=None):
        wsb = lib.svae_gmm_estep_ws_bytes(n, k, z) if wsb is None else wsb
        return lib.svae_gmm_estep(x, s2, n, params, k, z, lse, label, resp, bound, ws, wsb, None)

    def mstep(x=A, s2=B, n=1000, lse=O, label=None, params=P, k=10, z=16, reg=1e-6, nk=O + 8192, ws=W, wsb=None):
        wsb = lib.svae_gmm_mstep_ws_bytes(n, k, z) if wsb is None else wsb
        return lib.svae_gmm_mstep(x, s2, n, lse, label, params, k, z, reg, nk, ws, wsb, None)

    def sample(params=P, k=10, z=16, n=1000, u=None, eps=None, zz=A, comp=O):
        return lib.svae_gmm_sample(params, k, z, n, u, eps, 1, zz, comp, None)

    def prepare(params=P, k=10, z=16):
        return lib.svae_gmm_prepare(params, k, z, None)

    for fn, nulls in ((estep, ('x', 'params', 'lse', 'bound', 'ws')), (mstep, ('x', 'params', 'nk', 'ws')),
                      (sample, ('params', 'zz', 'comp')), (prepare, ('params',))):
        for name in nulls:
            assert fn(**{name: None}) == 1, (fn.__name__, name)
        for bad in shapes_bad:
            if fn is prepare and 'n' in bad:
                continue
            assert fn(**bad) == 1, (fn.__name__, bad)
        assert fn(params=P + 4) == 1, fn.__name__                     # the block is 16-byte aligned
    for fn in (estep, mstep):
        assert fn(x=A + 4) == 1 and fn(s2=B + 4) == 1, fn.__name__     # rows are 16-byte aligned
    assert mstep(lse=None, label=None) == 1 and mstep(lse=O, label=O + 4096) == 1   # exactly one of the two
    assert mstep(reg=-1.0) == 1 and mstep(reg=float('nan')) == 1
    assert estep(label=O + 2) == 1 and estep(bound=O + 4) == 1 and sample(u=O + 2) == 1
    for ws_bytes, fn in ((lib.svae_gmm_estep_ws_bytes, estep), (lib.svae_gmm_mstep_ws_bytes, mstep)):
        need = ws_bytes(1000, 10, 16)
        assert need > 0 and need % 8 == 0
        assert fn(wsb=need - 1) == 1 and fn(wsb=0) == 1 and fn(ws=W + 4) == 1
        for bad in shapes_bad:
            args = dict(n=1000, k=10, z=16)
            args.update(bad)
            assert ws_bytes(args['n'], args['k'], args['z']) == 0, bad
    geom = (ctypes.c_int32 * 6)()
    assert lib.svae_gmm_geometry(1000, 10, 16, 0, None) == 1
    for bad in shapes_bad:
        args = dict(n=1000, k=10, z=16)
        args.update(bad)
        assert lib.svae_gmm_geometry(args['n'], args['k'], args['z'], 1, ctypes.addressof(geom)) == 1
        if 'n' not in bad:
            assert lib.svae_gmm_params_floats(args['k'], args['z']) == 0
    assert list(geom) == [0] * 6                                       # nothing written


def test_workspace_geometry_and_layout_formulas():
    """The documented geometry, workspaces and parameter block (include/svae.h), and the header's constants."""
    from sparse_vae import _native, kernels as K
    lib = _native.lib
    assert (_native.GMM_MAX_K, _native.GMM_TILE_COMPONENTS, _native.GMM_ROWS_PER_BLOCK) == (256, 16, 256)
    assert (R.MAX_K, R.TILE, R.ROWS_PER_BLOCK) == (256, 16, 256)
    hdr = open(os.path.join(ROOT, 'include', 'svae.h')).read()
    for line in ('#define SVAE_GMM_MAX_K 256', '#define SVAE_GMM_TILE_COMPONENTS 16',
                 '#define SVAE_GMM_ROWS_PER_BLOCK 256'):
        assert line in hdr

    def ceil(a, b):
        return -(-a // b)

    for n, k, z in [(1, 1, 4), (65, 2, 64), (1025, 33, 64), (513, 256, 68), (1 << 20, 100, 64), (1 << 24, 256, 256),
                    (1 << 24, 1, 256), (524289, 3, 4)]:
        rpg = ceil(ceil(n, max(1, 16384 // k)), 64) * 64
        G = ceil(n, rpg)
        for has_s2 in (0, 1):
            segs = 4 if has_s2 and z > 128 else 1
            assert K.gmm_geometry(n, k, z, has_s2) == (256, ceil(n, 256), 16, G, rpg, segs), (n, k, z)
        assert lib.svae_gmm_estep_ws_bytes(n, k, z) == ceil(n, 256) * 8
        assert lib.svae_gmm_mstep_ws_bytes(n, k, z) == (G + 1) * k * (2 * z + 1) * 8
        kp = ceil(k, 4) * 4
        assert lib.svae_gmm_params_floats(k, z) == 2 * kp + 4 * k * z
        off = K.gmm_param_offsets(k, z)
        assert [off[s][0] for s in ('weight', 'logc', 'mean', 'var', 'inv_var', 'sd')] == \
            [0, kp, 2 * kp, 2 * kp + k * z, 2 * kp + 2 * k * z, 2 * kp + 3 * k * z]
        assert all(off[s][0] % 4 == 0 for s in ('mean', 'var', 'inv_var', 'sd'))     # rows stay 16-byte aligned
    assert lib.svae_gmm_mstep_ws_bytes(1 << 24, 256, 256) < 68 * (1 << 20)            # sensible at the largest shape
    assert K.gmm_geometry(100000, 3, 64)[3] > 1                                       # several M-step row groups


# ---- the Python and command-line surface ----------------------------------------------------------------------------
def test_mixture_refuses_cpu_tensors():
    from sparse_vae import GaussianMixture, LatentIndex
    x = torch.randn(20, 8)
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        GaussianMixture(3).fit(x)
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        GaussianMixture(3).fit(x, torch.ones_like(x))
    index = LatentIndex(8).add(x, torch.ones_like(x))
    for source in ('posterior', 'mean'):
        with pytest.raises(RuntimeError, match='There is no CPU fallback'):
            index.fit_mixture(3, source=source)
    with pytest.raises(ValueError):
        index.fit_mixture(3, source='sample')
    prior = GaussianMixture.standard_normal(8)
    for call in (lambda: prior.score_samples(x), lambda: prior.sample(4), lambda: prior.predict(x),
                 lambda: prior.predict_proba(x), lambda: prior.score(x), lambda: prior.bic(x)):
        with pytest.raises(RuntimeError, match='There is no CPU fallback'):
            call()
    with pytest.raises(RuntimeError, match='before fit'):
        GaussianMixture(3).sample(4)
    with pytest.raises(ValueError):
        GaussianMixture(3, init='random')
    with pytest.raises(ValueError):
        GaussianMixture(3, init=(torch.ones(4) / 4, torch.zeros(4, 8), torch.ones(4, 8)))
    with pytest.raises(ValueError):
        GaussianMixture(0)
    with pytest.raises(ValueError):
        GaussianMixture(257)
    gm = GaussianMixture(5)
    assert (gm.max_iter, gm.tol, gm.reg_covar, gm.n_init, gm.seed, gm.check_every, gm.init) == \
        (100, 1e-3, 1e-6, 1, 0, 4, 'kmeans')
    assert gm.means_ is None and gm.converged_ is None


def test_save_load_round_trip_of_a_hand_made_model(tmp_path):
    from sparse_vae import GaussianMixture
    w = torch.tensor([0.2, 0.5, 0.3])
    m = torch.arange(24, dtype=torch.float32).reshape(3, 8) / 7
    v = 0.5 + torch.arange(24, dtype=torch.float32).reshape(3, 8) / 11
    gm = GaussianMixture.from_parameters(w, m, v, max_iter=7, tol=0.5, reg_covar=1e-4, n_init=2, seed=9, check_every=3)
    path = str(tmp_path / 'prior.npz')
    gm.save(path)
    with np.load(path) as f:
        assert {'weights', 'means', 'variances', 'max_iter', 'tol', 'reg_covar', 'n_init', 'seed',
                'check_every'} <= set(f.files)
    back = GaussianMixture.load(path)
    assert torch.equal(back.weights_, w) and torch.equal(back.means_, m) and torch.equal(back.variances_, v)
    assert (back.n_components, back.max_iter, back.tol, back.reg_covar, back.n_init, back.seed, back.check_every) == \
        (3, 7, 0.5, 1e-4, 2, 9, 3)
    one = GaussianMixture.standard_normal(16)
    assert one.n_components == 1 and one.weights_.tolist() == [1.0]
    assert (one.means_ == 0).all() and (one.variances_ == 1).all() and one.means_.shape == (1, 16)


def test_fit_prior_lists_its_flags():
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'fit_prior.py'), '--help'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ('--k', '--out', '--source', '--holdout', '--n-init', '--max-iter', '--seed', '--top'):
        assert flag in r.stdout, flag


def test_sample_script_accepts_a_prior():
    sys.path.insert(0, ROOT)
    try:
        import sample
    finally:
        sys.path.remove(ROOT)
    parser = sample.build_parser()
    assert parser.parse_args([]).prior is None
    assert parser.parse_args(['--prior', 'prior.npz']).prior == 'prior.npz'
