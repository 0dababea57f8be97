"""The Gaussian-mixture kernels (csrc/gmm.hip), sparse_vae.GaussianMixture and the two scripts on the device, against
the float64 restatement of tests/gmm_ref.py. Exact cases (integer coordinates and hard labels: every f64 sum is exact in
any order) must EQUAL the reference; everything in f32 is held within the bounds gmm_ref.py derives from the orders the
kernel states; the blob cases compare every row's label with no exemption, which
test_gmm_ref.py::test_blob_cases_leave_no_row_near_a_tie licenses on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import gmm_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))              # a copy: the cached cases are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def kernels():
    from sparse_vae import kernels as K
    return K


def pack(w, m, v):
    return kernels().gmm_pack(gpu(w), gpu(m), gpu(v))


def model_of(params, K, Z):
    Kn = kernels()
    return tuple(Kn.gmm_view(params, K, Z, s).cpu().numpy() for s in ('weight', 'mean', 'var'))


def test_geometry_of_the_cases():
    """Each size hits the boundary it is named for, read from the library's own geometry."""
    from sparse_vae import _native
    K = kernels()
    assert (_native.GMM_ROWS_PER_BLOCK, _native.GMM_TILE_COMPONENTS, _native.GMM_MAX_K) == \
        (R.ROWS_PER_BLOCK, R.TILE, R.MAX_K)
    shapes = R.exact_shapes()
    for Z in R.ZS:
        for has_s2 in (False, True):
            g = K.gmm_geometry(1000, 10, Z, has_s2)
            Rz, T = g[0], g[2]
            assert (Rz, T) == (R.ROWS_PER_BLOCK, R.TILE)
            ns = {n for n, k, z, s in shapes if z == Z and s == has_s2}
            ks = {k for n, k, z, s in shapes if z == Z and s == has_s2}
            assert {65, Rz + 1, 2 * Rz + 1} <= ns and {1, 2, T, T + 1, 2 * T + 1, R.MAX_K} <= ks
            assert K.gmm_geometry(Rz, 1, Z, has_s2)[1] == 1 and K.gmm_geometry(Rz + 1, 1, Z, has_s2)[1] == 2
            assert K.gmm_geometry(2 * Rz + 1, 1, Z, has_s2)[1] == 3
            assert any(K.gmm_geometry(n, k, Z, has_s2)[3] > 1 for n, k, z, s in shapes)   # several M-step row groups
            assert any(K.gmm_geometry(n, k, Z, has_s2)[4] > 64 for n, k, z, s in shapes)  # several batches in a group
    assert K.gmm_geometry(513, 3, 256, True)[5] > 1 and K.gmm_geometry(513, 3, 256, False)[5] == 1
    assert {z <= 64 for z in R.ZS} == {True, False} and 68 % 64 and 68 > 64


@pytest.mark.parametrize('n,K,Z,has_s2', R.exact_shapes())
def test_hard_mstep_equals_the_reference_on_exact_cases(n, K, Z, has_s2):
    Kn = kernels()
    x, s2, w, m, v, label = R.exact_case(n, K, Z, has_s2)
    want = R.mstep(x, s2, w, m, v, 0.5, label=label)
    xt, st, lt = gpu(x), gpu(s2), gpu(label)
    outs = []
    for _ in range(2):
        params = pack(w, m, v)
        nk = Kn.gmm_mstep(xt, st, params, K, label=lt, reg_covar=0.5)
        outs.append((params.clone(), nk.clone()))
        gw, gm, gv = model_of(params, K, Z)
        assert np.array_equal(nk.cpu().numpy(), want['nk'])
        assert np.array_equal(gm, want['mean']) and np.array_equal(gv, want['var']) and np.array_equal(gw, want['weight'])
        sd = Kn.gmm_view(params, K, Z, 'sd').cpu().numpy()
        iv = Kn.gmm_view(params, K, Z, 'inv_var').cpu().numpy()
        assert np.array_equal(sd, np.sqrt(gv.astype(np.float64)).astype(np.float32))
        assert np.array_equal(iv, (1.0 / gv.astype(np.float64)).astype(np.float32))
        logc = Kn.gmm_view(params, K, Z, 'logc').cpu().numpy().astype(np.float64)
        ref = R.derived(gw, gm, gv)[1]
        live = np.isfinite(ref)
        assert (np.isneginf(logc) == np.isneginf(ref)).all()
        assert (np.abs(logc[live] - ref[live]) <= 2 * R.EPS24 * np.abs(ref[live]) + 1e-12).all()
    if K >= 3:
        assert want['nk'][K - 1] == 0 and want['weight'][K - 1] == 0          # the empty component kept its row
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def check_estep(x, s2, w, m, v, labels):
    """The device's E-step of one model against the reference, row by row -> the device's lse."""
    Kn = kernels()
    K, Z = m.shape
    n = len(x)
    e = R.estep(x, s2, w, m, v)
    xt, st, params = gpu(x), gpu(s2), pack(w, m, v)
    lse, label, resp, bound = Kn.gmm_estep(xt, st, params, K, want_resp=True)
    lse2, label2, resp2, bound2 = Kn.gmm_estep(xt, st, params, K, want_resp=True)
    assert torch.equal(lse, lse2) and torch.equal(label, label2) and torch.equal(resp, resp2)      # bit for bit
    assert torch.equal(bound, bound2)
    got = lse.cpu().numpy().astype(np.float64)
    over = np.abs(got - e['lse']) / e['lse_err']
    print(f'lse: worst error / bound {over.max():.3f}')
    assert (over <= 1).all(), (over.max(), int(over.argmax()))
    r = resp.cpu().numpy().astype(np.float64)
    over = np.abs(r - e['resp']) / e['resp_err']
    print(f'resp: worst error / bound {over.max():.3f}')
    assert (over <= 1).all(), over.max()
    if labels:
        assert np.array_equal(label.cpu().numpy(), e['label'])
    total = got.sum()
    assert abs(float(bound.item()) - total) <= n * 2.0 ** -52 * np.abs(got).sum()       # f64 summation error
    return lse, params


@pytest.mark.parametrize('n,K,Z,has_s2', R.exact_shapes())
def test_estep_within_the_derived_bounds(n, K, Z, has_s2):
    x, s2, w, m, v, _ = R.exact_case(n, K, Z, has_s2)
    rng = np.random.default_rng(n + K + Z)
    w = rng.dirichlet(np.ones(K)).astype(np.float32)
    v = (np.asarray(v) * rng.uniform(0.7, 1.3, v.shape)).astype(np.float32)
    x = (np.asarray(x) + rng.uniform(-0.5, 0.5, x.shape)).astype(np.float32)
    check_estep(x, s2, w, m, v, labels=False)


@pytest.mark.parametrize('case', R.BLOBS)
def test_estep_and_soft_mstep_follow_the_reference_on_blobs(case):
    """Every iterate of the reference's fit: the E-step per row with identical labels, then the soft M-step fed the
    device's own lse, within the derived bounds."""
    Kn = kernels()
    K, Z, _ = case
    x, s2 = R.blob_case(*case)[:2]
    xt, st = gpu(x), gpu(s2)
    assert Kn.gmm_geometry(len(x), K, Z, s2 is not None)[3] > 1                        # several row groups
    for w, m, v in R.blob_fit(*case)['hist'][::2]:
        lse, params = check_estep(x, s2, w, m, v, labels=True)
        want = R.mstep(x, s2, w, m, v, R.REG, lse=lse.cpu().numpy())
        nk = Kn.gmm_mstep(xt, st, params, K, lse=lse, reg_covar=R.REG)
        again = pack(w, m, v)
        nk2 = Kn.gmm_mstep(xt, st, again, K, lse=lse, reg_covar=R.REG)
        assert torch.equal(params, again) and torch.equal(nk, nk2)                     # bit for bit
        gw, gm, gv = model_of(params, K, Z)
        for name, got, ref, err in (('nk', nk.cpu().numpy(), want['nk'], want['nk_err']),
                                    ('mean', gm, want['mean'], want['mean_err']),
                                    ('var', gv, want['var'], want['var_err']),
                                    ('weight', gw, want['weight'], want['weight_err'])):
            # the reference's own f32 rounding of the stored parameter is one more u
            slack = 0 if name == 'nk' else np.abs(ref.astype(np.float64)) * R.EPS24
            over = np.abs(got.astype(np.float64) - ref.astype(np.float64)) / (err + slack)
            print(f'{name}: worst error / bound {over.max():.3f}')
            assert (over <= 1).all(), (name, over.max())


def test_zero_weight_lost_mass_and_nan_rules():
    Kn = kernels()
    x, s2, w, m, v = R.blob_case(3, 64, True)
    xt, st = gpu(x), gpu(s2)
    # a zero-weight component contributes exactly 0: the same bits as the mixture without it, and it is never the label
    w4 = np.array([0.5, 0.0, 0.3, 0.2], np.float32)
    m4 = np.concatenate([m[:1], m[:1] * 0, m[1:]])
    v4 = np.ones_like(m4)
    lse4, lab4, resp4, _ = Kn.gmm_estep(xt, st, pack(w4, m4, v4), 4, want_resp=True)
    lse3, lab3, _, _ = Kn.gmm_estep(xt, st, pack(w4[[0, 2, 3]], m4[[0, 2, 3]], v4[[0, 2, 3]]), 3)
    assert torch.equal(lse4, lse3) and (resp4[:, 1] == 0).all() and not (lab4 == 1).any()
    assert torch.equal(lab4, torch.where(lab3 > 0, lab3 + 1, lab3))
    m4n = m4.copy()
    m4n[1] = np.nan                                                    # ... also when its q is NaN
    assert torch.equal(Kn.gmm_estep(xt, st, pack(w4, m4n, v4), 4)[0], lse3)
    # a component that loses all mass keeps its mean and variance and gets weight 0
    far = m4.copy()
    far[3] = 1e4
    params = pack(np.full(4, 0.25, np.float32), far, v4 * 2)
    lse = Kn.gmm_estep(xt, st, params, 4)[0]
    nk = Kn.gmm_mstep(xt, st, params, 4, lse=lse)
    gw, gm, gv = model_of(params, 4, 64)
    assert nk[3].item() == 0 and gw[3] == 0 and np.array_equal(gm[3], far[3]) and (gv[3] == 2).all()
    assert abs(gw.astype(np.float64).sum() - 1) < 1e-6 and np.isneginf(Kn.gmm_view(params, 4, 64, 'logc')[3].item())
    assert torch.isfinite(Kn.gmm_estep(xt, st, params, 4)[0]).all()                    # and the next E-step skips it
    # NaN: loses to every number; a NaN a_ik makes lse NaN; an all-NaN row gets label 0
    mn = np.array(m, copy=True)
    mn[0] = np.nan
    lse, lab, _, bound = Kn.gmm_estep(xt, st, pack(w, mn, v), 3)
    assert torch.isnan(lse).all() and not (lab == 0).any()
    assert np.isnan(bound.item())
    xn = np.array(x, copy=True)
    xn[7] = np.nan
    lse, lab, _, _ = Kn.gmm_estep(gpu(xn), st, pack(w, m, v), 3)
    assert np.isnan(lse[7].item()) and lab[7].item() == 0 and torch.isfinite(lse[:7]).all()


# ---- sampling --------------------------------------------------------------------------------------------------------
def test_sample_with_injected_uniforms_and_normals():
    Kn = kernels()
    rng = np.random.default_rng(3)
    K, Z, n = 5, 8, 600
    w = np.array([0.25, 0.0, 0.5, 0.25, 0.0], np.float32)
    below = np.nextafter(np.float32(0.25), np.float32(0))
    edges = np.array([0.0, below, 0.25, 0.5, np.nextafter(np.float32(0.75), np.float32(0)), 0.75, 1 - 2.0 ** -24],
                     np.float32)
    u = np.concatenate([edges, rng.random(n - len(edges)).astype(np.float32)])
    # dyadic: sd in {0.5, 1, 2}, eps and means multiples of 2^-6 below 8: the product-sum is exact in f32
    m = (rng.integers(-256, 257, (K, Z)) / 64).astype(np.float32)
    v = rng.choice([0.25, 1.0, 4.0], (K, Z)).astype(np.float32)
    eps = (rng.integers(-256, 257, (n, Z)) / 64).astype(np.float32)
    comp, z, exact = R.sample(w, m, v, u, eps)
    assert exact.all() and comp[:7].tolist() == [0, 0, 2, 2, 2, 3, 3]
    zt, ct = Kn.gmm_sample(pack(w, m, v), K, Z, n, u=gpu(u), eps=gpu(eps))
    assert np.array_equal(ct.cpu().numpy(), comp) and np.array_equal(zt.cpu().numpy().astype(np.float64), z)
    assert not np.isin(ct.cpu().numpy(), [1, 4]).any()                  # a weight-0 component is never drawn
    # general values: fmaf rounds once, so within half an ulp of the f64 value (1 ulp allowed)
    m = rng.standard_normal((K, Z)).astype(np.float32)
    v = rng.uniform(0.2, 3.0, (K, Z)).astype(np.float32)
    eps = rng.standard_normal((n, Z)).astype(np.float32)
    comp, z, _ = R.sample(w, m, v, u, eps)
    zt, ct = Kn.gmm_sample(pack(w, m, v), K, Z, n, u=gpu(u), eps=gpu(eps))
    got = zt.cpu().numpy()
    assert np.array_equal(ct.cpu().numpy(), comp)
    assert (np.abs(got.astype(np.float64) - z) <= np.spacing(np.abs(z).astype(np.float32))).all()


def test_sample_with_the_library_rng():
    Kn = kernels()
    K, Z, n = 4, 16, 200_000
    w = np.array([0.2, 0.0, 0.5, 0.3], np.float32)
    m = np.arange(K * Z, dtype=np.float32).reshape(K, Z) / 8 - 3
    v = np.tile(np.array([[0.25], [1.0], [2.0], [0.5]], np.float32), (1, Z))
    params = pack(w, m, v)
    z, comp = Kn.gmm_sample(params, K, Z, n, seed=11)
    z2, comp2 = Kn.gmm_sample(params, K, Z, n, seed=11)
    assert torch.equal(z, z2) and torch.equal(comp, comp2)             # one seed, one result
    z3, comp3 = Kn.gmm_sample(params, K, Z, n, seed=12)
    assert not torch.equal(comp, comp3) and not torch.equal(z, z3)
    comp, z = comp.cpu().numpy(), z.cpu().numpy().astype(np.float64)
    counts = np.bincount(comp, minlength=K)
    assert counts[1] == 0
    for k in (0, 2, 3):
        p = float(w[k])
        dev = abs(counts[k] - n * p) / np.sqrt(n * p * (1 - p))
        zk = z[comp == k]
        nk = len(zk)
        mean_dev = np.abs(zk.mean(axis=0) - m[k]) / np.sqrt(v[k] / nk)
        var_dev = np.abs(zk.var(axis=0) - v[k]) / (v[k] * np.sqrt(2.0 / nk))
        print(f'component {k}: count {dev:.2f} sigma, mean {mean_dev.max():.2f} sigma, var {var_dev.max():.2f} sigma')
        assert dev < 5 and (mean_dev < 5).all() and (var_dev < 5).all()
    # the one-component standard normal is svae_latent_draw(0, 1), bit for bit
    one = pack(np.ones(1, np.float32), np.zeros((1, Z), np.float32), np.ones((1, Z), np.float32))
    z1, c1 = Kn.gmm_sample(one, 1, Z, 5001, seed=77)
    zero = torch.zeros(5001, Z, device='cuda')
    assert torch.equal(z1, Kn.latent_draw(zero, torch.ones_like(zero), seed=77)) and (c1 == 0).all()


# ---- GaussianMixture -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case,tol', [((3, 64, True), 1e-2), ((R.TILE + 1, 68, False), 1e-1)])
def test_fit_follows_the_reference_on_overlapping_blobs(case, tol):
    from sparse_vae import GaussianMixture
    K, Z, _ = case
    x, s2, w0, m0, v0 = R.blob_case(*case)
    xt, st = gpu(x), gpu(s2)
    init = tuple(torch.from_numpy(np.array(t)) for t in (w0, m0, v0))
    fits = [GaussianMixture(K, tol=tol, reg_covar=R.REG, init=init, check_every=c, max_iter=40).fit(xt, st)
            for c in (4, 1, 5)]
    gm = fits[0]
    for other in fits[1:]:                                             # independent of check_every
        assert other.n_iter_ == gm.n_iter_ and other.lower_bounds_ == gm.lower_bounds_
        assert torch.equal(other._params, gm._params) and torch.equal(other.nk_, gm.nk_)
    t = gm.n_iter_
    assert gm.converged_ and 3 <= t < 40 and t == R.stop_iteration(gm.lower_bounds_, tol)
    assert gm.lower_bound_ == gm.lower_bounds_[-1] and len(gm.lower_bounds_) == t
    base, spread = R.fit_spread(case, t)
    b = gm.lower_bounds_
    for i in range(t - 1):                                             # non-decreasing within the per-step bound
        assert b[i + 1] >= b[i] - (base['lse_err'][i] + base['lse_err'][i + 1]), (i, b)
    got = dict(weight=gm.weights_, mean=gm.means_, var=gm.variances_)
    for name in ('weight', 'mean', 'var'):
        dev = np.abs(got[name].cpu().numpy().astype(np.float64) - base[name].astype(np.float64)).max()
        print(f'{name}: deviation {dev:.3e}, reference spread {spread[name]:.3e}, ratio {dev / spread[name]:.3f}')
        assert dev <= 4 * spread[name], (name, dev, spread[name])
    assert abs(gm.weights_.sum().item() - 1) < 1e-5 and abs(gm.nk_.sum().item() - len(x)) < 1e-3 * len(x)
    # the density and the assignments of the fitted model
    assert abs(gm.score(xt, st) - gm.score_samples(xt, st).double().mean().item()) < 1e-9 * abs(gm.score(xt, st))
    proba = gm.predict_proba(xt, st)
    assert torch.equal(gm.predict(xt, st), proba.argmax(dim=1)) and (proba.sum(dim=1) - 1).abs().max() < 1e-4
    n = len(x)
    assert abs(gm.bic(xt, st) - (-2 * gm.score(xt, st) * n + (2 * K * Z + K - 1) * np.log(n))) < 1e-6 * n
    z, comp = gm.sample(64, seed=3)
    assert z.shape == (64, 1, Z) and comp.shape == (64,) and comp.dtype == torch.int64 and z.is_cuda


def test_kmeans_starts_the_index_method_and_persistence(tmp_path):
    from sparse_vae import GaussianMixture, LatentIndex
    x, s2 = R.blob_case(3, 64, True)[:2]
    index = LatentIndex(64, 'cuda').add(gpu(x), gpu(np.sqrt(s2)))
    one = index.fit_mixture(3, seed=1)
    b = one.lower_bounds_
    step = 2 * R.estep(x, s2, *(t.cpu().numpy() for t in (one.weights_, one.means_, one.variances_)))['lse_err'].mean()
    assert one.converged_ and all(b[i + 1] >= b[i] - step for i in range(len(b) - 1)), b
    best = index.fit_mixture(3, n_init=3, seed=1)
    runs = [index.fit_mixture(3, seed=1 + r).lower_bound_ for r in range(3)]
    assert best.lower_bound_ == max(runs) and runs[0] == one.lower_bound_
    again = GaussianMixture(3, seed=1).fit(index)
    assert torch.equal(again._params, one._params)                     # one seed, one result
    points = index.fit_mixture(3, source='mean', seed=1)
    assert torch.equal(points._params, GaussianMixture(3, seed=1).fit(index.loc.contiguous())._params)
    assert points.variances_.mean().item() < one.variances_.mean().item()              # the posteriors' own variance
    path = str(tmp_path / 'prior.npz')
    one.save(path)
    back = GaussianMixture.load(path, 'cuda')
    assert torch.equal(back._params, one._params) and back.n_iter_ == one.n_iter_
    assert torch.equal(back.score_samples(index), one.score_samples(index))
    normal = GaussianMixture.standard_normal(64, 'cuda')
    z = torch.randn(100, 64, device='cuda')
    e = R.estep(z.cpu().numpy(), None, np.ones(1, np.float32), np.zeros((1, 64), np.float32), np.ones((1, 64), np.float32))
    want = -0.5 * (z.double() ** 2).sum(dim=1) - 32 * np.log(2 * np.pi)
    assert np.allclose(e['lse'], want.cpu().numpy(), rtol=1e-12)
    assert (np.abs(normal.score_samples(z).double().cpu().numpy() - e['lse']) <= e['lse_err']).all()
    assert one.score(index) > normal.score(index)


# ---- command line ---------------------------------------------------------------------------------------------------
def test_fit_prior_and_sample_with_a_prior(tmp_path):
    from sparse_vae import LatentIndex
    n, Z = 1500, 64
    loc = R.two_component_rows(n, Z)
    titles = [f'doc {i}' for i in range(n)]
    path, prior, out = tmp_path / 'latents.npz', tmp_path / 'prior.npz', tmp_path / 'samples.npz'
    LatentIndex(Z).add(torch.from_numpy(loc), torch.full((n, Z), 0.1), titles).save(path)

    def run(*argv):
        return subprocess.run([sys.executable, *map(str, argv)], capture_output=True, text=True, timeout=300, cwd=ROOT)

    r = run('fit_prior.py', path, '--k', 2, '--out', prior, '--holdout', 0.2, '--top', 3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    print(r.stdout)
    lines = r.stdout.splitlines()
    held = [ln for ln in lines if ln.strip().startswith('held out')][0].split()
    fitted = [ln for ln in lines if ln.strip().startswith('fitted')][0].split()
    assert float(held[-2]) > float(held[-1]) + 10 and float(fitted[-2]) > float(fitted[-1]) + 10   # beats N(0, I)
    assert sum(ln.startswith('component ') for ln in lines) == 2 and any('least likely' in ln for ln in lines)
    assert sum(ln.startswith('  ') and 'doc ' in ln for ln in lines) == 3 * 3
    with np.load(prior) as f:
        w, m = f['weights'], f['means']
    order = np.argsort(w)
    assert np.allclose(w[order], [0.3, 0.7], atol=0.05) and np.allclose(m[order].mean(axis=1), [-2, 1.5], atol=0.1)
    for extra in ((), ('--loop',)):
        r = run('sample.py', '--preset', 'tiny', '--prior', prior, '--num-samples', 10, '--slots', 4, '--max-length',
                16, '--seed', 5, '--out', out, *extra)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        with np.load(out) as f:
            assert f['ids'].shape == (10, 15) and f['components'].shape == (10,)
            assert set(f['components'].tolist()) <= {0, 1} and 'prior' in str(f['hparams'])
            comps = f['components'].copy() if not extra else comps
            assert np.array_equal(f['components'], comps)               # seeded: the same components either way
