"""The t-SNE kernels (csrc/tsne.hip), LatentIndex.knn_graph, sparse_vae.TSNE and tsne.py on the device, each against the
float64 restatement of tests/tsne_ref.py computed from the same f32 inputs. EPS24 = 2^-24 is the unit roundoff of f32;
every bound below counts roundings in that unit, relative to the sum of the absolute values of the terms added."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import tsne_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS24 = 2.0 ** -24
TINY = 2.0 ** -126          # below the smallest normal f32 a value has absolute, not relative, precision


def dev():
    return torch.device('cuda', 0)


def gpu(a, dtype=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dtype)


def f64(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- affinities ------------------------------------------------------------------------------------------------------
AFF_CASES = [(k, perp) for k in (2, 31, 45, 63, 64) for perp in (1.5, 15.0, k / 3.0) if 1.0 < perp < k]


@pytest.mark.parametrize('n', [1, 63, 65, 1000])
@pytest.mark.parametrize('k,perp', AFF_CASES)
def test_affinities(k, perp, n):
    from sparse_vae import kernels as K
    rng = np.random.default_rng(1000 * k + n)
    dist = (rng.random((n, k)) * 4.0 + 0.01).astype(np.float32)
    if n > 1:
        dist[0] *= np.float32(1e-6)
        dist[-1] *= np.float32(1e6)
    p_t, beta_t = K.tsne_affinities(gpu(dist), perp)
    p, beta = f64(p_t), f64(beta_t)
    assert np.isfinite(p).all() and np.isfinite(beta).all() and (beta > 0).all()
    assert (p >= 0).all()
    assert np.abs(p.sum(-1) - 1.0).max() <= (k + 8) * EPS24
    order = np.argsort(dist, axis=1, kind='stable')
    assert (np.diff(np.take_along_axis(p, order, 1), axis=1) <= 0).all(), 'p must not increase with the distance'
    want = R.softmax64(dist, beta)
    err = np.abs(p - want) / ((k + 16) * EPS24 * want + TINY)
    h_err = np.abs(R.entropy64(p) - np.log(perp)).max()
    print(f'k {k} perplexity {perp:.3g} rows {n}: p err / bound {err.max():.3f}, entropy off by {h_err:.2e}')
    assert err.max() <= 1.0
    assert h_err <= 1e-4


def test_affinities_degenerate_rows():
    """All distances equal, all zero, and 40 tied minima at perplexity 15: no entropy target can be met; the rows
    still come out finite and normalised, the ties share the mass equally."""
    from sparse_vae import kernels as K
    k = 63
    rng = np.random.default_rng(3)
    tied = np.concatenate([np.full(40, 0.7), 0.7 + 0.5 + rng.random(k - 40)])
    dist = np.stack([np.full(k, 3.0), np.zeros(k), rng.permutation(tied)]).astype(np.float32)
    p_t, beta_t = K.tsne_affinities(gpu(dist), 15.0)
    p = f64(p_t)
    assert np.isfinite(p).all() and np.isfinite(f64(beta_t)).all()
    assert np.abs(p.sum(-1) - 1.0).max() <= (k + 8) * EPS24
    assert np.abs(p[:2] * k - 1.0).max() <= (k + 8) * EPS24
    ties = dist[2] == dist[2].min()
    assert ties.sum() == 40 and np.abs(p[2][ties] * 40 - 1.0).max() <= (k + 8) * EPS24 and (p[2][~ties] < 1e-30).all()


# ---- repulsion -------------------------------------------------------------------------------------------------------
# 513: one row more than a workgroup owns (SVAE_TSNE_ROWS_PER_BLOCK = 512). 257, 513 and 4097 put exactly one column
# in the last column slice (the slices are 256 columns wide at all three). Up to 16,384 rows a slice is a single LDS
# tile; REP_N_LOOP are the sizes at which a workgroup goes round its column-tile loop more than once, reusing the
# tile: 16,385 (2 tiles per slice) and 28,673 (4) with one column in the last slice, 32,769 (5) with one column in
# the last tile of the last slice. test_repulse_geometry_of_the_cases checks all of this against the library.
REP_N = [2, 3, 63, 64, 65, 257, 513, 4097]
REP_N_LOOP = [16385, 28673, 32769]


def test_repulse_geometry_of_the_cases():
    from sparse_vae import kernels as K
    rows, slices, cols = K.tsne_repulse_geometry(513)
    assert rows == 512 and 513 == rows + 1
    for n in (257, 513, 4097):
        rows, slices, cols = K.tsne_repulse_geometry(n)
        assert slices > 1 and cols == 256 and n - (slices - 1) * cols == 1
    for n, tiles_per_slice, last in zip(REP_N_LOOP, (2, 4, 5), (1, 1, 769)):
        rows, slices, cols = K.tsne_repulse_geometry(n)
        assert cols == 256 * tiles_per_slice and slices > 1 and n - (slices - 1) * cols == last
    assert 769 % 256 == 1


@pytest.mark.parametrize('n', REP_N + REP_N_LOOP)
def test_repulse_exact_counts(n):
    """Every point at (0, 0) or (1, 0): q is 1 or 1/2, every term and every partial sum is exact in f32, so the
    results are the pair counts themselves. A dropped, a doubled or a self pair changes a count. (The rows' sums stay
    below 2^24; their total, an integer, is added in f64 and rounded once, so it is the f32 nearest the count.)"""
    from sparse_vae import kernels as K
    site = np.random.default_rng(n).integers(0, 2, n)
    y = np.stack([site, np.zeros(n)], 1).astype(np.float32)
    rep, zrow, zsum = K.tsne_repulse(gpu(y))
    n1 = int(site.sum())
    same = np.where(site == 1, n1, n - n1)
    other = n - same
    want_z = (same - 1) + other / 2.0
    want_x = np.where(site == 1, 1.0, -1.0) * other / 4.0
    assert np.array_equal(f64(zrow), want_z)
    assert np.array_equal(f64(rep)[:, 0], want_x) and np.array_equal(f64(rep)[:, 1], np.zeros(n))
    assert want_z.max() < 2 ** 23 and want_z.sum() < 2 ** 53
    assert zsum.cpu().numpy()[0] == np.float32(want_z.sum())
    if n in REP_N_LOOP:
        rep2, zrow2, zsum2 = K.tsne_repulse(gpu(y))
        assert torch.equal(rep, rep2) and torch.equal(zrow, zrow2) and torch.equal(zsum, zsum2)


@pytest.mark.parametrize('std', [1.0, 10.0])
@pytest.mark.parametrize('n', REP_N)
def test_repulse_random(n, std):
    from sparse_vae import kernels as K
    rng = np.random.default_rng(7 * n + int(std))
    y = (rng.standard_normal((n, 2)) * std).astype(np.float32)
    dup = min(16, n // 2)
    y[n - dup:] = y[:dup]                                   # exact duplicates: q = 1, no force
    yt = gpu(y)
    rep, zrow, zsum = K.tsne_repulse(yt)
    rep2, zrow2, zsum2 = K.tsne_repulse(yt)
    assert torch.equal(rep, rep2) and torch.equal(zrow, zrow2) and torch.equal(zsum, zsum2)
    want_rep, want_z, want_sum, a_rep = R.repulse64(y, with_abs=True)
    # N - 1 additions in any order + 16 roundings inside a term (subtraction, two FMAs, the add of 1, a 1-ulp
    # reciprocal, the square, the product)
    bound = (n + 16) * EPS24
    r_rep = np.abs(f64(rep) - want_rep) / np.maximum(bound * a_rep, 1e-300)
    r_z = np.abs(f64(zrow) - want_z) / (bound * want_z)
    r_sum = abs(float(zsum.item()) - want_sum) / (bound * want_sum)
    print(f'N {n} std {std}: max err / bound rep {r_rep.max():.4f} zrow {r_z.max():.4f} zsum {r_sum:.4f}')
    assert r_rep.max() <= 1.0 and r_z.max() <= 1.0 and r_sum <= 1.0


@pytest.mark.parametrize('n', REP_N_LOOP[:2])
def test_repulse_random_where_the_tile_loop_repeats(n):
    """Random points at sizes where a slice is several LDS tiles. The float64 reference is computed for some 1,280
    of the rows (the first 256, the last 512 and a seeded sample of 512) against every column; zsum is
    checked against the f64 sum of the kernel's own zrow, which the exact-count test pins for all rows."""
    from sparse_vae import kernels as K
    rng = np.random.default_rng(n)
    y = (rng.standard_normal((n, 2)) * 10.0).astype(np.float32)
    y[n - 16:] = y[:16]
    yt = gpu(y)
    rep, zrow, zsum = K.tsne_repulse(yt)
    rep2, zrow2, zsum2 = K.tsne_repulse(yt)
    assert torch.equal(rep, rep2) and torch.equal(zrow, zrow2) and torch.equal(zsum, zsum2)
    rows = np.unique(np.concatenate([np.arange(256), np.arange(n - 512, n), rng.choice(n, 512, replace=False)]))
    want_rep, want_z, _, a_rep = R.repulse64(y, with_abs=True, rows=rows)
    bound = (n + 16) * EPS24
    r_rep = np.abs(f64(rep)[rows] - want_rep) / (bound * a_rep)
    r_z = np.abs(f64(zrow)[rows] - want_z) / (bound * want_z)
    total = f64(zrow).sum()
    r_sum = abs(float(zsum.item()) - total) / (EPS24 * total)          # exact f64 sum, one rounding to f32
    print(f'N {n}: max err / bound rep {r_rep.max():.4f} zrow {r_z.max():.4f}; zsum off its rows by {r_sum:.3f} '
          f'roundings')
    assert r_rep.max() <= 1.0 and r_z.max() <= 1.0 and r_sum <= 1.0


# ---- attraction ------------------------------------------------------------------------------------------------------
def hub_graph(n, k, rng):
    """Row 0 in every other row's list; the last quarter of the rows in nobody's."""
    allowed = np.arange(max(2, n - n // 4))
    nbr = np.empty((n, k), np.int64)
    for i in range(n):
        pool = allowed[allowed != i]
        nbr[i] = rng.choice(pool, size=k, replace=len(pool) < k)
        if i != 0 and 0 not in nbr[i]:
            nbr[i, rng.integers(k)] = 0
    return nbr


@pytest.mark.parametrize('n,k', [(2, 1), (65, 1), (65, 8), (65, 63), (1000, 1), (1000, 8), (1000, 63)])
def test_attract(n, k):
    from sparse_vae import kernels as K
    from sparse_vae.tsne import reverse_edges
    rng = np.random.default_rng(31 * n + k)
    nbr = hub_graph(n, k, rng)
    indeg = np.bincount(nbr.reshape(-1), minlength=n)
    assert indeg[0] >= n - 1 and (n < 8 or (indeg == 0).sum() >= n // 4)
    if k == 1:
        p = np.ones((n, 1), np.float32)
    else:
        p = R.affinities64(np.sort(rng.random((n, k)) * 3.0 + 0.1, axis=1), 3.0 if k == 8 else 15.0)[0]
        p = p.astype(np.float32)
    y = (rng.standard_normal((n, 2)) * 3.0).astype(np.float32)
    nbr_t = gpu(nbr, torch.int32)
    rev_ptr, rev_edge = reverse_edges(nbr_t)
    args = (gpu(y), nbr_t, gpu(p), rev_ptr, rev_edge)
    attr = K.tsne_attract(*args)
    assert torch.equal(attr, K.tsne_attract(*args))
    want, a = R.attract64(y, nbr, p, with_abs=True)
    bound = ((k + indeg)[:, None] + 16) * EPS24 * a
    ratio = np.abs(f64(attr) - want) / np.maximum(bound, 1e-300)
    print(f'N {n} k {k}: max err / bound {ratio.max():.4f} (largest in-degree {indeg.max()})')
    assert ratio.max() <= 1.0


# ---- update ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [2, 65, 1000])
def test_update(n):
    from sparse_vae import kernels as K
    rng = np.random.default_rng(n)
    y = rng.standard_normal((n, 2)).astype(np.float32)
    vel = (rng.standard_normal((n, 2)) * 0.1).astype(np.float32)
    attr = rng.standard_normal((n, 2)).astype(np.float32)
    rep = (rng.standard_normal((n, 2)) * n).astype(np.float32)
    gains = rng.choice([0.01, 0.011, 0.5, 1.0, 2.6], size=(n, 2)).astype(np.float32)
    flat = lambda a: a.reshape(-1)                                          # noqa: E731
    flat(vel)[::3] = 0.0                                                     # ties of the sign rule
    flat(attr)[1::4] = 0.0
    flat(rep)[1::4] = 0.0
    zsum = np.float32(0.37 * n * n)
    ex, lr, mom = np.float32(12.0), np.float32(max(n / 48.0, 50.0)), np.float32(0.8)
    yt, vt, gt = gpu(y), gpu(vel), gpu(gains)
    K.tsne_update(yt, vt, gt, gpu(attr), gpu(rep), gpu(np.array([zsum])), float(ex), float(lr), float(mom))
    g64 = R.update64(y, vel, gains, attr, rep, zsum, n, ex, lr, mom)[3]
    g_abs = 4.0 * (np.abs(float(ex) / (2.0 * n) * attr.astype(np.float64)) + np.abs(rep.astype(np.float64) / zsum))
    g_err = 8 * EPS24 * g_abs
    inc_gpu = f64(gt) > gains
    decided = (np.abs(g64) > g_err) | (g_abs == 0) | (vel == 0)
    assert n < 65 or (decided.mean() > 0.9 and (g_abs == 0).any() and (vel == 0).any())
    assert np.array_equal(inc_gpu[decided], (vel * g64 < 0)[decided]), 'gains branch'
    assert n < 65 or (inc_gpu.any() and (~inc_gpu).any())
    y64, v64, gn64, _ = R.update64(y, vel, gains, attr, rep, zsum, n, ex, lr, mom, inc=inc_gpu)
    t_vel = np.abs(float(mom) * vel.astype(np.float64)) + float(lr) * gn64 * g_abs
    r_g = np.abs(f64(gt) - gn64) / (8 * EPS24 * (gains + 0.2))
    r_v = np.abs(f64(vt) - v64) / np.maximum(8 * EPS24 * t_vel, 1e-300)
    r_y = np.abs(f64(yt) - y64) / (8 * EPS24 * (np.abs(y) + t_vel))
    print(f'N {n}: max err / bound gains {r_g.max():.3f} vel {r_v.max():.3f} y {r_y.max():.3f}')
    floored = (gains < 0.012) & ~inc_gpu                                     # 0.8 * gains falls below the floor
    assert (n < 65 or floored.any()) and (gt.cpu().numpy()[floored] == np.float32(0.01)).all()
    assert r_g.max() <= 1.0 and r_v.max() <= 1.0 and r_y.max() <= 1.0


# ---- knn_graph -------------------------------------------------------------------------------------------------------
def make_index(n, z, seed):
    from sparse_vae import LatentIndex
    g = torch.Generator().manual_seed(seed)
    loc = torch.randn(n, z, generator=g)
    scale = torch.rand(n, z, generator=g) * 1.5 + 0.1
    return LatentIndex(z).add(loc.to(dev()), scale.to(dev()))


@pytest.mark.parametrize('metric', ['l2', 'kl'])
@pytest.mark.parametrize('n,k,chunk', [(2, 1, 512), (64, 1, 512), (64, 10, 512), (64, 63, 512), (65, 1, 512),
                                       (65, 10, 7), (65, 63, 512), (1500, 1, 512), (1500, 10, 512), (1500, 63, 512)])
def test_knn_graph(n, k, chunk, metric):
    index = make_index(n, 16, n + k)
    dist, idx = index.knn_graph(k, metric, chunk=chunk)
    assert dist.shape == (n, k) and idx.shape == (n, k) and dist.dtype == torch.float32 and idx.dtype == torch.int32
    assert dist.is_cuda and idx.is_cuda
    i_np, d_np = idx.cpu().numpy(), dist.cpu().numpy()
    assert ((0 <= i_np) & (i_np < n)).all() and (i_np != np.arange(n)[:, None]).all()
    assert (np.diff(np.sort(i_np, 1), axis=1) > 0).all(), 'a row lists a neighbour twice'
    rows = torch.arange(n, device=dev())
    dense = index.scores(rows, metric)
    assert torch.equal(dist, dense.gather(1, idx.to(torch.int64))), 'a distance differs from LatentIndex.scores'
    s, h = index.search(rows, k + 1, metric)
    s, h = s.cpu().numpy(), h.cpu().numpy()
    for r in range(n):
        keep = [c for c in range(k + 1) if h[r, c] != r][:k]
        assert i_np[r].tolist() == h[r, keep].tolist() and d_np[r].tolist() == s[r, keep].tolist(), r


def test_knn_graph_of_identical_rows():
    """70 copies of one row, k = 63: every distance ties at 0, ties go to the lower row, so rows 64..69 are not among
    their own 64 hits; each still gets 63 distinct other rows."""
    from sparse_vae import LatentIndex
    loc = torch.full((70, 16), 0.25, device=dev())
    index = LatentIndex(16).add(loc, torch.ones_like(loc))
    dist, idx = index.knn_graph(63, 'l2')
    i_np = idx.cpu().numpy()
    assert (dist == 0).all() and (i_np != np.arange(70)[:, None]).all()
    assert (np.diff(np.sort(i_np, 1), axis=1) > 0).all() and ((0 <= i_np) & (i_np < 70)).all()
    _, hits = index.search(torch.arange(70, device=dev()), 64, 'l2')
    assert not (hits[69] == 69).any()


# ---- the whole fit ---------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def blob_data():
    x, labels = R.blobs(300, 64, 6, 0)
    return x, labels


def test_five_step_parity(blob_data):
    """Five optimiser steps from a unit-scale init, the device's own k-NN graph on both sides, against the float64
    restatement. The bar is the restatement's own float32 noise floor, measured here: t-SNE's early steps amplify
    rounding differences, so a longer run or a tiny init would compare noise with noise. Both sides stop the
    perplexity search by the specified rule (1e-5, 100 steps) and so land on the same beta: against a restatement
    calibrated to 1e-13 the device was measured 9.1e-4 off (the float32 floor, 6.2e-5 under the shared rule, was
    5.8e-5 with those affinities): all of it the 1e-5 of entropy the rule leaves, amplified like the rounding
    errors are."""
    from sparse_vae import LatentIndex, TSNE
    x, _ = blob_data
    loc = gpu(x)
    index = LatentIndex(64).add(loc, torch.ones_like(loc))
    dist, idx = index.knn_graph(45, 'l2')
    init = np.random.default_rng(11).standard_normal((300, 2)).astype(np.float32)
    tsne = TSNE(perplexity=15.0, n_neighbors=45)
    y_gpu = f64(tsne.fit_graph(dist, idx, gpu(init), n_iter=5))
    d_np, i_np = dist.cpu().numpy(), idx.cpu().numpy()
    y64 = R.fit64(d_np, i_np, init, 5, np.float64)
    y32 = R.fit64(d_np, i_np, init, 5, np.float32)
    floor = np.abs(y32.astype(np.float64) - y64).max()
    rms = np.sqrt((y64 ** 2).mean())
    err = np.abs(y_gpu - y64).max()
    bar = max(8 * floor, 1e-4 * rms)
    print(f'five steps: max |y_gpu - y_64| {err:.3e}, float32 floor {floor:.3e}, rms {rms:.3f}, err / bar '
          f'{err / bar:.3f}, err / floor {err / floor:.3f}')
    beta64 = R.affinities64(d_np, 15.0, tol=1e-5, steps=100)[1]
    same_beta = (f64(tsne.beta_) == beta64).mean()
    print(f'rows whose beta is the restatement\'s bit for bit: {same_beta:.3f}')
    assert np.isfinite(y_gpu).all() and err <= bar
    assert same_beta >= 0.9
    assert tsne.embedding_ is not None and tsne.beta_.shape == (300,) and tsne.knn_[0] is not None


def _purity(emb, labels, k=10):
    d = ((emb[:, None, :] - emb[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    nn = np.argsort(d, axis=1)[:, :k]
    return (labels[nn] == labels[:, None]).mean()


def test_quality_against_sklearn(blob_data):
    """400 iterations on six blobs against sklearn.manifold.TSNE (the reference's fallback without tsnecuda) on the
    CPU: trustworthiness and 10-NN label purity of the plane no worse than sklearn's less the seed-to-seed spread."""
    manifold = pytest.importorskip('sklearn.manifold')
    from sparse_vae import TSNE
    x, labels = blob_data
    ours_t = TSNE(perplexity=15, n_iter=400, seed=0).fit_transform(gpu(x))
    ours = f64(ours_t)
    again = TSNE(perplexity=15, n_iter=400, seed=0).fit_transform(gpu(x))
    assert torch.equal(ours_t, again), 'two fits with one seed differ'
    theirs = manifold.TSNE(perplexity=15, init='random', random_state=0).fit_transform(x)
    t_ours = manifold.trustworthiness(x, ours, n_neighbors=10)
    t_theirs = manifold.trustworthiness(x, theirs, n_neighbors=10)
    p_ours, p_theirs = _purity(ours, labels), _purity(theirs.astype(np.float64), labels)
    print(f'trustworthiness ours {t_ours:.4f} sklearn {t_theirs:.4f}; purity ours {p_ours:.4f} sklearn {p_theirs:.4f}')
    assert np.isfinite(ours).all()
    assert t_ours >= t_theirs - 0.03
    assert p_ours >= p_theirs - 0.02


def test_tsne_script(tmp_path):
    """tsne.py in a fresh process: a 500-row index file, a 200-row seeded subset, 50 iterations."""
    from sparse_vae import LatentIndex
    x, _ = R.blobs(500, 32, 5, 2)
    loc = torch.from_numpy(x)
    titles = [f'doc {i}' for i in range(500)]
    src, out = str(tmp_path / 'latents.npz'), str(tmp_path / 'tsne.npz')
    LatentIndex(32).add(loc, torch.full_like(loc, 0.5), titles).save(src)
    done = subprocess.run([sys.executable, os.path.join(ROOT, 'tsne.py'), src, '--out', out, '--max-points', '200',
                           '--n-iter', '50', '--perplexity', '10'], capture_output=True, text=True, timeout=300)
    assert done.returncode == 0, done.stderr[-2000:]
    with np.load(out, allow_pickle=False) as z:
        emb, rows, got = z['embedding'], z['rows'], [str(t) for t in z['titles']]
    assert emb.shape == (200, 2) and emb.dtype == np.float32 and np.isfinite(emb).all()
    assert rows.shape == (200,) and len(set(rows.tolist())) == 200 and rows.min() >= 0 and rows.max() < 500
    assert got == [titles[i] for i in rows.tolist()]
