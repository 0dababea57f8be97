"""The k-means kernels (csrc/kmeans.hip), sparse_vae.KMeans and the two scripts on the device, against the float64
restatement of tests/kmeans_ref.py. Exact cases (integer coordinates: every f32 distance and every f64 sum is exact in
any order) must EQUAL the reference; the blob cases compare every row's label with no exemption, which
test_kmeans_ref.py::test_blob_cases_leave_no_row_near_a_tie licenses on the CPU."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(a, dtype=None):
    t = torch.from_numpy(np.array(a))              # a copy: the cached cases are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def kernels():
    from sparse_vae import kernels as K
    return K


def test_geometry_of_the_cases():
    """Each size hits the boundary it is named for, read from the library's own constants."""
    from sparse_vae import _native
    K = kernels()
    assert _native.KMEANS_TILE_CENTROIDS == R.TILE
    for Z in R.ZS:
        assert K.kmeans_geometry(1000, 10, Z)[0] == R.rows_per_block(Z)
        assert K.kmeans_geometry(1000, 10, Z)[2] == R.TILE
    shapes = R.exact_shapes()
    for Z in R.ZS:
        Rz, C = R.rows_per_block(Z), R.TILE
        ns = {n for n, k, z in shapes if z == Z}
        ks = {k for n, k, z in shapes if z == Z}
        assert {65, Rz + 1, 2 * Rz + 1} <= ns and {1, 2, C, C + 1, 2 * C + 1, 257} <= ks
        assert any(n == k for n, k, z in shapes if z == Z)
        assert K.kmeans_geometry(Rz, 1, Z)[1] == 1 and K.kmeans_geometry(Rz + 1, 1, Z)[1] == 2      # a 1-row block
        assert K.kmeans_geometry(2 * Rz + 1, 1, Z)[1] == 3
        g = K.kmeans_geometry(2 * Rz + 1, C + 1, Z)
        assert g[3] > 1 and g[5] > 1 and g[7] > 1        # several sort blocks, row groups and seed blocks
    assert {z <= 64 for z in R.ZS} == {True, False} and 68 % 64 and 68 > 64
    assert 256 < 257 <= _native.KMEANS_MAX_K             # the counting sort's second bin per thread
    n_big = 256 * 2048 + 1                               # a sort block longer than one LDS chunk of 2048 labels
    assert K.kmeans_geometry(n_big, 3, 4)[4] > 2048
    assert K.kmeans_geometry(65537, 3, 4)[7] > 256       # the seed's prefix sums reach their third level


def prev_variants(n, K, want):
    rng = np.random.default_rng(n + K)
    return {'none': np.full(n, -1, np.int32), 'same': want.copy(), 'shifted': np.roll(want, 1),
            'junk': np.where(rng.random(n) < 0.5, want, K + 7).astype(np.int32)}


@pytest.mark.parametrize('n,K,Z', R.exact_shapes())
def test_assign_equals_the_reference_on_exact_cases(n, K, Z):
    Kn = kernels()
    x, cent = R.exact_case(n, K, Z)
    want_lab, want_d2, _, want_in = R.exact_assign(n, K, Z)
    xt, ct = gpu(x), gpu(cent)
    for name, prev in prev_variants(n, K, want_lab).items():
        label = gpu(prev)
        lab, d2, changed, inertia = Kn.kmeans_assign(xt, ct, label)
        assert lab.data_ptr() == label.data_ptr()
        assert np.array_equal(lab.cpu().numpy(), want_lab), name
        assert np.array_equal(d2.cpu().numpy().astype(np.float64), want_d2), name
        assert int(changed.item()) == int((prev != want_lab).sum()), name
        assert float(inertia.item()) == want_in, name
    lab2, d2n, _, _ = Kn.kmeans_assign(xt, ct, want_d2=False)
    assert d2n is None and np.array_equal(lab2.cpu().numpy(), want_lab)


def test_assign_all_nan_row_and_single_nan_centroid():
    Kn = kernels()
    x, _ = R.exact_case(65, 2, 4)
    lab, d2, changed, inertia = Kn.kmeans_assign(gpu(x), gpu(np.full((2, 4), np.nan, np.float32)),
                                                 gpu(np.zeros(65, np.int32)))
    assert (lab == 0).all() and torch.isnan(d2).all() and int(changed.item()) == 0 and np.isnan(inertia.item())
    cent = np.array([[np.nan] * 4, [1, 2, 3, 4]], np.float32)
    lab, d2, _, _ = Kn.kmeans_assign(gpu(x), gpu(cent))
    assert (lab == 1).all() and np.array_equal(d2.cpu().numpy(), R.assign(x, cent)[1])


@pytest.mark.parametrize('n,K,Z', R.exact_shapes())
def test_update_equals_the_reference_on_exact_cases(n, K, Z):
    Kn = kernels()
    x, cent = R.exact_case(n, K, Z)
    cent = np.nan_to_num(cent, nan=-3.0)
    true = R.exact_assign(n, K, Z)[0]
    rng = np.random.default_rng(n * 31 + K)
    variants = {'assigned': true, 'all in one': np.full(n, K - 1, np.int32),
                'random with junk': np.where(rng.random(n) < 0.8, rng.integers(0, K, n), rng.choice([-1, K, 1 << 30], n))}
    if n > 1 and K > 1:
        lone = np.zeros(n, np.int32)
        lone[n // 3] = K - 1                       # a cluster of one row; K > 2: empty clusters in between
        variants['one row'] = lone
    xt = gpu(x)
    for name, label in variants.items():
        label = np.asarray(label, np.int32)
        want_c, want_n = R.update(x, label, cent)
        ct = gpu(cent)
        got_c, got_n = Kn.kmeans_update(xt, gpu(label), ct)
        assert got_c.data_ptr() == ct.data_ptr()
        assert np.array_equal(got_n.cpu().numpy(), want_n), name
        assert got_c.cpu().numpy().tobytes() == want_c.tobytes(), name      # bit for bit, kept centroids included


def seed_uniforms(K, rng):
    u = rng.integers(0, 1024, K) / 1024.0
    if K > 1:
        u[rng.integers(1, K)] = 0.0
    if K > 2:
        u[rng.integers(1, K)] = 1023 / 1024.0
    return u.astype(np.float32)


@pytest.mark.parametrize('n,K,Z', [s for s in R.exact_shapes() if s[1] <= 65])
def test_seed_equals_the_reference_on_exact_cases(n, K, Z):
    Kn = kernels()
    x, _ = R.exact_case(n, K, Z)
    xt = gpu(x)
    rng = np.random.default_rng(n + 3 * K + Z)
    for first in (0.0, 1023 / 1024.0, None):
        u = seed_uniforms(K, rng)
        if first is not None:
            u[0] = first
        want = R.seed(x, K, u)
        rows, cent = Kn.kmeans_seed(xt, K, u=gpu(u))
        assert np.array_equal(rows.cpu().numpy(), want), (first, u)
        assert np.array_equal(cent.cpu().numpy(), x[want])
        pts = {x[r].tobytes() for r in want}
        assert len(pts) == len(want) or len({r.tobytes() for r in x}) < K   # duplicates are never drawn twice


def test_seed_identical_rows_and_too_few_points():
    Kn = kernels()
    x, _ = R.exact_case(65, 2, 4)
    same = np.tile(x[:1], (300, 1))
    u = np.array([0.5, 0.25, 0.75, 0.0], np.float32)
    rows, cent = Kn.kmeans_seed(gpu(same), 4, u=gpu(u))
    assert rows.tolist() == [150, 0, 0, 0] and np.array_equal(cent.cpu().numpy(), same[:4])
    two = np.concatenate([same, x[1:2]])
    assert Kn.kmeans_seed(gpu(two), 3, u=gpu(u[:3]))[0].tolist() == R.seed(two, 3, u[:3]).tolist() == [150, 300, 0]


def test_large_shapes_third_prefix_level_and_long_sort_blocks():
    """N = 256 * 2048 + 1 at Z = 4: sort blocks longer than one LDS chunk, 2049 seed blocks (three prefix levels),
    1025 assign row blocks. Exact data, so everything equals the reference."""
    Kn = kernels()
    n, K, Z = 256 * 2048 + 1, 3, 4
    x, cent = R.exact_case(n, K, Z)
    cent = np.nan_to_num(cent, nan=5.0)
    xt = gpu(x)
    want_lab, want_d2, _, want_in = R.assign(x, cent)
    lab, d2, changed, inertia = Kn.kmeans_assign(xt, gpu(cent))
    assert np.array_equal(lab.cpu().numpy(), want_lab) and float(inertia.item()) == want_in
    assert np.array_equal(d2.cpu().numpy().astype(np.float64), want_d2) and int(changed.item()) == n
    want_c, want_n = R.update(x, want_lab, cent)
    got_c, got_n = Kn.kmeans_update(xt, lab, gpu(cent))
    assert np.array_equal(got_n.cpu().numpy(), want_n) and got_c.cpu().numpy().tobytes() == want_c.tobytes()
    for u in ([0.5, 1023 / 1024.0, 0.0], [1023 / 1024.0, 0.5, 0.25], [0.0, 1 / 1024.0, 0.75]):
        u = np.asarray(u, np.float32)
        assert Kn.kmeans_seed(xt, K, u=gpu(u))[0].tolist() == R.seed(x, K, u).tolist(), u


# ---- Lloyd's loop against the reference's ---------------------------------------------------------------------------
@pytest.mark.parametrize('K,Z', R.BLOBS)
def test_kmeans_follows_the_reference_on_blobs(K, Z):
    from sparse_vae import KMeans
    x, cent0 = R.blob_case(K, Z)
    want = R.blob_lloyd(K, Z)
    xt = gpu(x)
    km = KMeans(K, init=gpu(cent0), max_iter=50, check_every=1).fit(xt)
    assert km.labels_.dtype == torch.int64 and km.counts_.dtype == torch.int64 and km.seed_rows_ is None
    assert np.array_equal(km.labels_.cpu().numpy(), want['labels'])           # every row, no exemption
    assert np.array_equal(km.counts_.cpu().numpy(), want['counts'])
    assert km.n_iter_ == want['n_iter']
    got_c, want_c = km.cluster_centers_.cpu().numpy().astype(np.float64), want['centers'].astype(np.float64)
    n = len(x)
    # one f32 ulp of the rounded quotient + the f64 sum of at most n terms (n 2^-53 of the mean magnitude)
    tol = np.spacing(np.abs(want['centers'])).astype(np.float64) + n * 2.0 ** -53 * np.abs(x).max()
    print(f'K {K} Z {Z}: centre error / tol {np.max(np.abs(got_c - want_c) / tol):.3f}, inertia rel '
          f'{abs(km.inertia_ - want["inertia"]) / want["inertia"]:.3e} (bound {R.dist_roundings(Z) * R.EPS24:.3e})')
    assert (np.abs(got_c - want_c) <= tol).all()
    assert abs(km.inertia_ - want['inertia']) <= (R.dist_roundings(Z) * R.EPS24 + n * 2.0 ** -53) * want['inertia']
    assert isinstance(km.inertia_, float)
    assert torch.equal(km.predict(xt), km.labels_)
    for every in (4, 7):
        other = KMeans(K, init=gpu(cent0), max_iter=50, check_every=every).fit(xt)
        assert torch.equal(other.cluster_centers_, km.cluster_centers_) and torch.equal(other.labels_, km.labels_)
        assert torch.equal(other.counts_, km.counts_) and other.inertia_ == km.inertia_
        assert other.n_iter_ == min(50, -(-km.n_iter_ // every) * every)


# ---- determinism, seeds, n_init, predict ----------------------------------------------------------------------------
def test_two_calls_agree_bit_for_bit():
    from sparse_vae import KMeans
    Kn = kernels()
    x, cent0 = R.blob_case(R.TILE + 1, 68)
    xt, ct = gpu(x), gpu(cent0)
    a, b = Kn.kmeans_assign(xt, ct), Kn.kmeans_assign(xt, ct)
    for s, t in zip(a, b):
        assert torch.equal(s, t)
    ua, ub = Kn.kmeans_update(xt, a[0], ct.clone()), Kn.kmeans_update(xt, a[0], ct.clone())
    assert torch.equal(ua[0], ub[0]) and torch.equal(ua[1], ub[1])
    sa, sb = Kn.kmeans_seed(xt, 33, seed=5), Kn.kmeans_seed(xt, 33, seed=5)
    assert torch.equal(sa[0], sb[0]) and torch.equal(sa[1], sb[1])
    rows = sa[0].cpu().numpy()
    assert rows.min() >= 0 and rows.max() < len(x) and len(set(rows.tolist())) == 33     # in range, distinct points
    assert not torch.equal(Kn.kmeans_seed(xt, 33, seed=6)[0], sa[0])
    f1, f2 = KMeans(5, seed=3, n_init=2).fit(xt), KMeans(5, seed=3, n_init=2).fit(xt)
    assert torch.equal(f1.cluster_centers_, f2.cluster_centers_) and torch.equal(f1.labels_, f2.labels_)
    assert torch.equal(f1.seed_rows_, f2.seed_rows_) and f1.inertia_ == f2.inertia_ and f1.n_iter_ == f2.n_iter_
    assert not torch.equal(KMeans(5, seed=4, n_init=1).fit(xt).seed_rows_, KMeans(5, seed=3, n_init=1).fit(xt).seed_rows_)


def test_n_init_keeps_the_start_with_the_least_inertia():
    from sparse_vae import KMeans
    x, _ = R.blob_case(R.TILE + 1, 64)
    xt = gpu(x)
    singles = [KMeans(6, seed=10 + r, n_init=1).fit(xt) for r in range(4)]
    inertias = [s.inertia_ for s in singles]
    best = singles[int(np.argmin(inertias))]        # argmin: the lowest r among ties
    km = KMeans(6, seed=10, n_init=4).fit(xt)
    assert km.inertia_ == best.inertia_ and torch.equal(km.seed_rows_, best.seed_rows_)
    assert torch.equal(km.cluster_centers_, best.cluster_centers_) and torch.equal(km.labels_, best.labels_)
    assert int(km.counts_.sum()) == len(x) and km.seed_rows_.dtype == torch.int64


def test_predict_and_the_index_method():
    from sparse_vae import KMeans, LatentIndex
    x, _ = R.blob_case(3, 64)
    xt = gpu(x)
    index = LatentIndex(64, device='cuda').add(xt, torch.ones_like(xt))
    a, b = index.kmeans(3, seed=1), KMeans(3, seed=1).fit(index.loc)
    assert a.n_iter_ < 100                          # converged: predict reproduces the labels
    assert torch.equal(a.cluster_centers_, b.cluster_centers_) and torch.equal(a.labels_, b.labels_)
    assert torch.equal(a.predict(index), a.labels_) and torch.equal(a.predict(xt[:, None, :]), a.labels_)
    assert torch.equal(KMeans(3, seed=1).fit_predict(xt), a.labels_)
    with pytest.raises(ValueError):
        KMeans(4).fit(xt[:3])


# ---- command line ---------------------------------------------------------------------------------------------------
def test_cluster_latents_and_tsne_clusters(tmp_path):
    from sparse_vae import LatentIndex
    rng = np.random.default_rng(5)
    centres = rng.integers(-6, 7, (4, 16)).astype(np.float32)
    which = rng.integers(0, 4, 300)
    loc = (centres[which] + 0.5 * rng.standard_normal((300, 16))).astype(np.float32)
    titles = [f'doc {i} of blob {which[i]}' for i in range(300)]
    path, out, emb = tmp_path / 'latents.npz', tmp_path / 'clusters.npz', tmp_path / 'tsne.npz'
    LatentIndex(16).add(torch.from_numpy(loc), torch.ones(300, 16), titles).save(path)

    def run(*argv):
        return subprocess.run([sys.executable, *map(str, argv)], capture_output=True, text=True, timeout=300, cwd=ROOT)

    r = run('cluster_latents.py', path, '--k', 4, '--out', out, '--top', 3)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(out, allow_pickle=False) as z:
        labels, centers, counts, inertia, tt = z['labels'], z['centers'], z['counts'], z['inertia'], z['titles']
    assert labels.shape == (300,) and centers.shape == (4, 16) and counts.shape == (4,) and inertia.shape == ()
    assert counts.sum() == 300 and np.array_equal(np.bincount(labels, minlength=4), counts) and list(tt) == titles
    assert float(inertia) > 0
    cluster, seen, sizes = None, 0, []
    for line in r.stdout.splitlines():
        if line.startswith('cluster '):
            cluster = int(line.split()[1].rstrip(':'))
            sizes.append(int(line.split()[2]))
            assert sizes[-1] == counts[cluster]
        elif line.startswith('  ') and cluster is not None:
            title = line.strip().split('  ', 1)[1]
            assert labels[titles.index(title)] == cluster, line
            seen += 1
    assert sizes == sorted(sizes, reverse=True) and len(sizes) == 4 and seen == sum(min(3, s) for s in sizes)

    r = run('tsne.py', path, '--out', emb, '--clusters', out, '--n-iter', 20, '--max-points', 200)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with np.load(emb, allow_pickle=False) as z:
        assert z['embedding'].shape == (200, 2) and np.array_equal(z['labels'], labels[z['rows']])
    bad = tmp_path / 'bad.npz'
    np.savez(bad, labels=labels[:299])
    r = run('tsne.py', path, '--out', emb, '--clusters', bad, '--n-iter', 20)
    assert r.returncode != 0 and 'holds labels of shape (299,)' in r.stderr and '300 rows' in r.stderr
