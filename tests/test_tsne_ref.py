"""t-SNE without a GPU: the float64 yardstick of tests/tsne_ref.py against the definition it restates (the gradient
of KL(P || Q) by finite differences), the host-side reverse-edge lists, and the argument checks of the new surface
(TSNE, the svae_tsne_* entry points), which all happen before any launch."""
import numpy as np
import pytest
import torch

import tsne_ref as R


def _graph(x, k):
    """Exact k nearest other rows of x by squared distance: (dist [N, k], idx [N, k])."""
    d = ((x[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind='stable')[:, :k]
    return np.take_along_axis(d, idx, 1), idx


def _kl(y, P):
    d = y[:, None, :] - y[None, :, :]
    q = 1.0 / (1.0 + (d * d).sum(-1))
    np.fill_diagonal(q, 0.0)
    Q = q / q.sum()
    m = P > 0
    return (P[m] * np.log(P[m] / Q[m])).sum()


def test_gradient_is_the_finite_difference_of_kl():
    """4 (attract64 / 2N - repulse64 / Z) is dKL(P || Q) / dy for the coalesced symmetric P = (p_j|i + p_i|j) / 2N:
    the yardstick is the gradient, and the two directed halves add up to the symmetric force."""
    N, k = 40, 8
    rng = np.random.default_rng(5)
    x = rng.standard_normal((N, 6))
    dist, idx = _graph(x, k)
    p, _ = R.affinities64(dist, 4.0)
    P = np.zeros((N, N))
    np.add.at(P, (np.repeat(np.arange(N), k), idx.reshape(-1)), p.reshape(-1))
    P = (P + P.T) / (2.0 * N)
    assert abs(P.sum() - 1.0) < 1e-12
    y = rng.standard_normal((N, 2))
    rep, _, zsum = R.repulse64(y)
    grad = 4.0 * (R.attract64(y, idx, p) / (2.0 * N) - rep / zsum)
    h, fd = 1e-6, np.zeros_like(y)
    for i in range(N):
        for c in range(2):
            yp, ym = y.copy(), y.copy()
            yp[i, c] += h
            ym[i, c] -= h
            fd[i, c] = (_kl(yp, P) - _kl(ym, P)) / (2 * h)
    err = np.abs(grad - fd).max() / np.abs(fd).max()
    print(f'gradient vs central difference: {err:.2e} of the largest component')
    assert err <= 1e-6


def test_update64_with_unit_exaggeration_descends_kl():
    N, k = 40, 8
    rng = np.random.default_rng(6)
    dist, idx = _graph(rng.standard_normal((N, 6)), k)
    p, _ = R.affinities64(dist, 4.0)
    P = np.zeros((N, N))
    np.add.at(P, (np.repeat(np.arange(N), k), idx.reshape(-1)), p.reshape(-1))
    P = (P + P.T) / (2.0 * N)
    y = rng.standard_normal((N, 2))
    rep, _, zsum = R.repulse64(y)
    y1, vel, gains, g = R.update64(y, np.zeros_like(y), np.ones_like(y), R.attract64(y, idx, p), rep, zsum, N, 1.0, 1.0,
                                   0.5)
    assert np.allclose(gains, 0.8) and np.allclose(vel, -0.8 * g)      # vel = 0: no strictly opposite sign
    assert _kl(y1, P) < _kl(y, P)


def _brute_reverse(nbr):
    n, k = nbr.shape
    by_target = {i: [] for i in range(n)}
    for j in range(n):
        for s in range(k):
            by_target[int(nbr[j, s])].append(j * k + s)
    return by_target


@pytest.mark.parametrize('n,k', [(50, 7), (9, 1), (2, 1)])
def test_reverse_edges_against_brute_force(n, k):
    from sparse_vae.tsne import reverse_edges
    rng = np.random.default_rng(n)
    nbr = np.empty((n, k), np.int64)
    allowed = np.arange(0, max(2, n // 2))         # the upper half of the rows is in nobody's list
    for i in range(n):
        pool = allowed[allowed != i]
        nbr[i] = rng.choice(pool, size=k, replace=False)
        if i != 0:
            nbr[i, 0] = 0                              # row 0 is a hub: in every other row's list
            if k > 1 and (nbr[i, 1:] == 0).any():
                nbr[i, 1:][nbr[i, 1:] == 0] = 1 if i != 1 else 2
    rev_ptr, rev_edge = reverse_edges(torch.from_numpy(nbr))
    assert rev_ptr.dtype == torch.int32 and rev_edge.dtype == torch.int32
    assert rev_ptr.shape == (n + 1,) and rev_edge.shape == (n * k,)
    want = _brute_reverse(nbr)
    rp, re_ = rev_ptr.tolist(), rev_edge.tolist()
    assert rp[0] == 0 and rp[-1] == n * k
    for i in range(n):
        assert re_[rp[i]:rp[i + 1]] == want[i], i
    assert len(want[0]) >= n - 1                       # the hub
    assert any(len(v) == 0 for v in want.values()) or n == 2
    assert sorted(re_) == list(range(n * k))
    # int32 input, as LatentIndex.knn_graph returns it
    rp2, re2 = reverse_edges(torch.from_numpy(nbr.astype(np.int32)))
    assert torch.equal(rp2, rev_ptr) and torch.equal(re2, rev_edge)


@pytest.mark.parametrize('k,perplexity', [(2, 1.5), (20, 5.0), (45, 15.0), (64, 21.3)])
def test_affinities64_hits_the_perplexity(k, perplexity):
    rng = np.random.default_rng(k)
    dist = rng.random((30, k)) * rng.choice([1e-6, 1.0, 1e6], size=(30, 1)) + 0.01
    p, beta = R.affinities64(dist, perplexity)
    assert np.abs(p.sum(-1) - 1.0).max() < 1e-12
    assert np.abs(R.entropy64(p) - np.log(perplexity)).max() <= 1e-9
    assert np.abs(p - R.softmax64(dist, beta)).max() < 1e-14


def test_affinities64_degenerate_rows():
    dist = np.stack([np.full(20, 3.0), np.zeros(20)])
    p, _ = R.affinities64(dist, 5.0)
    assert np.isfinite(p).all() and np.allclose(p, 1.0 / 20, rtol=1e-14)


def test_tsne_refuses_cpu_input():
    from sparse_vae import LatentIndex, TSNE
    x = torch.randn(30, 8)
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        TSNE(perplexity=5.0).fit_transform(x)
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        TSNE(perplexity=5.0).fit_transform(LatentIndex(8).add(x, torch.ones_like(x)))
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        TSNE(perplexity=5.0).fit_graph(torch.rand(30, 16), torch.zeros(30, 16, dtype=torch.int32))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        from sparse_vae import kernels as K
        K.tsne_repulse(torch.zeros(4, 2))


def test_tsne_argument_checks():
    from sparse_vae import TSNE
    with pytest.raises(ValueError):
        TSNE(perplexity=30, n_neighbors=20)
    with pytest.raises(ValueError):
        TSNE(perplexity=1.0)
    with pytest.raises(ValueError):
        TSNE(metric='cosine')
    with pytest.raises(ValueError):
        TSNE(perplexity=20.0)._neighbors(15)           # 14 other rows cannot carry perplexity 20
    assert TSNE(perplexity=20.0)._neighbors(10 ** 6) == 60 and TSNE(perplexity=30.0)._neighbors(10 ** 6) == 63
    assert TSNE(perplexity=15.0)._neighbors(300) == 45


def test_knn_graph_argument_checks():
    from sparse_vae import LatentIndex
    x = torch.randn(30, 8)
    index = LatentIndex(8).add(x, torch.ones_like(x))
    with pytest.raises(ValueError):
        index.knn_graph(5, metric='cosine')
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        index.knn_graph(5)


def test_bad_arguments_are_rejected_without_launch():
    """NULL operands, N < 2, k outside 1..64, N * k >= 2^31 and a perplexity outside (1, k) return SVAE_EINVAL
    before any launch, so this runs without a GPU."""
    from sparse_vae import _native
    lib, P = _native.lib, 4096                          # P: a non-NULL, aligned address that is never dereferenced
    assert lib.svae_tsne_affinities(None, 10, 8, 3.0, P, P, None) == 1
    assert lib.svae_tsne_affinities(P, 10, 8, 3.0, None, P, None) == 1
    assert lib.svae_tsne_affinities(P, 10, 8, 3.0, P, None, None) == 1
    assert lib.svae_tsne_affinities(P, 0, 8, 3.0, P, P, None) == 1
    for k in (0, 65, -1):
        assert lib.svae_tsne_affinities(P, 10, k, 3.0, P, P, None) == 1
    for perp in (1.0, 8.0, 0.5, 9.0, float('nan')):
        assert lib.svae_tsne_affinities(P, 10, 8, perp, P, P, None) == 1
    assert lib.svae_tsne_affinities(P, 2 ** 25, 64, 3.0, P, P, None) == 1         # N * k = 2^31

    assert lib.svae_tsne_repulse_ws_bytes(1) == 0 and lib.svae_tsne_repulse_slice_cols(1) == 0
    nbytes = lib.svae_tsne_repulse_ws_bytes(1000)
    assert nbytes > 0 and nbytes % 8 == 0
    assert lib.svae_tsne_repulse(None, 1000, P, nbytes, P, P, P, None) == 1
    assert lib.svae_tsne_repulse(P, 1000, None, nbytes, P, P, P, None) == 1
    assert lib.svae_tsne_repulse(P, 1000, P, nbytes - 8, P, P, P, None) == 1       # workspace too small
    assert lib.svae_tsne_repulse(P, 1000, P, nbytes, None, P, P, None) == 1
    assert lib.svae_tsne_repulse(P, 1000, P, nbytes, P, None, P, None) == 1
    assert lib.svae_tsne_repulse(P, 1000, P, nbytes, P, P, None, None) == 1
    assert lib.svae_tsne_repulse(P, 1, P, nbytes, P, P, P, None) == 1
    big = 2 ** 24 + 1                                   # more rows than 2^24: 2N would not be exact in f32
    assert lib.svae_tsne_repulse_ws_bytes(big) == 0 and lib.svae_tsne_repulse_slice_cols(big) == 0
    assert lib.svae_tsne_repulse_ws_bytes(2 ** 31 - 1) == 0 and lib.svae_tsne_repulse_slice_cols(2 ** 31 - 1) == 0
    assert lib.svae_tsne_repulse(P, big, P, 2 ** 40, P, P, P, None) == 1

    good = [P, P, P, P, P, 1000, 8, P, None]
    for i in (0, 1, 2, 3, 4, 7):
        args = list(good)
        args[i] = None
        assert lib.svae_tsne_attract(*args) == 1, i
    for n, k in ((1, 8), (1000, 0), (1000, 65), (2 ** 25, 64)):
        assert lib.svae_tsne_attract(P, P, P, P, P, n, k, P, None) == 1

    good = [P, P, P, P, P, P, 1000, 12.0, 200.0, 0.5, None]
    for i in range(6):
        args = list(good)
        args[i] = None
        assert lib.svae_tsne_update(*args) == 1, i
    assert lib.svae_tsne_update(P, P, P, P, P, P, 1, 12.0, 200.0, 0.5, None) == 1
    assert lib.svae_tsne_update(P, P, P, P, P, P, 2 ** 24 + 1, 12.0, 200.0, 0.5, None) == 1


def test_repulse_geometry_depends_on_n_alone():
    """The slice width is a whole number of tiles, the slices cover the columns, and the workspace holds them."""
    from sparse_vae import _native
    lib = _native.lib
    for n in (2, 3, 256, 257, 512, 513, 4097, 65536, 524288, 2 ** 24):
        cols = lib.svae_tsne_repulse_slice_cols(n)
        slices = -(-n // cols)
        assert cols % _native.TSNE_TILE_COLS == 0 and 1 <= slices <= 64
        assert (slices - 1) * cols < n <= slices * cols
        assert lib.svae_tsne_repulse_ws_bytes(n) == (slices * 3 * n * 4 + 7) // 8 * 8 + -(-n // 256) * 8
    assert lib.svae_tsne_repulse_slice_cols(513) == 256 and lib.svae_tsne_repulse_slice_cols(65536) == 4096
