"""k-means without a device: the float64 restatement of tests/kmeans_ref.py against brute-force loops, its tie / NaN /
empty-cluster / total == 0 rules, the condition under which the GPU tests may demand identical labels for every row
of the blob cases, the argument checks of the svae_kmeans_* entry points (which return before any launch), and the
Python and command-line surface."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import kmeans_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_assign(x, cent):
    lab, d2 = [], []
    for i in range(len(x)):
        best, bi = float('nan'), 0
        for c in range(len(cent)):
            d = 0.0
            for z in range(x.shape[1]):
                d += (float(x[i, z]) - float(cent[c, z])) ** 2
            if d < best or (best != best and d == d):
                best, bi = d, c
        lab.append(bi)
        d2.append(best)
    return np.array(lab), np.array(d2)


def test_assign_matches_a_triple_loop():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((23, 8)).astype(np.float32)
    cent = rng.standard_normal((5, 8)).astype(np.float32)
    lab, d2, changed, inertia = R.assign(x, cent)
    blab, bd2 = brute_assign(x, cent)
    assert (lab == blab).all() and np.allclose(d2, bd2, rtol=1e-13, atol=0)
    assert changed == 23 and abs(inertia - bd2.sum()) <= 1e-12 * bd2.sum()
    assert R.assign(x, cent, lab)[2] == 0
    assert R.assign(x, cent, np.roll(lab, 1))[2] == int((np.roll(lab, 1) != lab).sum())


def test_assign_tie_and_nan_rules():
    x = np.array([[0, 0, 0, 0], [2, 0, 0, 0], [1, 0, 0, 0]], np.float32)
    cent = np.array([[2, 0, 0, 0], [0, 0, 0, 0], [2, 0, 0, 0], [0, 0, 0, 0]], np.float32)
    lab, d2, _, _ = R.assign(x, cent)
    assert lab.tolist() == [1, 0, 0] and d2.tolist() == [0.0, 0.0, 1.0]     # duplicates and the midpoint: lower index
    cent[0] = np.nan
    lab, d2, _, _ = R.assign(x, cent)
    assert lab.tolist() == [1, 2, 1] and d2.tolist() == [0.0, 0.0, 1.0]     # NaN loses to every number
    lab, d2, _, inertia = R.assign(x, np.full((2, 4), np.nan, np.float32))
    assert lab.tolist() == [0, 0, 0] and np.isnan(d2).all() and np.isnan(inertia)
    d = np.array([[np.nan, np.inf, 3.0], [np.nan, np.inf, np.inf], [np.inf, np.nan, np.inf]])
    assert R.winners(d).tolist() == [2, 1, 0]
    for n, K, Z in R.exact_shapes()[:6]:
        x, cent = R.exact_case(n, K, Z)
        blab, bd2 = brute_assign(x[:9], cent)
        lab, d2, _, _ = R.assign(x[:9], cent)
        assert (lab == blab).all() and np.array_equal(d2, bd2, equal_nan=True)


def test_update_matches_a_loop_and_keeps_empty_clusters():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((40, 8)).astype(np.float32)
    cent0 = rng.standard_normal((6, 8)).astype(np.float32)
    label = rng.integers(0, 4, 40)                 # clusters 4 and 5 stay empty
    label[5], label[6], label[7] = -1, 6, 1 << 20  # ignored
    label[label == 3] = 2
    label[11] = 3                                  # a cluster of one row
    cent, count = R.update(x, label, cent0)
    for c in range(6):
        rows = [i for i in range(40) if label[i] == c]
        assert count[c] == len(rows)
        if not rows:
            assert np.array_equal(cent[c], cent0[c])
            continue
        s = np.zeros(8)
        for i in rows:
            s += x[i].astype(np.float64)
        want = (s / len(rows)).astype(np.float32)
        assert np.abs(cent[c].astype(np.float64) - want) .max() <= np.spacing(np.abs(want)).max()
    assert count.tolist()[3:] == [1, 0, 0] and np.array_equal(cent[3], x[11])
    assert cent.dtype == np.float32 and count.sum() == 37
    one, cnt = R.update(x, np.zeros(40, np.int64), cent0)
    assert cnt.tolist() == [40, 0, 0, 0, 0, 0] and np.array_equal(one[1:], cent0[1:])


def brute_seed(x, K, u):
    n = len(x)
    rows = [min(int(u[0] * n), n - 1)]
    mind = [float('inf')] * n
    for s in range(1, K):
        for i in range(n):
            d = sum((float(a) - float(b)) ** 2 for a, b in zip(x[i], x[rows[-1]]))
            mind[i] = min(mind[i], d)
        total = 0.0
        for m in mind:
            total += m
        pick, cum = 0, 0.0
        if total > 0:
            pick = n - 1
            for i, m in enumerate(mind):
                cum += m
                if cum > float(u[s]) * total:
                    pick = i
                    break
        rows.append(pick)
    return rows


def test_seed_matches_a_loop_and_its_rules():
    rng = np.random.default_rng(2)
    x = rng.integers(-15, 16, (30, 4)).astype(np.float32)
    x[7] = x[2]
    x[29] = x[2]
    for trial in range(8):
        u = rng.integers(0, 1024, 6) / 1024.0
        u[trial % 6] = 0.0 if trial % 2 else 1023 / 1024.0
        rows = R.seed(x, 6, u)
        assert rows.tolist() == brute_seed(x, 6, u)
        pts = {tuple(x[r]) for r in rows}
        assert len(pts) == 6                       # a row at distance 0 (chosen, or its duplicate) is never drawn
    assert R.seed(x, 3, [0.999, 0.0, 0.0])[0] == 29
    same = np.tile(x[:1], (9, 1))
    assert R.seed(same, 4, [0.5, 0.9, 0.1, 0.7]).tolist() == [4, 0, 0, 0]      # total == 0: row 0
    two = np.concatenate([same, x[1:2]])
    assert R.seed(two, 3, [0.0, 0.5, 0.5]).tolist() == [0, 9, 0]              # fewer distinct points than K


def test_lloyd_reaches_a_fixed_point():
    x, cent0 = R.blob_case(3, 64)
    out = R.lloyd(x, cent0, 50)
    assert out['n_iter'] < 50 and len(out['gaps']) == out['n_iter']
    lab, _, changed, inertia = R.assign(x, out['centers'], out['labels'])
    assert changed == 0 and abs(inertia - out['inertia']) <= 1e-12 * inertia
    assert out['counts'].sum() == len(x) and (out['counts'] > 0).all()
    assert R.lloyd(x[:5], cent0[:1], 50)['gaps'] == [float('inf'), float('inf')]


@pytest.mark.parametrize('K,Z', R.BLOBS)
def test_blob_cases_leave_no_row_near_a_tie(K, Z):
    """The condition under which test_kmeans_gpu.py exempts no row from its label comparison: in every iteration of
    the reference, every row's relative gap between its best and second-best distance exceeds the device distance's
    rounding bound by GAP_FACTOR (whose derivation is in kmeans_ref.py)."""
    out = R.blob_lloyd(K, Z)
    bound = R.dist_roundings(Z) * R.EPS24
    assert 2 <= out['n_iter'] < 50
    assert min(out['gaps']) > R.GAP_FACTOR * bound, (min(out['gaps']), bound)
    assert (out['counts'] > 0).all()
    assert len(R.blob_case(K, Z)[0]) == 2 * R.rows_per_block(Z) + 1


def test_rounding_bound_and_exact_cases():
    assert [R.dist_roundings(Z) for Z in R.ZS] == [5, 35, 37, 131]
    src = open(os.path.join(ROOT, 'sparse-vae_amd', 'csrc', 'kmeans.hip')).read()
    assert '(Z / 2 + 3) 2^-24 d2' in src
    for n, K, Z in R.exact_shapes():
        x, cent = R.exact_case(n, K, Z)
        assert x.shape == (n, Z) and cent.shape == (K, Z) and n >= K
        assert np.abs(x).max() <= 15 and np.nanmax(np.abs(cent)) <= 15
        assert Z * 30 * 30 < 2 ** 24 and n * Z * 30 * 30 < 2 ** 29


# ---- argument checks (no launch, so no GPU) --------------------------------------------------------------------------
def test_bad_arguments_are_rejected_without_launch():
    from sparse_vae import _native
    lib = _native.lib
    A, B, W, O = 4096, 8192, 1 << 20, 1 << 16      # non-null, aligned addresses that are never dereferenced
    MAXK = _native.KMEANS_MAX_K
    assert MAXK >= 1024
    shapes_bad = (dict(z=6), dict(z=0), dict(z=260), dict(k=0), dict(k=MAXK + 1, n=1 << 20), dict(k=101, n=100),
                  dict(n=0, k=1), dict(n=(1 << 24) + 1))

    def assign(x=A, n=1000, cent=B, k=10, z=16, label=O, d2=O + 4096, changed=O + 8192, inertia=O + 8200, ws=W,
               wsb=None):
        wsb = lib.svae_kmeans_assign_ws_bytes(n, k, z) if wsb is None else wsb
        return lib.svae_kmeans_assign(x, n, cent, k, z, label, d2, changed, inertia, ws, wsb, None)

    def update(x=A, n=1000, label=O, k=10, z=16, cent=B, count=O + 4096, ws=W, wsb=None):
        wsb = lib.svae_kmeans_update_ws_bytes(n, k, z) if wsb is None else wsb
        return lib.svae_kmeans_update(x, n, label, k, z, cent, count, ws, wsb, None)

    def seed(x=A, n=1000, k=10, z=16, u=None, rows=O, cent=B, ws=W, wsb=None):
        wsb = lib.svae_kmeans_seed_ws_bytes(n, k, z) if wsb is None else wsb
        return lib.svae_kmeans_seed(x, n, k, z, u, 1, rows, cent, ws, wsb, None)

    for fn, nulls in ((assign, ('x', 'cent', 'label', 'changed', 'inertia', 'ws')),
                      (update, ('x', 'label', 'cent', 'count', 'ws')), (seed, ('x', 'rows', 'cent', 'ws'))):
        for name in nulls:
            assert fn(**{name: None}) == 1, (fn.__name__, name)
        for bad in shapes_bad:
            assert fn(**bad) == 1, (fn.__name__, bad)
        assert fn(x=A + 4) == 1, fn.__name__                         # rows are 16-byte aligned
    for ws_bytes, fn in ((lib.svae_kmeans_assign_ws_bytes, assign), (lib.svae_kmeans_update_ws_bytes, update),
                         (lib.svae_kmeans_seed_ws_bytes, seed)):
        need = ws_bytes(1000, 10, 16)
        assert need > 0 and need % 8 == 0
        assert fn(wsb=need - 1) == 1 and fn(wsb=0) == 1
        for bad in shapes_bad:
            args = dict(n=1000, k=10, z=16)
            args.update(bad)
            assert ws_bytes(args['n'], args['k'], args['z']) == 0, bad
    geom = (ctypes.c_int32 * 8)()
    assert lib.svae_kmeans_geometry(1000, 10, 16, None) == 1
    for bad in shapes_bad:
        args = dict(n=1000, k=10, z=16)
        args.update(bad)
        assert lib.svae_kmeans_geometry(args['n'], args['k'], args['z'], ctypes.addressof(geom)) == 1
    assert list(geom) == [0] * 8                                     # nothing written


def test_workspace_and_geometry_formulas():
    """The documented geometry and workspaces (include/svae.h)."""
    from sparse_vae import _native, kernels as K
    lib = _native.lib
    assert (_native.KMEANS_MAX_K, _native.KMEANS_TILE_CENTROIDS, _native.KMEANS_SORT_BLOCKS,
            _native.KMEANS_SEED_BLOCK_ROWS) == (1024, 32, 256, 256)
    hdr = open(os.path.join(ROOT, 'include', 'svae.h')).read()
    for line in ('#define SVAE_KMEANS_MAX_K 1024', '#define SVAE_KMEANS_TILE_CENTROIDS 32',
                 '#define SVAE_KMEANS_SORT_BLOCKS 256', '#define SVAE_KMEANS_SEED_BLOCK_ROWS 256'):
        assert line in hdr

    def ceil(a, b):
        return -(-a // b)

    for n, k, z in [(1, 1, 4), (65, 2, 64), (1025, 33, 64), (513, 257, 68), (1 << 20, 1000, 64), (1 << 24, 1024, 64),
                    (1 << 24, 10, 256), (524289, 3, 4)]:
        rb = 512 if z <= 64 else 256
        want_blocks = min(ceil(n, 256), 256)
        rows_per = ceil(n, want_blocks)
        B = ceil(n, rows_per)
        bpg = ceil(B, max(1, min(4096 // k, B)))
        G = ceil(B, bpg)
        assert K.kmeans_geometry(n, k, z) == (rb, ceil(n, rb), 32, B, rows_per, G, 256, ceil(n, 256)), (n, k, z)
        assert lib.svae_kmeans_assign_ws_bytes(n, k, z) == ceil(n, rb) * 16
        assert lib.svae_kmeans_update_ws_bytes(n, k, z) == G * k * z * 8 + ceil((B * k + k + 1 + n) * 4, 8) * 8
        assert lib.svae_kmeans_seed_ws_bytes(n, k, z) == ceil(n, 256) * 8 + ceil(n * 4, 8) * 8
    assert lib.svae_kmeans_update_ws_bytes(1 << 24, 1024, 64) < 68 * (1 << 20)     # sensible at the largest shape


# ---- the Python and command-line surface ----------------------------------------------------------------------------
def test_kmeans_refuses_cpu_tensors():
    from sparse_vae import KMeans, LatentIndex
    x = torch.randn(20, 8)
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        KMeans(3).fit(x)
    index = LatentIndex(8).add(x, torch.ones_like(x))
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        index.kmeans(3)
    with pytest.raises(RuntimeError, match='There is no CPU fallback'):
        KMeans(3, init=torch.zeros(3, 8)).fit_predict(x)
    with pytest.raises(ValueError):
        KMeans(3, init='random')
    with pytest.raises(ValueError):
        KMeans(3, init=torch.zeros(4, 8))
    with pytest.raises(ValueError):
        KMeans(0)
    km = KMeans(5)
    assert (km.n_init, km.max_iter, km.init, km.seed, km.check_every) == (4, 100, 'k-means++', 0, 4)
    assert km.cluster_centers_ is None


@pytest.mark.parametrize('script,flags', [('cluster_latents.py', ('--k', '--out', '--n-init', '--max-iter', '--seed',
                                                                  '--top')),
                                          ('tsne.py', ('--clusters', '--plot', '--max-points'))])
def test_scripts_list_the_new_flags(script, flags):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script), '--help'], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in flags:
        assert flag in r.stdout, flag
