"""Float64 numpy restatement of the k-means contracts of include/svae.h (svae_kmeans_assign / _update / _seed) and of
sparse_vae.KMeans' Lloyd loop, computed from the same f32 inputs; the case generators of the k-means tests; and the
rounding bound of the device's f32 distance."""
import functools

import numpy as np

EPS24 = 2.0 ** -24

# The safety factor between the reference's smallest relative gap (d_second - d_best) / d_second and the distance's
# rounding bound under which the GPU tests demand identical labels for EVERY row. 2 of it are the two distances of the
# comparison. The rest covers a device centroid that differs from the reference's by one f32 ulp in a coordinate (the
# two f64 quotients agree to ~1e-13 relative, so an f32 rounding boundary can fall between them): that moves d2 by at
# most 2^-22 |c| sqrt(d2), relatively 4 (|c| / sqrt(d2)) 2^-24, and for the blobs below |c| / sqrt(d2) is about
# (centre scale 8) / (spread 1), i.e. 32 * 2^-24 per distance, less than dist_roundings(64) = 35. Total < 4 + slack.
GAP_FACTOR = 64.0


def dist_roundings(Z):
    """The device's d2 in units of 2^-24 d2, counted from the summation order in the header of csrc/kmeans.hip: each
    of the two fmaf chains takes Z / 2 FMAs (one rounding each on a partial sum of non-negative terms), every square
    carries the two roundings of its difference (d = fl(x - c): (1 + e)^2), and the chains' sum is one more."""
    return Z // 2 + 3


def sqdist(x, c, chunk_elems=1 << 22):
    """f64 [N, K] squared distances from direct differences of the f32 inputs."""
    x64, c64 = np.asarray(x, np.float64), np.asarray(c, np.float64)
    n, Z = x64.shape
    out = np.empty((n, c64.shape[0]))
    step = max(1, chunk_elems // max(1, c64.shape[0] * Z))
    with np.errstate(invalid='ignore'):
        for i in range(0, n, step):
            d = x64[i:i + step, None, :] - c64[None]
            out[i:i + step] = np.einsum('nkz,nkz->nk', d, d)
    return out


def winners(d):
    """Per row of d [N, K]: the smallest distance's index; ties to the lower index; NaN loses to every number (+inf
    included); an all-NaN row gets 0."""
    nan = np.isnan(d)
    lab = np.argmin(np.where(nan, np.inf, d), axis=1)
    rows = np.arange(d.shape[0])
    fix = nan[rows, lab] & ~nan.all(axis=1)        # only +inf numbers in the row, and a NaN before the first of them
    lab[fix] = np.argmax(~nan[fix], axis=1)
    lab[nan.all(axis=1)] = 0
    return lab


def assign(x, cent, prev=None):
    """-> (label int32 [N], d2 f64 [N], changed, inertia)."""
    d = sqdist(x, cent)
    lab = winners(d).astype(np.int32)
    d2 = d[np.arange(len(lab)), lab]
    changed = len(lab) if prev is None else int((np.asarray(prev) != lab).sum())
    return lab, d2, changed, float(d2.sum())


def update(x, label, cent):
    """-> (cent f32 [K, Z], count int32 [K]): the f64 mean of a cluster's rows rounded to f32; an empty cluster keeps
    its centroid; labels outside 0..K-1 are ignored."""
    x64 = np.asarray(x, np.float64)
    cent = np.array(cent, np.float32, copy=True)
    K = cent.shape[0]
    label = np.asarray(label)
    count = np.zeros(K, np.int32)
    for c in range(K):
        rows = np.flatnonzero(label == c)
        count[c] = len(rows)
        if len(rows):
            cent[c] = (x64[rows].sum(axis=0) / float(len(rows))).astype(np.float32)
    return cent, count


def seed(x, K, u):
    """k-means++ with the uniforms u [K] -> rows int32 [K]."""
    n = x.shape[0]
    u = np.asarray(u, np.float64)
    rows = [min(int(np.floor(u[0] * n)), n - 1)]
    mind = None
    for s in range(1, K):
        d = sqdist(x, x[rows[-1]][None])[:, 0]
        mind = d if mind is None else np.minimum(mind, d)
        cum = np.cumsum(mind)                      # f64, in row order
        total = cum[-1]
        if total == 0:
            rows.append(0)
        else:
            rows.append(min(int(np.searchsorted(cum, u[s] * total, side='right')), n - 1))   # first cum > target
    return np.asarray(rows, np.int32)


def lloyd(x, cent0, max_iter):
    """sparse_vae.KMeans' loop from cent0 polled every iteration: assign, update, stop after the first iteration in
    which no label changed. -> dict(centers, labels, counts, inertia, n_iter, gaps); labels and inertia are the last
    assignment's; gaps[i] is iteration i's smallest (d_second - d_best) / d_second over the rows (inf at K = 1)."""
    cent = np.array(cent0, np.float32, copy=True)
    label, gaps, n_iter = None, [], max_iter
    for it in range(1, max_iter + 1):
        d = sqdist(x, cent)
        if d.shape[1] > 1:
            two = np.partition(d, 1, axis=1)[:, :2]
            gaps.append(float(((two[:, 1] - two[:, 0]) / two[:, 1]).min()))
        else:
            gaps.append(float('inf'))
        new = winners(d).astype(np.int32)
        changed = len(new) if label is None else int((new != label).sum())
        label = new
        inertia = float(d[np.arange(len(new)), new].sum())
        cent, count = update(x, label, cent)
        if changed == 0:
            n_iter = it
            break
    return dict(centers=cent, labels=label, counts=count, inertia=inertia, n_iter=n_iter, gaps=gaps)


# ---- cases ------------------------------------------------------------------------------------------------------------
R_SMALL_Z, R_LARGE_Z, TILE = 512, 256, 32          # the values the tests check against svae_kmeans_geometry
ZS = (4, 64, 68, 256)


def rows_per_block(Z):
    return R_SMALL_Z if Z <= 64 else R_LARGE_Z


def exact_shapes():
    """(N, K, Z): N in {K, 65, R + 1, 2R + 1}, K in {1, 2, C, C + 1, 2C + 1, 257} (257: the sort's second bin per
    thread), every Z; not the full product, but every N with a small and a ragged K and every K at the largest N."""
    out = []
    for Z in ZS:
        R, C = rows_per_block(Z), TILE
        for n, K in ((1, 1), (C + 1, C + 1), (65, 2), (65, C), (2 * C + 1, 2 * C + 1), (R + 1, C + 1), (R + 1, 1),
                     (2 * R + 1, 1), (2 * R + 1, 2), (2 * R + 1, C), (2 * R + 1, C + 1), (2 * R + 1, 2 * C + 1),
                     (2 * R + 1, 257)):
            out.append((n, K, Z))
    return out


@functools.lru_cache(maxsize=None)
def exact_case(n, K, Z, salt=0):
    """Integer coordinates in [-15, 15]: every difference, square and partial sum is an integer below 2^24 at Z <= 256,
    so every f32 distance is exact in any order and every f64 sum is exact. Centroid K - 1 duplicates centroid 0 (the
    lower index must win), centroid 1 is a row of NaN (K >= 3), the first rows equal centroids, and rows repeat."""
    rng = np.random.default_rng(1000003 * n + 1009 * K + Z + 7919 * salt)
    x = rng.integers(-15, 16, (n, Z)).astype(np.float32)
    cent = rng.integers(-15, 16, (K, Z)).astype(np.float32)
    m = min(n, K)
    x[:m:2] = cent[:m:2]                           # rows equal to a centroid
    if n >= 8:
        x[n // 2] = x[3]                           # duplicate rows
        x[n - 1] = x[3]
    if K >= 2:
        cent[K - 1] = cent[0]
    if K >= 3:
        cent[1] = np.nan
    x.setflags(write=False)
    cent.setflags(write=False)
    return x, cent


@functools.lru_cache(maxsize=None)
def exact_assign(n, K, Z):
    x, cent = exact_case(n, K, Z)
    return assign(x, cent)


BLOBS = ((3, 64), (TILE + 1, 64), (3, 68), (TILE + 1, 68))   # (K, Z); N = 2R + 1


@functools.lru_cache(maxsize=None)
def blob_case(K, Z, seed_=0):
    """f32 unit Gaussians around K separated centres (integer coordinates in [-8, 8], so two centres are about
    sqrt(48 Z) apart against a cluster radius of sqrt(Z)); cent0 = the centres moved by N(0, 2^2) noise."""
    n = 2 * rows_per_block(Z) + 1
    rng = np.random.default_rng(424243 + 131 * K + Z + 17 * seed_)
    centres = rng.integers(-8, 9, (K, Z)).astype(np.float64)
    which = rng.integers(0, K, n)
    which[:K] = np.arange(K)                       # no blob is empty
    x = (centres[which] + rng.standard_normal((n, Z))).astype(np.float32)
    cent0 = (centres + 2.0 * rng.standard_normal((K, Z))).astype(np.float32)
    x.setflags(write=False)
    cent0.setflags(write=False)
    return x, cent0


@functools.lru_cache(maxsize=None)
def blob_lloyd(K, Z, seed_=0):
    x, cent0 = blob_case(K, Z, seed_)
    return lloyd(x, cent0, 50)
