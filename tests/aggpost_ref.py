"""Float64 numpy restatement of the aggregate-posterior contracts of include/svae.h (svae_aggpost_logq / _decompose) and
of LatentIndex.elbo_surgery, computed from the same f32 inputs; the case generators of the tests; and the rounding
bounds of the device's f32 arithmetic, derived from the orders stated in the header of csrc/aggpost.hip. No bound here
is a hand-picked constant.

Units: u = 2^-24, the largest relative error of one f32 rounding. logf is the device library's, good to 1 ulp = 2 u;
v_exp_f32 is good to 1 ulp = 2 u. All bounds are first order in u.

The terms. With d = fl(z - loc), w = fl(1 / scale), t = fl(d w): t carries three roundings, t^2 six.
  joint    q = two fmaf chains of Z / 2 steps each on partial sums of non-negative terms (Z / 2 roundings relative to
           q), one add for the chains' sum, six from t^2: (Z / 2 + 7) u q. c_j = fl(-(sum_d logf(scale_jd)) - Z C), the
           sum in f64: 2 u |log scale| per dimension from logf, u |c_j| from the one rounding. l = fmaf(-0.5, q, c):
           one more rounding, u |l|. Together ((Z / 2 + 7) q / 2 + 2 sum_d |log scale_jd| + |c_j| + |l_ij|) u.
  per dim  l = fmaf(-0.5 t, t, nc), the product by -0.5 exact: 6 u t^2 / 2 from t^2, u |l| from the fmaf, and nc =
           -fl(logf(scale) + fl(C)): 2 u |log scale| from logf, u C from the constant, u |nc| <= u (|log scale| + C) from
           the add. Together (3 t^2 + 3 |log scale| + 2 C + |l|) u.

The log-sum-exp (lse_bound). d lse / d l_j = r_j, the term's share, so the terms' errors enter as sum_j r_j err_j. The
sum S itself, relative to the exact sum of the device's own terms:
  * every live term is exponentiated once, as ex(l_j - Mx) against the running maximum Mx <= max: the subtraction
    rounds once, the product by fl(log2 e) twice more (the constant and the product), all relative to the argument, so
    the argument is off by 3 u |l_j - Mx| <= 3 u |l_j - max|, and v_exp_f32 adds 2 u: the term is off by
    (3 |l_j - max| + 2) u of itself, sum_j r_j (3 |b_j| + 2) u of S with b_j = l_j - max. (The term that sets a new
    maximum is ex(0) = 1 exactly; the inexact exponential of that step is the rescale below.)
  * inside a tile of T rows the f32 sum s takes one fmaf per row: T u relative to s. A row that raises the maximum by a
    rescales s by ex(-a), off by (3 a + 2) u of the rescaled part, which holds at most T terms of at most e^-a each
    beside a new term of 1: a min(1, T e^-a) <= max(1, ln T) of the new s. That is at most T (3 + 3 max(1, ln T)) u
    relative to the tile's sum, hence to S (the tiles' sums add up to S with non-negative weights <= 1).
  * across tiles everything is f64 (the carried sum, the rescale by the library's exp of an exactly representable
    difference, the merge of the slices, log S and log n): 2^-52 per tile and a few more, against which u counts.
  * a term below 2^-126 of the maximum may be flushed by v_exp_f32: N 2^-126 in all, relative to S >= 1.
  * the output is rounded to f32 once: u |logq|.
So the f32 error does not grow with N: that is what the f64 carry is for.

decompose: every term and sum is f64; the reference adds in numpy's order, the device in its own: the two agree to
M 2^-52 times the sum of the terms' magnitudes (dec_bound)."""
import functools
import math

import numpy as np

EPS24 = 2.0 ** -24
HALF_LOG_2PI = 0.918938533204672741780

# Geometry the tests check against svae_aggpost_geometry (SVAE_AGGPOST_* of include/svae.h, mirrored in _native).
POINTS_PER_BLOCK, TILE_ROWS, PASS_DIMS = 256, 16, 16
MIN_SLICE_ROWS, TARGET_WG = 64, 1024
ZS = (4, 64, 68, 256)


def geometry(M, N, Z, per_dim):
    """svae_aggpost_geometry restated: (points per workgroup, point blocks, slices, rows per slice, tile rows,
    dimensions per pass)."""
    pb = -(-M // POINTS_PER_BLOCK)
    want = 1 if pb >= TARGET_WG else -(-TARGET_WG // pb)
    per = max(MIN_SLICE_ROWS, -(-N // want))
    rps = -(-per // TILE_ROWS) * TILE_ROWS
    return (POINTS_PER_BLOCK, pb, -(-N // rps), rps, TILE_ROWS, min(Z, PASS_DIMS) if per_dim else Z)


def ws_bytes(M, N, Z, per_dim):
    return geometry(M, N, Z, per_dim)[2] * M * ((1 + Z) if per_dim else 1) * 16


def shapes():
    """(M, N, Z) of the row-by-row GPU cases: per Z every N boundary at M = 65 and every M boundary at N = rows per
    slice + 1. N: one row, two, a tile less and more one row, one row into the second slice, one into the third. M: one
    point, a wave less and more one lane, one point into the second workgroup."""
    T, P, S = TILE_ROWS, POINTS_PER_BLOCK, MIN_SLICE_ROWS
    out = []
    for Z in ZS:
        out += [(65, n, Z) for n in (1, 2, T - 1, T + 1, S + 1, 2 * S + 1)]
        out += [(m, S + 1, Z) for m in (1, 63, P + 1)]
    return out


def _f64(*a):
    return tuple(np.asarray(x, np.float64) for x in a)


def _chunks(M, N, Z):
    step = max(1, (1 << 22) // (N * Z))
    return [(i, min(M, i + step)) for i in range(0, M, step)]


def joint_terms(z, loc, scale):
    """-> (l f64 [M, N], err f64 [M, N]): l_ij = sum_d l_ijd from direct differences of the f32 inputs, and the
    device's rounding bound."""
    z, loc, scale = _f64(z, loc, scale)
    M, Z = z.shape
    N = loc.shape[0]
    logs = np.log(scale)
    c = -logs.sum(axis=1) - Z * HALF_LOG_2PI
    alog = np.abs(logs).sum(axis=1)
    q = np.empty((M, N))
    for a, b in _chunks(M, N, Z):
        t = (z[a:b, None, :] - loc[None]) / scale[None]
        q[a:b] = (t * t).sum(axis=2)
    l = c[None] - 0.5 * q
    err = ((Z // 2 + 7) * 0.5 * q + 2 * alog[None] + np.abs(c)[None] + np.abs(l)) * EPS24
    return l, err


def dim_terms(z, loc, scale):
    """-> (l f64 [M, N, Z], err f64 [M, N, Z]): l_ijd and the device's rounding bound."""
    z, loc, scale = _f64(z, loc, scale)
    logs = np.log(scale)
    t = (z[:, None, :] - loc[None]) / scale[None]
    l = -0.5 * t * t - logs[None] - HALF_LOG_2PI
    err = (3 * t * t + 3 * np.abs(logs)[None] + 2 * HALF_LOG_2PI + np.abs(l)) * EPS24
    return l, err


def counts(M, N, skip):
    """n_i f64 [M]: N, or N - 1 where skip_i names a row."""
    n = np.full(M, float(N))
    if skip is not None:
        sk = np.asarray(skip)
        n[(sk >= 0) & (sk < N)] -= 1
    return n


def lse_bound(l, err, skip, axis_rows=1):
    """logsumexp over the rows (axis 1) of l [M, N] or [M, N, Z] minus log n_i, leaving out row skip_i -> (out, bound),
    the bound as derived in the module docstring."""
    l = np.array(l, np.float64)
    err = np.array(err, np.float64)
    M, N = l.shape[:2]
    if skip is not None:
        sk = np.asarray(skip)
        for i in np.nonzero((sk >= 0) & (sk < N))[0]:
            l[i, sk[i]] = -np.inf
            err[i, sk[i]] = 0.0
    n = counts(M, N, skip)
    n = n.reshape((M,) + (1,) * (l.ndim - 2))
    mx = l.max(axis=1, keepdims=True)
    with np.errstate(invalid='ignore'):
        b = np.where(np.isneginf(l), 0.0, l - mx)
        e = np.where(np.isneginf(l), 0.0, np.exp(b))
    S = e.sum(axis=1, keepdims=True)
    r = e / S
    out = (mx + np.log(S))[:, 0] - np.log(n)
    T = TILE_ROWS
    tiles = -(-N // T) + 8
    bound = ((r * err).sum(axis=1)
             + ((r * (3 * np.abs(b) + 2)).sum(axis=1) + T * (3 + 3 * max(1.0, math.log(T)))) * EPS24
             + N * 2.0 ** -126 + tiles * 2.0 ** -52 * (1 + np.abs(out))
             + np.abs(out) * EPS24)
    return out, bound


def logq(z, loc, scale, skip=None, per_dim=False):
    """-> dict(logq [M], logq_err [M], and with per_dim logq_dim [M, Z], logq_dim_err [M, Z]) in f64."""
    l, err = joint_terms(z, loc, scale)
    out = {}
    out['logq'], out['logq_err'] = lse_bound(l, err, skip)
    if per_dim:
        M, Z = np.asarray(z).shape
        N = np.asarray(loc).shape[0]
        lq, le = np.empty((M, Z)), np.empty((M, Z))
        for a, b in _chunks(M, N, Z):
            ld, ed = dim_terms(z[a:b], loc, scale)
            lq[a:b], le[a:b] = lse_bound(ld, ed, None if skip is None else np.asarray(skip)[a:b])
        out['logq_dim'], out['logq_dim_err'] = lq, le
    return out


def brute_logq(z, loc, scale, skip=None):
    """The definitions as a double loop over (point, row), no vectorised shortcut: (logq [M], logq_dim [M, Z])."""
    z, loc, scale = _f64(z, loc, scale)
    M, Z = z.shape
    N = loc.shape[0]
    lq, lqd = np.empty(M), np.empty((M, Z))
    for i in range(M):
        joint, dims = [], [[] for _ in range(Z)]
        for j in range(N):
            if skip is not None and skip[i] == j:
                continue
            tot = 0.0
            for d in range(Z):
                v = -0.5 * ((z[i, d] - loc[j, d]) / scale[j, d]) ** 2 - math.log(scale[j, d]) - 0.5 * math.log(2 * math.pi)
                dims[d].append(v)
                tot += v
            joint.append(tot)
        n = len(joint)

        def lse(v):
            m = max(v)
            return m + math.log(sum(math.exp(x - m) for x in v)) - math.log(n)
        lq[i] = lse(joint)
        lqd[i] = [lse(dims[d]) for d in range(Z)]
    return lq, lqd


def decompose(z, src, loc, scale, lq, lqd):
    """svae_aggpost_decompose restated -> f64 [4 + Z] = {mi, marginal_kl, tc, kl_mc, dim_kl[Z]} from the f32 points and
    rows and the given logq [M], logq_dim [M, Z]."""
    z, loc, scale, lq, lqd = _f64(z, loc, scale, lq, lqd)
    src = np.asarray(src, np.int64)
    M, Z = z.shape
    t = (z - loc[src]) / scale[src]
    cond = (-0.5 * t * t - np.log(scale[src]) - HALF_LOG_2PI).sum(axis=1)
    lpd = -0.5 * z * z - HALF_LOG_2PI
    out = np.empty(4 + Z)
    out[0] = (cond - lq).sum() / M
    out[1] = (lq - lpd.sum(axis=1)).sum() / M
    out[2] = (lq - lqd.sum(axis=1)).sum() / M
    out[3] = out[0] + out[1]
    out[4:] = (lqd - lpd).sum(axis=0) / M
    return out


def dec_bound(z, src, loc, scale, lq, lqd):
    """|device - decompose(...)| per output: f64 sums of M (Z + 1) terms in two different orders, 2^-52 per add on the
    sum of the terms' magnitudes (a first-order bound with every add counted against the whole)."""
    z, loc, scale, lq, lqd = _f64(z, loc, scale, lq, lqd)
    src = np.asarray(src, np.int64)
    M, Z = z.shape
    t = (z - loc[src]) / scale[src]
    cond = (0.5 * t * t + np.abs(np.log(scale[src])) + HALF_LOG_2PI).sum(axis=1)
    lp = (0.5 * z * z + HALF_LOG_2PI).sum(axis=1)
    adds = (M + 8) * (Z + 4) * 2.0 ** -52
    out = np.empty(4 + Z)
    out[0] = adds * (cond + np.abs(lq)).sum() / M
    out[1] = adds * (lp + np.abs(lq)).sum() / M
    out[2] = adds * (np.abs(lq) + np.abs(lqd).sum(axis=1)).sum() / M
    out[3] = out[0] + out[1]
    out[4:] = adds * (np.abs(lqd) + 0.5 * z * z + HALF_LOG_2PI).sum(axis=0) / M
    return out + 1e-300


def draw(loc, scale, eps):
    """z = fmaf(scale, eps, loc) as svae_latent_draw forms it: the f64 value (the product of two f32 is exact in f64)
    rounded to f32."""
    loc, scale, eps = _f64(loc, scale, eps)
    return (loc + scale * eps).astype(np.float32)


def surgery(loc, scale, rows, z, leave_one_out=False):
    """LatentIndex.elbo_surgery restated for the draws z f32 [M, Z] of the rows `rows` -> dict(out f64 [4 + Z],
    kl_analytic, mi_cap, logq, logq_dim and their bounds)."""
    rows = np.asarray(rows, np.int64)
    N = len(loc)
    r = logq(z, loc, scale, skip=rows.astype(np.int32) if leave_one_out else None, per_dim=True)
    l64, s64 = _f64(loc, scale)
    kl = (0.5 * (l64[rows] ** 2 + s64[rows] ** 2 - 1.0) - np.log(s64[rows])).sum(axis=1).mean()
    r.update(out=decompose(z, rows, loc, scale, r['logq'], r['logq_dim']), kl_analytic=float(kl),
             mi_cap=math.log(N - 1 if leave_one_out else N))
    return r


# ---- cases ---------------------------------------------------------------------------------------------------------
def _frozen(*a):
    for x in a:
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def case(M, N, Z, kind='vae', seed=0):
    """-> (z f32 [M, Z], src int32 [M], loc f32 [N, Z], scale f32 [N, Z]), read-only. Point i is a draw from row
    src_i = i mod N.
    'vae':       means ~ N(0, 1), half the dimensions informative (scale 0.05..0.5) and half collapsed (scale ~ 1).
    'separated': loc_j0 = 64 j, all else 0, scale 1, |eps| <= 4: every foreign term is below exp(-1800) of the own.
    'extreme':   scales log-uniform over 1e-4..1e2 in one index."""
    rng = np.random.default_rng([M, N, Z, seed])
    eps = np.clip(rng.standard_normal((M, Z)), -4, 4)
    src = (np.arange(M) % N).astype(np.int32)
    if kind == 'vae':
        loc = rng.standard_normal((N, Z))
        scale = np.where(np.arange(Z)[None] % 2 == 0, rng.uniform(0.05, 0.5, (N, Z)), rng.uniform(0.9, 1.1, (N, Z)))
        loc[:, 1::2] *= 0.05
    elif kind == 'separated':
        loc = np.zeros((N, Z))
        loc[:, 0] = 64.0 * np.arange(N)
        scale = np.ones((N, Z))
    elif kind == 'extreme':
        loc = rng.standard_normal((N, Z))
        scale = 10.0 ** rng.uniform(-4, 2, (N, Z))
    else:
        raise ValueError(kind)
    loc, scale = loc.astype(np.float32), scale.astype(np.float32)
    z = draw(loc[src], scale[src], eps.astype(np.float32))
    return _frozen(z, src, loc, scale)
