"""Float64 numpy restatement of the Gaussian-mixture contracts of include/svae.h (svae_gmm_prepare / _estep / _mstep /
_sample) and of sparse_vae.GaussianMixture's EM loop, computed from the same f32 inputs; the case generators of the
mixture tests; and the rounding bounds of the device's f32 arithmetic, derived from the orders stated in the header of
csrc/gmm.hip. No bound here is a hand-picked constant.

Units: u = 2^-24, the largest relative error of one f32 rounding. expf and logf are the device library's, good to 1 ulp
= 2 u. All bounds are first order in u."""
import functools

import numpy as np

EPS24 = 2.0 ** -24
TWO_PI = 6.283185307179586476925

# Geometry the tests check against svae_gmm_geometry.
ROWS_PER_BLOCK, TILE, MAX_K = 256, 16, 256
ZS = (4, 64, 68, 256)

# The safety factor between a row's top-two gap in a_ik and the sum of the two entries' rounding bounds under which
# the GPU tests demand identical labels for EVERY row. 1 of it is the comparison itself (each of the two values moves
# by at most its bound); the bound is first order, and its neglected second-order terms are below
# (Z / 2 + 5) u < 2^-16 of it. The reference and the device see the same f32 parameters (the tests pass the
# reference's), so nothing else enters; the factor 2 leaves the first-order bound a margin of its own size.
GAP_FACTOR = 2.0


def q_roundings(Z):
    """The device's q = sum_d ((x - m)^2 + s2) inv_var in units of u q, counted from the order in the header of
    csrc/gmm.hip: each of the two fmaf chains takes Z / 2 FMAs (one rounding each on a partial sum of non-negative
    terms), a term carries the two roundings of its difference (d = fl(x - m): (1 + e)^2), the rounding of
    e = fmaf(d, d, s2) and the rounding of inv_var = (float)(1 / var), and the chains' sum is one more."""
    return Z // 2 + 5


def derived(weight, mean, var):
    """f64 (inv_var [K, Z], logc [K]) from the f32 model, as svae_gmm_prepare forms them before rounding."""
    w, v = np.asarray(weight, np.float64), np.asarray(var, np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        logc = np.log(w) - 0.5 * np.log(TWO_PI * v).sum(axis=1)
    return 1.0 / v, logc


def a_matrix(x, s2, weight, mean, var):
    """-> (a f64 [N, K], err f64 [N, K]): a_ik = logc_k - q / 2 from direct differences of the f32 inputs, and the
    device's rounding bound ((Z / 2 + 5) q / 2 + |logc| + |a|) u. A component with logc = -inf has a = -inf, err 0."""
    x64, m64 = np.asarray(x, np.float64), np.asarray(mean, np.float64)
    iv, logc = derived(weight, mean, var)
    n, Z = x64.shape
    s = np.zeros_like(x64) if s2 is None else np.asarray(s2, np.float64)
    q = np.empty((n, m64.shape[0]))
    with np.errstate(invalid='ignore', over='ignore'):
        for k in range(m64.shape[0]):
            d = x64 - m64[k]
            q[:, k] = ((d * d + s) * iv[k]).sum(axis=1)
        a = logc[None] - 0.5 * q
        err = (q_roundings(Z) * 0.5 * q + np.abs(logc)[None] + np.abs(a)) * EPS24
    dead = np.isneginf(logc)
    a[:, dead] = -np.inf
    err[:, dead] = 0.0
    return a, err


def winners(a):
    """Per row of a [N, K]: the largest entry's index; ties to the lower index; NaN loses to every number (-inf
    included); an all-NaN row gets 0."""
    nan = np.isnan(a)
    lab = np.argmax(np.where(nan, -np.inf, a), axis=1)
    rows = np.arange(a.shape[0])
    fix = nan[rows, lab] & ~nan.all(axis=1)        # only -inf numbers in the row, and a NaN before the first of them
    lab[fix] = np.argmax(~nan[fix], axis=1)
    lab[nan.all(axis=1)] = 0
    return lab.astype(np.int32)


def logsumexp(a):
    """Row-wise; -inf entries contribute exactly 0; a NaN entry makes the row NaN; an all -inf row gives -inf."""
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        m = np.max(np.where(np.isnan(a), -np.inf, a), axis=1)
        ms = np.where(np.isfinite(m), m, 0.0)
        out = ms + np.log(np.exp(a - ms[:, None]).sum(axis=1))
    out[np.isnan(a).any(axis=1)] = np.nan
    return out


def lse_bound(a, err, lse):
    """|device lse_i - lse_i|. d lse / d a_k = r_k, so the entries' errors enter as sum_k r_k err_ik. The online sum S
    (header of csrc/gmm.hip) takes one step per live component, and a step costs, relative to the S it produces: one
    expf (2 u), the rounding of its argument t (u |t| on a share of S that is at most min(1, K e^-|t|), so at most
    max(1, ln K) u), and one fmaf or add (u); an old S that is rescaled carries its error along with factor <= 1. That
    is K (3 + max(1, ln K)) u on log S; logf adds 2 u |log S| <= 2 u ln K and the last add u |lse|."""
    K = a.shape[1]
    with np.errstate(invalid='ignore'):
        r = np.exp(a - lse[:, None])
        lnk = np.log(max(K, 1))
        return (np.nan_to_num(r * err).sum(axis=1) + (K * (3 + max(1.0, lnk)) + 2 * lnk) * EPS24
                + np.abs(lse) * EPS24)


def resp_bound(a, err, lse, lse_err):
    """|device r_ik - r_ik| for r = expf(a - lse): the argument is off by err_ik + lse_err_i + u |a - lse| (its own
    rounding), expf adds 2 u, all relative to r; plus 2^-149 where r is subnormal or underflows: there expf's 1 ulp is
    one step of the subnormal grid, not 2 u r."""
    with np.errstate(invalid='ignore', over='ignore'):
        t = a - lse[:, None]
        r = np.exp(t)
        return np.nan_to_num(r * (err + lse_err[:, None] + (np.abs(t) + 2) * EPS24)) + 2.0 ** -149


def estep(x, s2, weight, mean, var, mutate=None):
    """-> dict(a, err, lse, lse_err, label, resp, resp_err, bound). mutate(a, err) -> a, if given, stands in for the
    device's rounding."""
    a, err = a_matrix(x, s2, weight, mean, var)
    if mutate is not None:
        a = mutate(a, err)
    lse = logsumexp(a)
    lse_err = lse_bound(a, err, lse)
    with np.errstate(invalid='ignore'):
        resp = np.exp(a - lse[:, None])
    return dict(a=a, err=err, lse=lse, lse_err=lse_err, label=winners(a), resp=resp,
                resp_err=resp_bound(a, err, lse, lse_err), bound=float(lse.sum()))


def top_two_gap(a, err):
    """Per row: (largest - second largest a_ik) / (the sum of the two entries' bounds); inf at K = 1."""
    if a.shape[1] < 2:
        return np.full(a.shape[0], np.inf)
    order = np.argsort(-a, axis=1, kind='stable')[:, :2]
    rows = np.arange(a.shape[0])
    gap = a[rows, order[:, 0]] - a[rows, order[:, 1]]
    return gap / (err[rows, order[:, 0]] + err[rows, order[:, 1]])


def mstep(x, s2, weight, mean, var, reg_covar, lse=None, label=None, a=None, round32=True):
    """One M-step by the documented f64 finalisation -> dict(weight, mean, var (f32), nk (f64), and for the soft form
    the derived bounds nk_err, mean_err, var_err, weight_err against the device's result).
    soft: r = exp(a - lse) with lse given (the device's own) and a from a_matrix (or passed). hard: r = [label == k]."""
    x64, m64 = np.asarray(x, np.float64), np.asarray(mean, np.float64)
    n, Z = x64.shape
    K = m64.shape[0]
    s = np.zeros_like(x64) if s2 is None else np.asarray(s2, np.float64)
    reg = float(np.float32(reg_covar))
    rho = None
    if label is not None:
        label = np.asarray(label)
        r = (label[:, None] == np.arange(K)[None]).astype(np.float64)
    else:
        if a is None:
            a, err = a_matrix(x, s2, weight, mean, var)
        else:
            a, err = a
        lse = np.asarray(lse, np.float64)
        t = a - lse[:, None]
        r = np.exp(t)
        rho = r * (err + (np.abs(t) + 2) * EPS24) + 2.0 ** -149       # |device r - r|: the same lse on both sides
    nk = r.sum(axis=0)
    f = np.float32 if round32 else np.float64
    new_w = np.zeros(K, f)
    new_m = np.array(mean, f, copy=True)
    new_v = np.array(var, f, copy=True)
    total = nk[nk > 0].sum()
    nk_err = None if rho is None else rho.sum(axis=0)
    mean_err, var_err, weight_err = np.zeros((K, Z)), np.zeros((K, Z)), np.zeros(K)
    for k in range(K):
        if not nk[k] > 0:
            continue
        d = (x64.astype(f) - np.asarray(mean, f)[k]).astype(np.float64)   # the device's f32 difference
        s1 = (r[:, k, None] * d).sum(axis=0)
        sq = (r[:, k, None] * (d * d + s)).sum(axis=0)
        m1, m2 = s1 / nk[k], sq / nk[k]
        m_new = m64[k] + m1
        v_new = m2 - m1 * m1 + reg
        new_m[k], new_v[k] = m_new.astype(f), v_new.astype(f)
        new_w[k] = f(nk[k] / total)
        if rho is not None:
            # d itself carries one rounding (u |d|): r |d| u on S1, 2 r d^2 u on S2
            s1_err = ((rho[:, k, None] + r[:, k, None] * EPS24) * np.abs(d)).sum(axis=0)
            sq_err = ((rho[:, k, None] + 2 * r[:, k, None] * EPS24) * d * d + rho[:, k, None] * s).sum(axis=0)
            m1_err = (s1_err + np.abs(m1) * nk_err[k]) / nk[k]
            mean_err[k] = m1_err + np.abs(m_new) * EPS24
            var_err[k] = (sq_err + m2 * nk_err[k]) / nk[k] + 2 * np.abs(m1) * m1_err + np.abs(v_new) * EPS24
            weight_err[k] = (nk_err[k] + nk[k] / total * nk_err.sum()) / total + nk[k] / total * EPS24
    out = dict(weight=new_w, mean=new_m, var=new_v, nk=nk)
    if rho is not None:
        out.update(nk_err=nk_err, mean_err=mean_err, var_err=var_err, weight_err=weight_err)
    return out


def sample(weight, mean, var, u, eps):
    """-> (comp int32 [n], z f64 [n, Z], exact: the f32 product-sum is exact where True). The device's sd is
    (float)sqrt((double)var)."""
    w = np.asarray(weight, np.float64)
    w = np.where(w > 0, w, 0.0)
    cum = np.cumsum(w)
    last = int(np.flatnonzero(w > 0)[-1]) if (w > 0).any() else 0
    target = np.asarray(u, np.float32).astype(np.float64) * cum[-1]
    comp = np.minimum(np.searchsorted(cum, target, side='right'), last).astype(np.int32)   # first cum > target
    sd = np.sqrt(np.asarray(var, np.float64)).astype(np.float32).astype(np.float64)
    z = sd[comp] * np.asarray(eps, np.float64) + np.asarray(mean, np.float64)[comp]
    return comp, z, z.astype(np.float32).astype(np.float64) == z


def fit(x, s2, weight, mean, var, reg_covar, n_iter, mutate=None, round32=True):
    """sparse_vae.GaussianMixture's loop from the given parameters for n_iter iterations (E-step, M-step, parameters
    rounded to f32 as the device stores them) -> dict(weight, mean, var, nk, bounds (per row: B_0 .. B_{n_iter-1}),
    lse_err (per iteration: the mean derived bound on lse), gaps (per iteration: the smallest top_two_gap), hist (the
    parameters each E-step saw)). round32 False keeps the parameters in f64: EM proper, whose bound never falls."""
    w, m, v = (np.array(t, np.float32 if round32 else np.float64, copy=True) for t in (weight, mean, var))
    bounds, lse_errs, gaps, hist = [], [], [], []
    nk = None
    for it in range(n_iter):
        hist.append((w, m, v))
        a, err = a_matrix(x, s2, w, m, v)
        gaps.append(float(top_two_gap(a, err).min()))
        if mutate is not None:
            a = mutate(a, err)
        lse = logsumexp(a)
        bounds.append(float(lse.mean()))
        lse_errs.append(float(lse_bound(a, err, lse).mean()))
        out = mstep(x, s2, w, m, v, reg_covar, lse=lse, a=(a, err), round32=round32)
        w, m, v, nk = out['weight'], out['mean'], out['var'], out['nk']
    return dict(weight=w, mean=m, var=v, nk=nk, bounds=bounds, lse_err=lse_errs, gaps=gaps, hist=hist)


def stop_iteration(bounds, tol):
    """GaussianMixture's rule on the per-row bounds B_0, B_1, ...: the first t >= 2 with |B_{t-1} - B_{t-2}| < tol,
    or None."""
    for t in range(2, len(bounds) + 1):
        if abs(bounds[t - 1] - bounds[t - 2]) < tol:
            return t
    return None


def sign_mutation(seed):
    """A mutate hook: every a_ik moved by its full bound with a seeded random sign."""
    def mutate(a, err):
        rng = np.random.default_rng(seed)
        return a + np.where(rng.integers(0, 2, a.shape) > 0, 1.0, -1.0) * err
    return mutate


@functools.lru_cache(maxsize=None)
def fit_spread(case, n_iter, n_mut=4):
    """The float64 reference's own sensitivity on a blob case: the largest deviation of (weight, mean, var) after
    n_iter iterations over n_mut runs whose a_ik are perturbed by the derived per-entry bound with random signs."""
    x, s2, w0, m0, v0 = blob_case(*case)
    base = fit(x, s2, w0, m0, v0, REG, n_iter)
    spread = {k: 0.0 for k in ('weight', 'mean', 'var')}
    for j in range(n_mut):
        mut = fit(x, s2, w0, m0, v0, REG, n_iter, mutate=sign_mutation(977 + j))
        for k in spread:
            spread[k] = max(spread[k], float(np.abs(mut[k].astype(np.float64) - base[k].astype(np.float64)).max()))
    return base, spread


# ---- cases ------------------------------------------------------------------------------------------------------------
REG = 1e-6


def exact_shapes():
    """(N, K, Z, has_s2): N in {65, R + 1, 2R + 1} and one N with several M-step row groups, K in {1, 2, T, T + 1,
    2T + 1, MAX_K}, every Z, with and without s2; not the full product, but every N with a small and a ragged K and
    every K at 2R + 1 rows. 5000 rows at MAX_K give M-step row groups of 128 rows: a wave then carries its f64
    accumulators across two batches of 64 (every smaller case has groups of 64)."""
    R, T = ROWS_PER_BLOCK, TILE
    out = []
    for Z in ZS:
        for n, K in ((65, 2), (65, T), (R + 1, 1), (R + 1, T + 1), (2 * R + 1, 1), (2 * R + 1, 2), (2 * R + 1, T),
                     (2 * R + 1, T + 1), (2 * R + 1, 2 * T + 1), (2 * R + 1, MAX_K), (1000, MAX_K), (5000, MAX_K)):
            for has_s2 in (False, True):
                out.append((n, K, Z, has_s2))
    return out


@functools.lru_cache(maxsize=None)
def exact_case(n, K, Z, has_s2, salt=0):
    """Integer coordinates in [-7, 7], integer variances in [0, 3], integer means on entry and hard labels: every
    d = x - m, every d^2 + s2 and every f64 partial sum is an integer far below 2^53, so the sufficient statistics are
    exact in any order and the device must EQUAL the documented finalisation. Some labels lie outside 0..K-1 (ignored),
    component K - 1 gets no row at K >= 3 (it keeps its parameters and gets weight 0)."""
    rng = np.random.default_rng(7000003 * n + 1013 * K + Z + 7919 * salt + int(has_s2))
    x = rng.integers(-7, 8, (n, Z)).astype(np.float32)
    s2 = rng.integers(0, 4, (n, Z)).astype(np.float32) if has_s2 else None
    mean = rng.integers(-7, 8, (K, Z)).astype(np.float32)
    var = rng.integers(1, 5, (K, Z)).astype(np.float32)
    weight = np.full(K, 1.0 / K, np.float32)
    label = rng.integers(0, max(1, K - 1) if K >= 3 else K, n).astype(np.int32)
    label[::17] = -1
    label[5::29] = K
    label[7::31] = 1 << 20
    for t in (x, mean, var, weight, label) + ((s2,) if has_s2 else ()):
        t.setflags(write=False)
    return x, s2, weight, mean, var, label


# (K, Z, has_s2); N = 2R + 1. K = T + 1 crosses a component tile; Z = 68 is no multiple of 64.
BLOBS = ((3, 64, True), (3, 64, False), (TILE + 1, 68, True), (TILE + 1, 68, False))
BLOB_ITERS = 6
SEP = 2.5


@functools.lru_cache(maxsize=None)
def blob_case(K, Z, has_s2, seed_=0):
    """Overlapping blobs: K centres N(0, SEP^2 / 2Z) per coordinate, so two centres are about SEP = 2.5 apart with
    unit variance along the line between them: neighbours share mass, and EM moves for many iterations instead of
    converging in one. With s2 the rows are posteriors of variance 0.1 .. 0.4 around means of spread
    sqrt(1 - s2). The start: the centres moved by N(0, 0.5^2), unit variances, equal weights.
    -> (x, s2 or None, weight0, mean0, var0), read-only f32."""
    n = 2 * ROWS_PER_BLOCK + 1
    rng = np.random.default_rng(515151 + 131 * K + Z + 17 * seed_ + int(has_s2))
    centres = SEP / np.sqrt(2.0 * Z) * rng.standard_normal((K, Z))
    which = rng.integers(0, K, n)
    which[:K] = np.arange(K)
    if has_s2:
        s2 = rng.uniform(0.1, 0.4, (n, Z))
        x = centres[which] + np.sqrt(1.0 - s2) * rng.standard_normal((n, Z))
        s2 = s2.astype(np.float32)
    else:
        s2 = None
        x = centres[which] + rng.standard_normal((n, Z))
    x = x.astype(np.float32)
    mean0 = (centres + 0.5 * rng.standard_normal((K, Z))).astype(np.float32)
    var0 = np.ones((K, Z), np.float32)
    weight0 = np.full(K, 1.0 / K, np.float32)
    for t in (x, mean0, var0, weight0) + ((s2,) if has_s2 else ()):
        t.setflags(write=False)
    return x, s2, weight0, mean0, var0


@functools.lru_cache(maxsize=None)
def blob_fit(K, Z, has_s2):
    x, s2, w0, m0, v0 = blob_case(K, Z, has_s2)
    return fit(x, s2, w0, m0, v0, REG, BLOB_ITERS)


@functools.lru_cache(maxsize=None)
def collapsed_case(n=600, Z=64, active=16, seed_=0):
    """The prototype of the design point: Z = 64 latent dimensions of which 16 are active (two clusters of means,
    posterior variance 0.05) and 48 are collapsed (means jittered by 0.02 around 0, posterior variance about 0.98).
    -> (mu f32 [n, Z], s2 f32 [n, Z])."""
    rng = np.random.default_rng(90210 + seed_)
    mu = 0.02 * rng.standard_normal((n, Z))
    s2 = 0.98 + 0.005 * rng.standard_normal((n, Z))
    side = rng.integers(0, 2, n)
    mu[:, :active] = np.where(side[:, None] > 0, 1.5, -1.5) + 0.3 * rng.standard_normal((n, active))
    s2[:, :active] = 0.05
    return mu.astype(np.float32), s2.astype(np.float32)


def two_component_rows(n, Z, seed_=0):
    """Rows drawn from a known two-component mixture far from N(0, I): weights 0.3 / 0.7, means -2 and +1.5 in every
    coordinate, standard deviations 0.5 and 0.7. -> f32 [n, Z] points."""
    rng = np.random.default_rng(31337 + seed_)
    c = rng.uniform(size=n) < 0.3
    z = np.where(c[:, None], -2.0 + 0.5 * rng.standard_normal((n, Z)), 1.5 + 0.7 * rng.standard_normal((n, Z)))
    return z.astype(np.float32)
