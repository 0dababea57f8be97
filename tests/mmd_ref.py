"""A numpy float64 restatement of the reference's three MMD estimators (math_utils.py:104-184) and of the raw sums the
MMD kernels compute (csrc/mmd.hip), for the tests. Inputs are taken as they are (f32 arrays are widened exactly);
squared distances are sums of squared differences, dimension by dimension; above 2^25 element operations (GPU test
sizes only) a centred f64 product form stands in, see sqdist."""
import math

import numpy as np

EPS24 = 2.0 ** -24
IMQ_BASE = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)


DIRECT_LIMIT = 2 ** 25      # N * M * Z up to which sqdist takes the differences dimension by dimension


def sqdist_direct(x, y):
    """[N, M] squared distances by direct differences (exact differences of f32 values, squares rounded in f64)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d2 = np.zeros((x.shape[0], y.shape[0]))
    for z in range(x.shape[1]):
        d = x[:, z, None] - y[None, :, z]
        d2 += d * d
    return d2


def sqdist_centred(x, y):
    """The same through one f64 matrix product, for the sizes where N * M * Z passes of numpy cost many seconds: both
    sets are centred on y's column means first (distances are translation invariant; the subtraction rounds at
    2^-53 |x|), then |x|^2 + |y|^2 - 2 x.y. After centring the three terms are of the size of d2 itself, so the error
    is a few 2^-53 (|x_c|^2 + |y_c|^2): about 1e-15 of d2 for rows that are not near-duplicates, eight orders below
    the 2^-24 the tests count in (test_mmd_ref.py holds the two forms to 1e-12 on rows at +30)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    c = y.mean(0)
    xc, yc = x - c, y - c
    d2 = (xc * xc).sum(-1)[:, None] + (yc * yc).sum(-1)[None, :] - 2.0 * (xc @ yc.T)
    return np.maximum(d2, 0.0)


def sqdist(x, y):
    """[N, M] squared distances in f64: direct differences up to DIRECT_LIMIT element operations (every golden case),
    the centred product form above it."""
    n, z = np.shape(x)
    return sqdist_direct(x, y) if n * np.shape(y)[0] * z <= DIRECT_LIMIT else sqdist_centred(x, y)


def pair_terms(x, y, kind, params, col_off=None):
    """(v, terms): v [N, M] = d2 + col_off, terms [P, N, M] = k_p(v), and the mask of the pairs that count (i < j when
    y is None)."""
    tri = y is None
    v = sqdist(x, x if tri else y)
    if col_off is not None:
        v = v + np.asarray(col_off, np.float64)[None, :]
    prm = np.asarray(params, np.float64)[:, None, None]
    terms = np.exp(-prm * v[None]) if kind == 'rbf' else prm / (prm + v[None])
    mask = np.triu(np.ones(v.shape, bool), 1) if tri else np.ones(v.shape, bool)
    return v, terms, mask


def pairsum64(x, y=None, kind='rbf', params=(1.0,), col_off=None, z_roundings=None, extra=(0.0, 0.0), off_roundings=0,
              d2=None):
    """sums [P] of svae_pairsum in f64. With z_roundings (the roundings of 2^-24 d2 in the device's d2) also the
    device's error bound [P]: the sum over the pairs of term * (z_roundings * sens + extra[0] * arg + extra[1]) * 2^-24.
    sens = |d log term / d log d2| with d2 the true squared distance: a d2 (RBF), d2 / (s + v) (IMQ), v = d2 + offset.
    arg = the same sensitivity with respect to v: a |v| (RBF), |v| / (s + v) (IMQ): extra[0] counts the roundings that
    are relative to v or to the exponent. extra[1] counts the roundings relative to the term itself. off_roundings
    counts roundings relative to the column offset itself (an offset that was rounded to f32 before the call)."""
    tri = y is None
    if d2 is None:                                                   # d2: sqdist(x, y) computed once by the caller
        d2 = sqdist(x, x if tri else y)
    v = d2 if col_off is None else d2 + np.asarray(col_off, np.float64)[None, :]
    mask = np.triu(np.ones(v.shape, bool), 1) if tri else np.ones(v.shape, bool)
    sums, bound = [], []
    for prm in np.asarray(params, np.float64):                       # one scale at a time: [N, M] temporaries only
        if kind == 'rbf':
            term, sens, arg = np.exp(-prm * v), prm * d2, prm * np.abs(v)
        else:
            term, sens, arg = prm / (prm + v), d2 / (prm + v), np.abs(v) / (prm + v)
        if off_roundings:
            arg = arg + (off_roundings / max(extra[0], 1e-300)) * np.abs(v - d2) * (prm if kind == 'rbf' else 1 / (prm + v))
        sums.append((term * mask).sum())
        if z_roundings is not None:
            bound.append((np.abs(term) * (z_roundings * sens + extra[0] * arg + extra[1]) * mask).sum() * EPS24)
    return np.array(sums) if z_roundings is None else (np.array(sums), np.array(bound))


def rowterm64(x, w, m=None):
    """(sum_i exp(-q_i / 2), q [N]) with q_i = sum_j (x_ij - m_j)^2 w_j."""
    x = np.asarray(x, np.float64)
    d = x if m is None else x - np.asarray(m, np.float64)[None]
    q = (d * d * np.asarray(w, np.float64)[None]).sum(-1)
    return np.exp(-0.5 * q).sum(), q


def rowterm_bound(q, Z, w_roundings=0):
    """The device's error bound on sum_i exp(-q_i / 2), in the arithmetic csrc/mmd.hip documents. q_i carries, relative
    to itself (all its terms are non-negative): 2 roundings from d = x - m squared, 1 from d * d, w_roundings if the
    weights were rounded to f32 before the call, and one per addition of its chain: a lane adds 4 * ceil(Z / 64)
    terms, then 4 butterfly steps. The exponent t = q / 2 carries 2 more (fl(-0.5 log2 e) and the product). The
    exponential is accurate to 1 ulp = 2 roundings, relative to the term; every later addition is in f64 (less than
    one rounding of 2^-24 in all)."""
    q = np.asarray(q, np.float64)
    q_units = 3 + w_roundings + 4 * -(-Z // 64) + 4
    return (np.exp(-0.5 * q) * ((q_units + 2) * 0.5 * q + 2 + 1)).sum() * EPS24


def colstats64(loc, scale):
    loc, scale = np.asarray(loc, np.float64), np.asarray(scale, np.float64)
    var = scale * scale
    kl = 0.5 * (loc * loc + var - 1.0 - np.log(var))
    with np.errstate(invalid='ignore', divide='ignore'):
        v = loc.var(0, ddof=1) if len(loc) > 1 else np.full(loc.shape[1], np.nan)
    return loc.mean(0), v, kl.mean(0)


# ---- the estimators ---------------------------------------------------------------------------------------------------
def analytic_algebra(n, d):
    kv = 0.125 * d
    normalizer = (kv / (1 + kv)) ** (d / 2)
    first = (kv / (2 + kv)) ** (d / 2)
    ugly = 2 * (kv ** 2 / ((1 + kv) * (3 + kv))) ** (d / 2)
    variance = (2 / (n * (n - 1))) * (first ** 2 + (kv / (4 + kv)) ** (d / 2) - ugly)
    return normalizer, first, variance


def custom_algebra(n, var):
    var = np.asarray(var, np.float64)
    d = len(var)
    kv = 0.125 * d
    klv = math.log(kv)
    ld = [0.5 * np.log(c * var + kv).sum() for c in (1, 2, 3, 4)]
    normalizer = math.exp(klv * d / 2 - ld[0])
    first = math.exp(klv * d / 2 - ld[1])
    ugly = math.exp(math.log(2) + klv * d - ld[0] - ld[2])
    variance = 2 / (n * (n - 1)) * (first ** 2 + math.exp(klv * d / 2 - ld[3]) - ugly)
    return normalizer, first, variance


def analytic_rbf(x, standardize=True):
    n, d = x.shape
    kv = 0.125 * d
    normalizer, first, variance = analytic_algebra(n, d)
    second = rowterm64(x, np.full(d, 1.0 / (1.0 + kv)))[0] / n
    third = pairsum64(x, None, 'rbf', [0.5 / kv])[0] / (n * (n - 1) / 2)
    mmd = first - 2 * normalizer * second + third
    return mmd / variance ** 0.5 if standardize else mmd


def custom_rbf(x, mean, var, standardize=True):
    n, d = x.shape
    kv = 0.125 * d
    mean = np.broadcast_to(np.asarray(mean, np.float64), (d,))
    var = np.broadcast_to(np.asarray(var, np.float64), (d,))
    normalizer, first, variance = custom_algebra(n, var)
    second = rowterm64(x, 1.0 / (kv + var), mean)[0] / n
    third = pairsum64(x, None, 'rbf', [0.5 / kv])[0] / (n * (n - 1) / 2)
    mmd = first - 2 * normalizer * second + third
    return mmd / variance ** 0.5 if standardize else mmd


def imq_scales(d):
    """The f32 values of the reference's scale tensor."""
    return [float(np.float32(b) * np.float32(2 * d)) for b in IMQ_BASE]


def imq_offsets(prior):
    p = np.asarray(prior, np.float64)
    return p.shape[1] - (p * p).sum(-1)


def imq(x, prior, prior_pair=None):
    """gaussian_imq_mmd_sq with the given standardised prior samples: `prior` in the cross term, `prior_pair` (default:
    the same) in the prior-prior term. The reference draws the two sets one after the other: its two helpers reach
    the cached sampler with different argument lists, (d, device) and (d, device, n), so the cache holds two draws."""
    n, d = x.shape
    s = imq_scales(d)
    first = pair_mean(x, None, s)
    middle = 2 * pair_mean(x, prior, s, imq_offsets(prior))
    return first - middle + pair_mean(prior if prior_pair is None else prior_pair, None, s)


def pair_mean(x, y, scales, col_off=None):
    _, terms, mask = pair_terms(x, y, 'imq', scales, col_off)
    return (terms * mask[None]).sum() / (len(scales) * mask.sum())


def imq_min_denominator(x, prior):
    """The smallest s + v over scales and pairs of the three sums of `imq` (the reference divides by it)."""
    s = min(imq_scales(x.shape[1]))
    def offdiag_min(a):
        d2 = sqdist(a, a)
        return d2[np.triu(np.ones(d2.shape, bool), 1)].min()

    lo = s + min(offdiag_min(x), offdiag_min(prior))
    return min(lo, s + (sqdist(x, prior) + imq_offsets(prior)[None]).min())
