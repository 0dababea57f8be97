"""float64 restatements of the decode kernels (csrc/decode.hip: svae_dec_linear, svae_dec_attn, svae_dec_sample) and
the error bounds the GPU tests hold them to. Inputs are the f32 arrays the kernels read, promoted to float64 here;
nothing in this file runs product code."""
import math

import numpy as np
import torch

EPS24 = 2.0 ** -24


# ---------------------------------------------------------------------------------------------- dec_linear
def quarter_ints(shape, seed):
    """Seeded f32 array of k / 4, k integer in [-3, 3]. Products are multiples of 1/16 with |.| <= 9/16, so every
    partial sum of up to 2^24 * 16 / 9 of them is exact in f32: any summation order gives the float64 result."""
    rng = np.random.default_rng(seed)
    return (rng.integers(-3, 4, size=shape) / 4.0).astype(np.float32)


def split_count(M, N, K, part_elems):
    """svae_dec_linear's split-K selection (decode.hip): K is split over workgroups, doubling the count, until
    ~512 workgroups are in flight, while every slice keeps >= 256 K-elements and a workspace of splits * M * N
    floats was given; 16 at the most."""
    cols, mblk = (N + 15) // 16, (M + 63) // 64
    splits = 1
    while (splits < 16 and cols * mblk * splits * 2 <= 512 and K // (splits * 2) >= 256
           and splits * 2 * M * N <= part_elems):
        splits *= 2
    return splits


def linear64(X, W, bias=None, resid=None):
    """X [M, K] . W [N, K]^T (+ bias) (+ resid), float64."""
    y = np.asarray(X, np.float64) @ np.asarray(W, np.float64).T
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if resid is not None:
        y = y + np.asarray(resid, np.float64)
    return y


def gelu64(x):
    """x Phi(x) = 0.5 x erfc(-x / sqrt 2): erfc keeps the negative tail free of the 1 + erf cancellation."""
    x = torch.as_tensor(np.asarray(x, np.float64))
    return (0.5 * x * torch.erfc(-x / math.sqrt(2.0))).numpy()


def rotary64(pre, rot, pos, rot_cols, rot_d):
    """The rotary epilogue on pre [M, N] (float64 pre-activations) at table row `pos`, from the f32 table values
    rot [positions, rot_d / 2, 2]: columns (2i, 2i + 1) below rot_cols -> (a cos - b sin, b cos + a sin) with the
    factors of pair (n % rot_d) / 2. Returns (y, mag): mag = |a cos| + |b sin| per output, the magnitude the
    bound scales with; both are zero-width (y = pre, mag = 0) from column rot_cols on."""
    pre = np.asarray(pre, np.float64)
    y, mag = pre.copy(), np.zeros_like(pre)
    n = np.arange(0, rot_cols, 2)
    cs = np.asarray(rot, np.float64)[pos, (n % rot_d) // 2]       # [pairs, 2]
    c, s = cs[:, 0], cs[:, 1]
    a, b = pre[:, n], pre[:, n + 1]
    y[:, n], y[:, n + 1] = a * c - b * s, b * c + a * s
    mag[:, n], mag[:, n + 1] = np.abs(a * c) + np.abs(b * s), np.abs(b * c) + np.abs(a * s)
    return y, mag


# ---------------------------------------------------------------------------------------------- dec_attn
def visible_keys(p, window):
    """Key positions a query at position p sees: dense causal 0..p, or with the sliding window the [CLS] block
    {j < 32} and the blocks from (p // 32 - (window - 1)) on, {j >= max(32, (p // 32 - (window - 1)) * 32)},
    up to p (the key set of the reference's windowed KV cache, attention.py:115-140)."""
    j = np.arange(p + 1)
    if window <= 0:
        return j
    lo2 = max(32, (p // 32 - (window - 1)) * 32)
    return j[(j < 32) | (j >= lo2)]


def attn64(q, k, v, scale):
    """One (sequence, head): q [hd], k, v [n, hd] over exactly the visible keys. Returns O [hd], A [hd] =
    sum_j p_j |v_jc|, S = max_j scale sum_c |q_c k_jc| and the spread max(s) - min(s) of the scores."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    s = scale * (k @ q)
    S = float((scale * (np.abs(k) @ np.abs(q))).max())
    e = np.exp(s - s.max())
    pr = e / e.sum()
    return pr @ v, pr @ np.abs(v), S, float(s.max() - s.min())


def attn_bound(A, S, n, hd):
    """|O_c - ref_c| <= 2^-24 (4 (ceil(n / G) + G + 40) + 2 (hd + 2) S) A_c with G = 1024 // hd key groups:
    ceil(n / G) + G additions of the kernel's own accumulation, the score rounding ((hd + 2) S 2^-24 absolute, in
    numerator and denominator) and 40 ulp for the fast exponential at arguments within 16 of the row maximum."""
    G = 1024 // hd
    return EPS24 * (4.0 * (-(-n // G) + G + 40) + 2.0 * (hd + 2) * S) * np.asarray(A, np.float64)


# ---------------------------------------------------------------------------------------------- dec_sample
def _kept(logits, top_k, top_p, temperature):
    """-> (order, probs, cum): vocabulary ids of the candidates in descending order of logit (after top-k), their
    softmax probabilities over the candidates, and the running sum; float64."""
    x = np.asarray(logits, np.float64) / float(temperature)
    order = np.argsort(-x, kind='stable')
    if top_k > 0:
        order = order[:top_k]
    e = np.exp(x[order] - x[order[0]])
    pr = e / e.sum()
    return order, pr, np.cumsum(pr)


def sample_distribution(logits, top_k, top_p, temperature):
    """The distribution GenerationState.process_logits (generation.py:47-68) samples the emitted id from, for one
    f32 logits row and temperature > 0, top_k != 1: -> (ids ascending int64, probabilities float64 summing to 1).

    logits / temperature; top_k > 0 keeps the k largest; top_p < 1 sorts the candidates descending, takes the
    softmax over them and drops every candidate whose cumulative probability exceeds top_p, except the first; the
    rest are sampled in proportion. The emitted id is the vocabulary id, except with top_k > 0 and top_p < 1: the
    reference then emits the sampled candidate's position in topk's output, here its descending rank (what topk
    returns wherever it returns its output sorted)."""
    order, pr, cum = _kept(logits, top_k, top_p, temperature)
    if top_p < 1.0:
        keep = cum <= top_p
        keep[0] = True
    else:
        keep = np.ones(order.size, dtype=bool)
    ids = np.arange(order.size)[keep] if (top_k > 0 and top_p < 1.0) else order[keep]
    p = pr[keep] / pr[keep].sum()
    o = np.argsort(ids)
    return ids[o].astype(np.int64), p[o]


def nucleus_margin(logits, top_k, top_p, temperature):
    """min_i |cum_i - top_p| over the candidates: below ~1e-6 a candidate could fall on either side of the nucleus
    in f32."""
    if top_p >= 1.0:
        return math.inf
    _, _, cum = _kept(logits, top_k, top_p, temperature)
    return float(np.abs(cum - top_p).min())


def chi2_threshold(nu):
    """The 1 - 1e-6 quantile of chi-square with nu degrees of freedom (Wilson-Hilferty, z = 4.753)."""
    return nu * (1.0 - 2.0 / (9.0 * nu) + 4.753 * math.sqrt(2.0 / (9.0 * nu))) ** 3


def chi2_binned(ids, probs, draws, min_expected=20.0):
    """Pearson chi-square of the drawn ids against (ids, probs): the support in ascending id order, neighbours
    merged until every bin expects >= min_expected draws (a short last bin joins the one before it).
    -> (chi2, degrees of freedom = bins - 1). Draws outside the support count as an infinite chi2."""
    draws = np.asarray(draws).ravel()
    n = draws.size
    pos = np.searchsorted(ids, draws)
    pos = np.minimum(pos, ids.size - 1)
    if not np.array_equal(ids[pos], draws):
        return math.inf, 0
    counts = np.bincount(pos, minlength=ids.size).astype(np.float64)
    exp_bins, obs_bins, e, o = [], [], 0.0, 0.0
    for pi, ci in zip(probs * n, counts):
        e += pi
        o += ci
        if e >= min_expected:
            exp_bins.append(e)
            obs_bins.append(o)
            e, o = 0.0, 0.0
    if e > 0.0 or o > 0.0:
        if exp_bins:
            exp_bins[-1] += e
            obs_bins[-1] += o
        else:
            exp_bins.append(e)
            obs_bins.append(o)
    ex, ob = np.asarray(exp_bins), np.asarray(obs_bins)
    return float(((ob - ex) ** 2 / ex).sum()), ex.size - 1
