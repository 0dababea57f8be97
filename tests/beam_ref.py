"""Float64 numpy restatement of beam search decoding (include/svae.h "beam search decoding";
csrc/beam.hip) and the error bounds the GPU tests hold the kernels to. Nothing here runs product code.

Semantics, per document, W beams, T-wide id rows (index 0 = start token, at most T - 2 generated tokens, indices
1 .. T-2). State: W live hypotheses with cumulative log-probability cum (0 for beam 0 and -inf for the others at the
start), a pool of at most W finished hypotheses. Step c (the index of the generated token, so also the generated
length): candidates cum[w] + logp[w][v]; the best 2W by (score descending, beam ascending, token ascending) are
walked in that order: an end token of rank < W enters the pool with score s / c^alpha (a free slot, else it replaces
the worst entry -- lowest score, the later slot among equals -- if strictly better), an end token of rank >= W is
dropped, any other candidate becomes the next live hypothesis until W are live. The document is done when the pool
holds W entries and (best live cum) / Lb^alpha <= the worst pool score, Lb = T - 2 if alpha > 0 else c. After the
last step the live hypotheses of documents not done enter the pool with length T - 2 under the same rule; the pool is
sorted by score descending (stable in slot order).

The divisor l^alpha is the f32 table the product computes once in float64 (len_pen_table): the kernels and this file
divide by the same numbers. `dtype` is the arithmetic of the scores: float64 for the reference, float32 to restate
the kernels' own divisions bit for bit where a test's inputs make every other operation exact.
"""
import collections
import math

import numpy as np

import decode_ref as R

EPS24 = R.EPS24
NEG_INF = -math.inf


def len_pen_table(T, alpha):
    """f32 [T]: l ** alpha for l >= 1 (entry 0 = 1), computed in float64 and rounded once."""
    return (np.maximum(np.arange(T), 1).astype(np.float64) ** float(alpha)).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the pool and the walk
def pool_insert(scores, W, score):
    """Slot an arrival takes, or -1: a free slot while there is one, else the worst entry's (lowest score, the later
    slot among equals) if the arrival is strictly better."""
    if len(scores) < W:
        return len(scores)
    worst = 0
    for i in range(1, W):
        if scores[i] <= scores[worst]:
            worst = i
    return worst if score > scores[worst] else -1


class Doc:
    """One document's state."""

    def __init__(self, W, T, start, dtype=np.float64):
        self.W, self.T, self.dtype = W, T, dtype
        self.cum = np.full(W, NEG_INF, dtype)
        self.cum[0] = 0.0
        self.err = np.zeros(W)                      # accumulated error bound of each live cum (the caller's)
        self.ids = np.zeros((W, T), np.int64)
        self.ids[:, 0] = start
        self.anc = np.zeros((W, T), np.int32)       # (uint8 in the product, W <= 16; the exhaustive test has more)
        self.pool_score, self.pool_logp, self.pool_len, self.pool_ids, self.pool_pen = [], [], [], [], []
        self.done = False
        self.min_margin = math.inf                  # smallest gap any decision of this document rested on
        self.history = []                           # per step: list of (parent, token, score) of the new rows
        self.events = collections.Counter()         # which rules fired: end_in, end_drop, replace, reject, tie

    def _worst(self):
        """(score, divisor) of the entry pool_insert would replace."""
        i = max(range(len(self.pool_score)), key=lambda k: (-self.pool_score[k], k))
        return self.pool_score[i], self.pool_pen[i]

    @staticmethod
    def _gap(a, pen_a, b, pen_b):
        """The gap between two normalised scores in units of the un-normalised sums: a = s_a / pen_a carries
        err / pen_a, so |a - b| is compared with the accumulated bound after scaling by the smaller divisor."""
        return abs(float(a) - float(b)) * float(min(pen_a, pen_b))

    def _put(self, score, logp, length, row, pen):
        slot = pool_insert(self.pool_score, self.W, score)
        if len(self.pool_score) == self.W:          # a comparison was made: it is a decision
            self.min_margin = min(self.min_margin, self._gap(score, pen, *self._worst()))
            self.events['replace' if slot >= 0 else 'reject'] += 1
        if slot < 0:
            return
        if slot == len(self.pool_score):
            for lst in (self.pool_score, self.pool_logp, self.pool_len, self.pool_ids, self.pool_pen):
                lst.append(None)
        self.pool_score[slot], self.pool_logp[slot], self.pool_len[slot] = score, logp, length
        self.pool_ids[slot], self.pool_pen[slot] = row, pen

    def select(self, cands, c, end, len_pen, alpha):
        """One step at index c. cands: (score, beam, token[, err]) of every candidate that counts, any order; at
        least the best 2W + 1 of them where the margins are wanted. Nothing happens to a done document."""
        if self.done:
            return
        W, T, dt = self.W, self.T, self.dtype
        cands = [t if len(t) == 4 else (*t, 0.0) for t in cands if t[0] > NEG_INF]
        cands.sort(key=lambda t: (-t[0], t[1], t[2]))
        cum, err = np.full(W, NEG_INF, dt), np.zeros(W)
        ids, anc = self.ids.copy(), self.anc.copy()
        hist, nl, walked = [], 0, 0
        for rank, (s, w, tok, e) in enumerate(cands[:2 * W]):
            if nl == W:
                break
            walked = rank + 1
            if rank and s == cands[rank - 1][0] and w != cands[rank - 1][1]:
                self.events['tie'] += 1
            if tok == end:
                self.events['end_in' if rank < W else 'end_drop'] += 1
                if rank < W:
                    row = np.zeros(T, np.int64)
                    row[:c], row[c] = self.ids[w, :c], end
                    self._put(dt(s) / dt(len_pen[c]), dt(s), c, row, len_pen[c])
            else:
                cum[nl], err[nl] = s, e
                ids[nl, :c], ids[nl, c] = self.ids[w, :c], tok
                anc[nl, :c - 1] = self.anc[w, :c - 1]
                anc[nl, c - 1] = w
                hist.append((w, tok, s))
                nl += 1
        # the step rests on the order of the candidates the walk consumed (the kept ones) and on the gap to the first
        # one it did not reach
        self.last_margin = step_margin([t[0] for t in cands], walked)
        self.min_margin = min(self.min_margin, self.last_margin)
        for j in range(nl, W):                      # a row left without a hypothesis: dead, its own prefix kept
            ids[j, c], anc[j, c - 1] = 0, j
        hist += [(-1, -1, NEG_INF)] * (W - nl)
        self.cum, self.err, self.ids, self.anc = cum, err, ids, anc
        self.history.append(hist)
        if len(self.pool_score) == W:
            worst = min(self.pool_score)
            Lb = T - 2 if alpha > 0 else c
            bound = dt(cum[0]) / dt(len_pen[Lb]) if nl else dt(NEG_INF)
            self.done = bool(bound <= worst)
            if nl:
                self.min_margin = min(self.min_margin, self._gap(bound, len_pen[Lb], *self._worst()))

    def finalize(self, len_pen):
        """-> the pool after the live hypotheses of a document not done entered it, sorted: lists of (score, logp,
        length, ids row). The document's own state is not changed."""
        saved = (list(self.pool_score), list(self.pool_logp), list(self.pool_len), list(self.pool_ids),
                 list(self.pool_pen), self.min_margin)
        dt, T = self.dtype, self.T
        if not self.done:
            for w in range(self.W):
                if self.cum[w] > NEG_INF:
                    self._put(dt(self.cum[w]) / dt(len_pen[T - 2]), dt(self.cum[w]), T - 2, self.ids[w].copy(),
                              len_pen[T - 2])
        order = sorted(range(len(self.pool_score)), key=lambda i: -self.pool_score[i])     # stable
        out = [(self.pool_score[i], self.pool_logp[i], self.pool_len[i], self.pool_ids[i]) for i in order]
        # the order of the results rests on the gaps between neighbouring pool scores
        margin = self.min_margin
        for i, j in zip(order[:-1], order[1:]):
            margin = min(margin, self._gap(self.pool_score[i], self.pool_pen[i], self.pool_score[j], self.pool_pen[j]))
        self.pool_score, self.pool_logp, self.pool_len, self.pool_ids, self.pool_pen, self.min_margin = saved
        return out, margin


def step_margin(sorted_scores, keep):
    """The smallest gap a step's ordering rests on: between neighbouring kept candidates (the first `keep` of the
    scores, sorted descending) and between the last kept and the first dropped one. inf where there is no pair."""
    s = np.asarray(sorted_scores[:keep + 1], np.float64)
    if s.size < 2:
        return math.inf
    return float((s[:-1] - s[1:]).min())


def top_candidates(cum, logp, W, err=None):
    """The best 2W + 1 candidates of one document as (score, beam, token, err of the beam, logp) tuples in (score
    descending, beam ascending, token ascending) order: cum [W], logp [W, V] (rows of dead beams are ignored), float64."""
    cum, logp = np.asarray(cum, np.float64), np.asarray(logp, np.float64)
    live = np.flatnonzero(cum > NEG_INF)
    V = logp.shape[1]
    sc = (cum[live, None] + logp[live]).ravel()
    beam, tok = np.repeat(live, V), np.tile(np.arange(V), live.size)
    k = min(sc.size, 2 * W + 1)
    part = np.argpartition(-sc, k - 1)[:k] if k < sc.size else np.arange(sc.size)
    # everything tied with the k-th best has to be seen by the exact ordering
    part = np.flatnonzero(sc >= sc[part].min())
    o = part[np.lexsort((tok[part], beam[part], -sc[part]))][:k]
    e = np.zeros(W) if err is None else np.asarray(err, np.float64)
    return [(float(sc[i]), int(beam[i]), int(tok[i]), float(e[beam[i]]), float(logp[beam[i], tok[i]])) for i in o]


def result_arrays(pools, n, T):
    B = len(pools)
    ids, lengths = np.zeros((B, n, T - 1), np.int64), np.zeros((B, n), np.int32)
    scores, logp = np.full((B, n), NEG_INF), np.full((B, n), NEG_INF)
    for b, pool in enumerate(pools):
        for i, (s, lp, ln, row) in enumerate(pool[:n]):
            scores[b, i], logp[b, i], lengths[b, i] = s, lp, ln
            ids[b, i, :ln] = row[1:ln + 1]
    return ids, scores, logp, lengths


def beam_search64(logp_fn, B, W, T, end, alpha, n, start=1):
    """The whole search in float64. logp_fn(b, c, prefixes) -> logp [W, V] (or (logp, err [W]): a bound on each row's
    error in the implementation under test, accumulated along the hypotheses) for document b at step c, where
    prefixes int64 [W, c] are the live id rows so far (rows of dead beams are ignored). start: one token or [B].
    -> dict(ids [B, n, T-1], scores, log_probs [B, n] float64, lengths int32 [B, n], margin [B] the smallest gap any
    decision of the document rested on, err [B] the largest accumulated bound among its results, docs)."""
    len_pen = len_pen_table(T, alpha)
    start = np.broadcast_to(np.asarray(start, np.int64), (B,))
    docs = [Doc(W, T, int(start[b])) for b in range(B)]
    errs = np.zeros(B)
    for c in range(1, T - 1):
        if all(d.done for d in docs):
            break
        for b, d in enumerate(docs):
            if d.done:
                continue
            out = logp_fn(b, c, d.ids[:, :c])
            logp, e = out if isinstance(out, tuple) else (out, np.zeros(W))
            sc_err = d.err + np.asarray(e, np.float64)
            cands = top_candidates(d.cum, logp, W, sc_err)
            # the candidate's own roundings: fl(x - mx) and the subtraction of log s (|x - mx| <= |logp| + |log s|, the
            # latter in the row's bound), then the sum cum + logp
            cands = [(s, w, t, er + EPS24 * (2 * abs(lp) + abs(s))) for s, w, t, er, lp in cands]
            errs[b] = max(errs[b], max(er for _, _, _, er in cands[:2 * W]))
            d.select(cands, c, end, len_pen, alpha)
    pools, margins = zip(*(d.finalize(len_pen) for d in docs))
    ids, scores, logp, lengths = result_arrays(pools, n, T)
    return dict(ids=ids, scores=scores, log_probs=logp, lengths=lengths, margin=np.asarray(margins), err=errs, docs=docs)


# ---------------------------------------------------------------------------------------------- svae_beam_topk
# The kernel: thread t holds entries t + 1024 e; mx = the row maximum (exact); s = sum expf(x - mx): 32 sequential
# additions per thread, 6 butterfly levels in the wave, 16 sequential additions over the waves, so every term passes
# through at most D = 54 additions of positive numbers, each adding at most 2^-24 relative: (1 + u)^54 - 1 <= 55 u.
# A term itself carries the rounding of x - mx (u |x - mx| absolute in the argument, so relative in the exponential)
# and expf's own error, taken as 2 ulp = 4 u. Weighted by the softmax p: the sum's relative error is at most
# u (55 + 4 + sum_i p_i |x_i - mx|), which is also the absolute error of its logarithm; logf adds 2 ulp of |log s|
# (4 u |log s|). Then logp = fl(fl(x - mx) - L): u |x - mx| + u |logp|; score = fl(cum + logp): u |score|.
# Subnormal terms flush to zero: at most V 2^-126, nothing at this scale.
TOPK_DEPTH = 32 + 6 + 16


def lse_bound(x):
    """Bound on the error of the kernel's log s for one f32 logits row (see above); float64 in, float."""
    x = np.asarray(x, np.float64)
    d = x - x.max()
    e = np.exp(d)
    s = e.sum()
    return EPS24 * (TOPK_DEPTH + 1 + 4 + float((e / s) @ np.abs(d)) + 4 * abs(math.log(s)))


def topk64(x, W):
    """-> (ids [2W] by (value descending, id ascending), logp float64 [2W], gaps [2W]: each value's distance to the
    next one in the order (the last: to the first dropped))."""
    x = np.asarray(x, np.float64)
    o = np.lexsort((np.arange(x.size), -x))[:2 * W + 1]
    d = x - x.max()
    lse = math.log(np.exp(d).sum())
    v = x[o]
    return o[:2 * W], d[o[:2 * W]] - lse, v[:-1] - v[1:]


def topk_score_bound(x, ids, cum):
    """Per candidate: |kernel cand_score - (cum + logp64)| <= this."""
    x = np.asarray(x, np.float64)
    d = x[ids] - x.max()
    e = np.exp(x - x.max())
    logp = d - math.log(e.sum())
    return lse_bound(x) + EPS24 * (np.abs(d) + np.abs(logp) + np.abs(cum + logp))


def row_bound(x):
    """The part of a candidate's logp bound that belongs to the row: the log-sum-exp's, and |log s| of the
    candidate's |x - mx| <= |logp| + |log s| (beam_search64 adds the candidate's own 2 |logp| and |score| terms)."""
    x = np.asarray(x, np.float64)
    return lse_bound(x) + EPS24 * abs(math.log(np.exp(x - x.max()).sum()))


# ---------------------------------------------------------------------------------------------- svae_beam_attn
def attn64(q, kcache, vcache, anc_row, doc0, h, p, window, kp, vp, scale):
    """One (row, head) of svae_beam_attn in float64: the visible key j < p comes from cache row doc0 + anc_row[j],
    key p is the row's own (kp, vp). kcache, vcache [R, H, T, hd]. -> decode_ref.attn64's (O, A, S, spread), n."""
    vis = R.visible_keys(p, window)
    old = vis[vis < p]
    rows = doc0 + np.asarray(anc_row)[old].astype(np.int64)
    k = np.concatenate([np.asarray(kcache)[rows, h, old], np.asarray(kp)[None]])
    v = np.concatenate([np.asarray(vcache)[rows, h, old], np.asarray(vp)[None]])
    return R.attn64(q, k, v, scale), vis.size


# ---------------------------------------------------------------------------------------------- the model-level test
def logp_tol(e_ref, lse_err):
    """Bound on one step's |GPU logp - float64 logp| for one candidate: every GPU logit is within 8 e_ref of the
    float64 one (the decode test's allowance: another summation order, not another precision), so x moves by at most
    8 e_ref and the log-sum-exp, 1-Lipschitz in the sup norm, by at most 8 e_ref; plus the kernel's own evaluation
    error lse_err (topk_score_bound at the row's magnitudes)."""
    return 16.0 * e_ref + lse_err


def decision_tol(e_ref, lse_err, step):
    """A decision of step `step` (1-based) compares two scores, each the sum of `step` logps."""
    return 2.0 * step * logp_tol(e_ref, lse_err)


# ---------------------------------------------------------------------------------------------- a Markov model
def markov_logp_fn(table, bound=False):
    """logp_fn of beam_search64 for logits[r] = table[previous token of r] (table f32 [V, V]): the float64
    log-softmax of that row, with row_bound per row when `bound`."""
    t64 = np.asarray(table, np.float64)
    d = t64 - t64.max(axis=1, keepdims=True)
    logp = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    rb = np.array([row_bound(r) for r in t64]) if bound else None

    def fn(b, c, prefixes):
        prev = prefixes[:, c - 1]
        return (logp[prev], rb[prev]) if bound else logp[prev]
    return fn
