"""CPU restatement of the reconstruction scores (csrc/textscore.hip, sparse_vae/reconstruction.py): what the GPU tests
compare against. Counts come from collections.Counter and a row-wise numpy Levenshtein; the metrics are the textbook
formulas in float64 over those integers.

    m_n     = sum over the distinct n-grams g of min(count_cand(g), count_ref(g))      (clipped matches)
    total_n = max(Lc - n + 1, 0)                                                       (candidate n-grams)
    exact   = #{j < min(Lc, Lr): c[j] == r[j]}
    BLEU    = BP * exp(mean_n log(m_n / total_n)),  BP = 1 if Lc > Lr else exp(1 - Lr / Lc);  0 when any m_n is 0 or
              Lc is 0;  smoothed: (m_n + 1) / (total_n + 1) for n >= 2
    corpus  = the same with m_n, total_n, Lc, Lr summed over the pairs first (Papineni et al. 2002)
"""
import math
from collections import Counter

import numpy as np


def ngrams(row, n):
    row = [int(t) for t in row]
    return Counter(tuple(row[j:j + n]) for j in range(len(row) - n + 1))


def ngram_matches(cand, ref, max_n=4):
    """[m_1 .. m_max_n] of one pair (sequences of ints, already cut to their lengths)."""
    out = []
    for n in range(1, max_n + 1):
        c, r = ngrams(cand, n), ngrams(ref, n)
        out.append(sum(min(k, r[g]) for g, k in c.items() if g in r))
    return out


def exact_matches(cand, ref):
    k = min(len(cand), len(ref))
    return int(np.sum(np.asarray(cand[:k]) == np.asarray(ref[:k]))) if k else 0


def levenshtein(a, b):
    """Unit-cost edit distance, one numpy row per token of a. The insertion chain within a row is the running
    minimum of (value - column) plus the column."""
    a, b = np.asarray(a, dtype=np.int64), np.asarray(b, dtype=np.int64)
    if len(a) == 0 or len(b) == 0:
        return int(len(a) + len(b))
    cols = np.arange(len(b) + 1, dtype=np.int64)
    prev = cols.copy()
    for i, t in enumerate(a, 1):
        cur = np.empty_like(prev)
        cur[0] = i
        cur[1:] = np.minimum(prev[1:] + 1, prev[:-1] + (b != t))
        prev = np.minimum.accumulate(cur - cols) + cols
    return int(prev[-1])


def overlap_counts(cand, ref, cand_len, ref_len):
    """The kernels' outputs for int arrays cand [P, wc], ref [P, wr] and lengths (clamped into [0, width]):
    (counts int64 [P, 5] = m1..m4, exact; edit int64 [P]; Lc; Lr)."""
    cand, ref = np.asarray(cand), np.asarray(ref)
    Lc = np.clip(np.asarray(cand_len, dtype=np.int64), 0, cand.shape[1])
    Lr = np.clip(np.asarray(ref_len, dtype=np.int64), 0, ref.shape[1])
    counts = np.zeros((len(cand), 5), dtype=np.int64)
    edit = np.zeros(len(cand), dtype=np.int64)
    for p in range(len(cand)):
        c, r = cand[p, :Lc[p]].astype(np.int64), ref[p, :Lr[p]].astype(np.int64)
        counts[p, :4] = ngram_matches(c, r)
        counts[p, 4] = exact_matches(c, r)
        edit[p] = levenshtein(c, r)
    return counts, edit, Lc, Lr


def totals(Lc, max_n=4):
    Lc = np.asarray(Lc, dtype=np.int64)
    return np.stack([np.maximum(Lc - n + 1, 0) for n in range(1, max_n + 1)], axis=-1)


def brevity_penalty(lc, lr):
    if lc <= 0:
        return 0.0
    return 1.0 if lc > lr else math.exp(1.0 - lr / lc)


def bleu_from_counts(m, tot, lc, lr, max_n=4, smooth=False):
    """One BLEU value from integer counts (a pair's, or a corpus's sums)."""
    if lc <= 0:
        return 0.0
    logs = 0.0
    for n in range(1, max_n + 1):
        num, den = float(m[n - 1]), float(tot[n - 1])
        if smooth and n >= 2:
            num, den = num + 1.0, den + 1.0
        if num <= 0.0 or den <= 0.0:
            return 0.0
        logs += math.log(num / den)
    return brevity_penalty(lc, lr) * math.exp(logs / max_n)


def sentence_bleu(matches, Lc, Lr, max_n=4, smooth=False):
    tot = totals(Lc)
    return np.array([bleu_from_counts(matches[p], tot[p], int(Lc[p]), int(Lr[p]), max_n, smooth)
                     for p in range(len(Lc))], dtype=np.float64)


def corpus_bleu(matches, Lc, Lr, max_n=4):
    matches, tot = np.asarray(matches, dtype=np.int64), totals(Lc)
    return bleu_from_counts(matches.sum(0), tot.sum(0), int(np.sum(Lc)), int(np.sum(Lr)), max_n)


def token_accuracy(exact, Lr):
    return float(np.sum(exact)) / float(np.sum(Lr))


def ter(edit, Lr):
    return float(np.sum(edit)) / float(np.sum(Lr))


def default_lengths(ids, end_token=2, zero_pad=False):
    """trim_samples' rule: tokens up to and including the first end token, else the full width (zero_pad: else the
    number of leading non-zero ids)."""
    ids = np.asarray(ids)
    out = np.empty(len(ids), dtype=np.int64)
    for p, row in enumerate(ids):
        hit = np.nonzero(row == end_token)[0]
        if len(hit):
            out[p] = hit[0] + 1
        elif zero_pad:
            z = np.nonzero(row == 0)[0]
            out[p] = z[0] if len(z) else len(row)
        else:
            out[p] = len(row)
    return out


def edited_copy(rng, row, rate, vocab):
    """A copy of row with seeded substitutions, deletions and insertions: `rate` edits per token in all, a third of
    them of each kind."""
    third = rate / 3.0
    out = []
    for t in row:
        u = rng.random()
        if u < third:
            out.append(int(rng.integers(0, vocab)))          # substitute
        elif u < 2 * third:
            continue                                          # delete
        else:
            out.append(int(t))
        if rng.random() < third:
            out.append(int(rng.integers(0, vocab)))          # insert
    return np.array(out, dtype=np.int64)
