"""The float64 beam search of tests/beam_ref.py against brute force, greedy decoding and a hand-written pool case
(CPU; the GPU tests hold the kernels to this reference), and reconstruct.py's --beams flags."""
import itertools
import math
import os
import sys

import numpy as np
import pytest

import beam_ref as BR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def markov_table(V, seed, scale=1.5):
    return (scale * np.random.default_rng(seed).standard_normal((V, V))).astype(np.float32)


def brute_force(table, T, start, end, alpha):
    """Every hypothesis of at most T - 2 tokens: finished ones end with the first end token, unfinished ones have
    T - 2 tokens and no end token. -> (best score, its tokens)."""
    t64 = np.asarray(table, np.float64)
    d = t64 - t64.max(axis=1, keepdims=True)
    logp = d - np.log(np.exp(d).sum(axis=1, keepdims=True))
    V, L = table.shape[0], T - 2
    pen = BR.len_pen_table(T, alpha).astype(np.float64)
    best, best_seq = -math.inf, None
    for n in range(1, L + 1):
        for seq in itertools.product(range(V), repeat=n):
            if end in seq[:-1] or (seq[-1] != end and n < L):
                continue
            prev, lp = start, 0.0
            for t in seq:
                lp += logp[prev, t]
                prev = t
            score = lp / pen[n if seq[-1] == end else L]
            if score > best:
                best, best_seq = score, seq
    return best, best_seq


@pytest.mark.parametrize('alpha', [0.0, 1.0])
@pytest.mark.parametrize('seed', [0, 1, 2])
def test_exhaustive_beam_equals_brute_force(alpha, seed):
    """V = 6, T = 6: with W = V^(T-2) beams nothing is ever pruned, so the best hypothesis is the global optimum."""
    V, T, end = 6, 6, 2
    table = markov_table(V, seed)
    out = BR.beam_search64(BR.markov_logp_fn(table), 1, V ** (T - 2), T, end, alpha, 1, start=1)
    best, seq = brute_force(table, T, 1, end, alpha)
    n = int(out['lengths'][0, 0])
    assert out['ids'][0, 0, :n].tolist() == list(seq)
    assert (out['ids'][0, 0, n:] == 0).all()
    assert abs(out['scores'][0, 0] - best) <= 1e-12 * abs(best)


@pytest.mark.parametrize('alpha', [0.0, 1.0])
def test_one_beam_is_greedy(alpha):
    V, T, end, B = 50, 20, 3, 6
    table = markov_table(V, 11, scale=2.5)
    start = np.arange(B) + 5
    out = BR.beam_search64(BR.markov_logp_fn(table), B, 1, T, end, alpha, 1, start=start)
    ended = 0
    for b in range(B):
        prev, seq = int(start[b]), []
        while len(seq) < T - 2:
            tok = int(np.lexsort((np.arange(V), -table[prev].astype(np.float64)))[0])
            seq.append(tok)
            prev = tok
            if tok == end:
                break
        ended += seq[-1] == end
        assert out['lengths'][b, 0] == len(seq)
        assert out['ids'][b, 0, :len(seq)].tolist() == seq and (out['ids'][b, 0, len(seq):] == 0).all()
    assert 0 < ended < B                           # both endings are exercised


def test_pool_rules_by_hand():
    """W = 2, alpha = 0 (score = log-probability), end token 9."""
    W, T, end = 2, 8, 9
    pen = BR.len_pen_table(T, 0.0)
    d = BR.Doc(W, T, start=1)
    # step 1: an end token of rank 0 enters the free pool; the next two candidates go live
    d.select([(-1.0, 0, end), (-2.0, 0, 5), (-3.0, 0, 6), (-4.0, 0, 7)], 1, end, pen, 0.0)
    assert d.pool_score == [-1.0] and d.pool_len == [1] and d.pool_ids[0].tolist() == [1, end, 0, 0, 0, 0, 0, 0]
    assert d.cum.tolist() == [-2.0, -3.0] and d.ids[:, :2].tolist() == [[1, 5], [1, 6]] and not d.done
    assert d.anc[:, 0].tolist() == [0, 0]
    # step 2: rank 1 end token enters (pool full), rank 2 end token is dropped although the walk reaches it
    d.select([(-2.5, 0, 4), (-3.0, 0, end), (-3.25, 1, end), (-3.5, 1, 3), (-6.0, 1, 2)], 2, end, pen, 0.0)
    assert d.pool_score == [-1.0, -3.0] and d.events['end_drop'] == 1
    assert d.cum.tolist() == [-2.5, -3.5] and d.ids[:, :3].tolist() == [[1, 5, 4], [1, 6, 3]]
    assert d.anc[:, :2].tolist() == [[0, 0], [0, 1]]
    assert not d.done                              # -2.5 can still beat the worst pool entry, -3
    # step 3: a better arrival replaces the worst entry; a worse one is refused; then the bound closes the document
    d.select([(-2.75, 0, end), (-2.875, 1, end), (-2.9, 0, 2), (-4.0, 1, 1)], 3, end, pen, 0.0)
    assert d.pool_score == [-1.0, -2.75] and d.pool_len == [1, 3]
    assert d.pool_ids[1].tolist() == [1, 5, 4, end, 0, 0, 0, 0]
    assert d.events['replace'] == 1 and d.events['reject'] == 1
    assert d.done and d.cum.tolist() == [-2.9, -4.0]
    before = (d.cum.copy(), d.ids.copy(), list(d.pool_score))
    d.select([(-0.5, 0, end)], 4, end, pen, 0.0)   # a done document takes nothing more
    assert np.array_equal(d.cum, before[0]) and np.array_equal(d.ids, before[1]) and d.pool_score == before[2]
    pool, _ = d.finalize(pen)
    assert [p[0] for p in pool] == [-1.0, -2.75]


def test_unfinished_hypotheses_enter_the_pool_at_the_end():
    """No end token ever: after T - 2 steps the live hypotheses are the results, with length T - 2 and
    score = cum / (T - 2)^alpha."""
    V, T, W = 8, 7, 3
    table = markov_table(V, 5)
    out = BR.beam_search64(BR.markov_logp_fn(table), 2, W, T, -1, 1.0, W, start=[1, 2])
    assert (out['lengths'] == T - 2).all()
    assert np.allclose(out['scores'], out['log_probs'] / np.float64(np.float32(T - 2)))
    assert (np.diff(out['scores'], axis=1) <= 0).all()
    assert (out['ids'][:, :, T - 2:] == 0).all() and (out['ids'][:, :, :T - 2] >= 0).all()


def test_step_margin():
    assert BR.step_margin([5.0, 4.0, 3.5, 1.0], 2) == 0.5      # the gap to the first dropped one counts
    assert BR.step_margin([5.0, 4.0, 3.5, 1.0], 3) == 0.5
    assert BR.step_margin([5.0, 4.75], 4) == 0.25
    assert BR.step_margin([5.0], 4) == math.inf


def test_reconstruct_parser_accepts_beams():
    sys.path.insert(0, ROOT)
    try:
        import reconstruct
    finally:
        sys.path.remove(ROOT)
    args = reconstruct.build_parser().parse_args(['--beams', '4', '--length-penalty', '0.6'])
    assert args.beams == 4 and args.length_penalty == 0.6
    args = reconstruct.build_parser().parse_args([])
    assert args.beams is None and args.length_penalty == 1.0
