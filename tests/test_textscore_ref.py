"""The CPU restatement of the reconstruction scores (tests/textscore_ref.py) against brute force, hand-computed values
and the textbook examples, and sparse_vae.interpolate_latents (plain torch). No GPU."""
import math

import numpy as np
import pytest
import torch

import textscore_ref as R


def brute_matches(c, r, n):
    """O(L^2): every distinct n-gram of c, counted on both sides by scanning."""
    grams = {tuple(c[j:j + n]) for j in range(len(c) - n + 1)}
    total = 0
    for g in grams:
        cc = sum(1 for j in range(len(c) - n + 1) if tuple(c[j:j + n]) == g)
        cr = sum(1 for j in range(len(r) - n + 1) if tuple(r[j:j + n]) == g)
        total += min(cc, cr)
    return total


def python_levenshtein(a, b):
    D = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        D[i][0] = i
    for j in range(len(b) + 1):
        D[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            D[i][j] = min(D[i - 1][j] + 1, D[i][j - 1] + 1, D[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return D[len(a)][len(b)]


def short_rows():
    rng = np.random.default_rng(5)
    for trial in range(120):
        vocab = (2, 3, 6, 32768)[trial % 4]
        yield (rng.integers(0, vocab, int(rng.integers(0, 14))).tolist(),
               rng.integers(0, vocab, int(rng.integers(0, 14))).tolist())


def test_matches_equal_brute_force():
    for c, r in short_rows():
        assert R.ngram_matches(c, r) == [brute_matches(c, r, n) for n in (1, 2, 3, 4)], (c, r)


def test_levenshtein_equals_pure_python_dp():
    for c, r in short_rows():
        assert R.levenshtein(c, r) == python_levenshtein(c, r), (c, r)
    assert R.levenshtein([ord(ch) for ch in 'kitten'], [ord(ch) for ch in 'sitting']) == 3
    assert R.levenshtein([], [4, 5, 6]) == 3 and R.levenshtein([4, 5], []) == 2 and R.levenshtein([], []) == 0


def test_papineni_clipping_example():
    """'the' x 7 against 'the cat is on the mat': the unigram count is clipped to the reference's two."""
    words = {'the': 10, 'cat': 11, 'is': 12, 'on': 13, 'mat': 14}
    cand = [words['the']] * 7
    ref = [words[w] for w in 'the cat is on the mat'.split()]
    m = R.ngram_matches(cand, ref)
    assert m == [2, 0, 0, 0]
    assert m[0] / R.totals([7])[0, 0] == 2 / 7


def test_bleu_of_identical_rows_is_one():
    row = list(range(20, 40))
    m = R.ngram_matches(row, row)
    assert m == [20, 19, 18, 17]
    assert R.sentence_bleu(np.array([m]), np.array([20]), np.array([20]))[0] == pytest.approx(1.0, abs=1e-15)
    assert R.corpus_bleu(np.array([m]), np.array([20]), np.array([20])) == pytest.approx(1.0, abs=1e-15)


def test_bleu_zeros():
    c, r = [1, 2, 3, 9, 4, 5, 6], [1, 2, 3, 8, 4, 5, 6]       # trigrams match, no 4-gram does
    m = R.ngram_matches(c, r)
    assert m[3] == 0 and m[2] > 0
    assert R.sentence_bleu(np.array([m]), np.array([7]), np.array([7]))[0] == 0.0
    assert R.sentence_bleu(np.array([m]), np.array([7]), np.array([7]), max_n=3)[0] > 0.0
    assert R.sentence_bleu(np.array([[0, 0, 0, 0]]), np.array([0]), np.array([5]))[0] == 0.0   # empty candidate
    assert R.sentence_bleu(np.array([[0, 0, 0, 0]]), np.array([0]), np.array([5]), smooth=True)[0] == 0.0
    assert R.sentence_bleu(np.array([[3, 2, 1, 0]]), np.array([3]), np.array([3]))[0] == 0.0   # shorter than the order


def test_brevity_penalty_on_a_truncated_copy():
    ref = list(range(100, 120))
    cand = ref[:10]
    m = R.ngram_matches(cand, ref)
    assert m == [10, 9, 8, 7]                                   # every precision is 1
    got = R.sentence_bleu(np.array([m]), np.array([10]), np.array([20]))[0]
    assert got == pytest.approx(math.exp(1 - 20 / 10), rel=1e-15)
    longer = R.sentence_bleu(np.array([R.ngram_matches(ref, cand)]), np.array([20]), np.array([10]))[0]
    assert longer == pytest.approx((10 / 20 * 9 / 19 * 8 / 18 * 7 / 17) ** 0.25, rel=1e-14)   # no penalty above


def test_corpus_bleu_differs_from_the_mean_of_sentences():
    """Two pairs at max_n = 2. Pair A: Lc = Lr = 4, m = (4, 3) of (4, 3): BLEU 1. Pair B: Lc = Lr = 4, m = (2, 1) of
    (4, 3): sqrt(1/2 * 1/3). Corpus: sqrt(6/8 * 4/6) = sqrt(1/2)."""
    A = ([5, 6, 7, 8], [5, 6, 7, 8])
    B = ([5, 6, 9, 9], [5, 6, 7, 8])
    m = np.array([R.ngram_matches(*A), R.ngram_matches(*B)])
    assert m[:, :2].tolist() == [[4, 3], [2, 1]]
    Lc = Lr = np.array([4, 4])
    sent = R.sentence_bleu(m, Lc, Lr, max_n=2)
    assert sent[0] == pytest.approx(1.0, rel=1e-15) and sent[1] == pytest.approx(math.sqrt(1 / 6), rel=1e-15)
    corpus = R.corpus_bleu(m, Lc, Lr, max_n=2)
    assert corpus == pytest.approx(math.sqrt(0.5), rel=1e-15)
    assert sent.mean() == pytest.approx((1 + math.sqrt(1 / 6)) / 2, rel=1e-15)      # 0.70412 against 0.70711
    assert abs(corpus - sent.mean()) > 2.9e-3


def test_smoothing():
    """(m + 1) / (total + 1) from the second order on: a pair without a 4-gram match scores above 0."""
    m, Lc, Lr = np.array([[5, 3, 1, 0]]), np.array([6]), np.array([6])
    assert R.sentence_bleu(m, Lc, Lr)[0] == 0.0
    want = (5 / 6 * 4 / 6 * 2 / 5 * 1 / 4) ** 0.25
    assert R.sentence_bleu(m, Lc, Lr, smooth=True)[0] == pytest.approx(want, rel=1e-15)
    assert R.sentence_bleu(np.array([[0, 0, 0, 0]]), Lc, Lr, smooth=True)[0] == 0.0            # order 1 is not smoothed


def test_accuracy_ter_and_default_lengths():
    assert R.exact_matches([1, 2, 3, 4], [1, 9, 3]) == 2
    assert R.token_accuracy(np.array([2, 3]), np.array([3, 5])) == 5 / 8
    assert R.ter(np.array([1, 4]), np.array([3, 5])) == 5 / 8
    ids = np.array([[7, 2, 5, 2], [7, 8, 9, 4], [7, 8, 0, 0], [0, 0, 0, 0]])
    assert R.default_lengths(ids).tolist() == [2, 4, 4, 4]
    assert R.default_lengths(ids, zero_pad=True).tolist() == [2, 4, 2, 0]


def test_edited_copies_keep_every_order():
    """What the GPU tests rely on: at 5 % and 30 % edits per token a 200-token row keeps some 4-gram."""
    rng = np.random.default_rng(11)
    ref = rng.integers(0, 32768, 200)
    for rate in (0.05, 0.30):
        cand = R.edited_copy(rng, ref, rate, 32768)
        m = R.ngram_matches(cand, ref)
        assert m[3] > 0 and m[0] < 200 and R.levenshtein(cand, ref) > 0


# ---------------------------------------------------------------------------------------------- interpolate_latents
def test_interpolate_latents_endpoints_and_line():
    from sparse_vae import interpolate_latents
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn(1, 64, generator=g), torch.randn(1, 64, generator=g)
    for mode in ('linear', 'slerp'):
        z = interpolate_latents(a, b, 9, mode=mode)
        assert z.shape == (9, 1, 64) and z.dtype == a.dtype
        assert torch.equal(z[0, 0], a[0]) and torch.equal(z[-1, 0], b[0])
    z = interpolate_latents(a, b, 5)
    assert torch.allclose(z[2, 0], 0.5 * (a[0] + b[0]), atol=1e-6)
    with pytest.raises(ValueError):
        interpolate_latents(a, b, 1)
    with pytest.raises(ValueError):
        interpolate_latents(a, b, 5, mode='cubic')


def test_slerp_preserves_the_norm_of_equal_norm_ends():
    from sparse_vae import interpolate_latents
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(64, generator=g, dtype=torch.float64), torch.randn(64, generator=g, dtype=torch.float64)
    b = b * (a.norm() / b.norm())
    z = interpolate_latents(a, b, 11, mode='slerp')
    assert torch.allclose(z[:, 0].norm(dim=1), a.norm().expand(11), rtol=1e-12, atol=0)
    lin = interpolate_latents(a, b, 11)
    assert lin[5, 0].norm() < 0.99 * a.norm()                   # the chord is shorter: the two modes differ
