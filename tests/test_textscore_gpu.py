"""svae_ngram_overlap and svae_edit_distance against the CPU restatement (tests/textscore_ref.py): exact integer
equality, one launch per kernel over a few hundred pairs that hold the smallest shapes at which either kernel can go
wrong, and the metrics of ReconstructionScores against the restatement's float64 to 1e-12 relative (the same formula
from the same integers: only the rounding of numpy's and math's log / exp differs).

The case list (build_cases) per pair: candidate row, reference row. Every pair is stored in matrices as wide as the
limit (leading dimensions wider than every length but the longest); the tails beyond the lengths hold a poison id
(half of the pairs) or a copy of the other side's tokens (the other half), so a read past a length changes a count.
"""
import functools

import numpy as np
import pytest
import torch

import textscore_ref as R
import sentinels as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K, _native, score_reconstructions, ReconstructionScores

MAXLEN = 2048
POISON = 31000


def build_cases():
    rng = np.random.default_rng(2024)
    big = lambda n: rng.integers(0, 32768, n)                 # noqa: E731
    cases = []
    for lc in range(6):                                        # short lengths crossed: every order's boundary
        for lr in range(6):
            cases.append((rng.integers(0, 3, lc), rng.integers(0, 3, lr)))
    for lc, lr in ((2, 9), (9, 2), (3, 40), (40, 3), (1, 300), (300, 1), (0, 70), (70, 0)):   # one side below n
        row = big(max(lc, lr))
        cases.append((row[:lc].copy(), row[:lr].copy()))
    bounds = (63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2047, 2048)
    for i, lc in enumerate(bounds):                            # sort-size, wave and strip boundaries, Lc != Lr
        lr = bounds[(i + 3) % len(bounds)]
        ref = big(lr)
        cand = R.edited_copy(rng, np.resize(ref, lc), 0.05, 32768)[:lc]
        cand = np.concatenate([cand, big(lc - len(cand))])
        cases.append((cand, ref))
        cases.append((ref.copy(), cand.copy()))
    cases.append((big(2048), big(2047)))
    cases.append((np.full(50, 7), np.full(20, 7)))             # clipping: one repeated token against a shorter row
    cases.append((np.full(20, 7), np.full(50, 7)))
    cases.append((np.full(300, 0), np.full(130, 0)))           # ... and token 0 is a token like any other
    for n in (10, 100, 700):                                   # vocabulary 3: every order clips
        cases.append((rng.integers(0, 3, n), rng.integers(0, 3, n + 5)))
    edge = big(90)
    edge[[0, 5, 6, 7, 8, 89]] = (0, 32767, 0, 0, 32767, 32767)  # tokens 0 and 32767 inside the valid part
    cases.append((edge.copy(), edge[::-1].copy()))
    cases.append((edge.copy(), np.concatenate([edge[:40], edge[45:]])))
    for n in (1, 4, 64, 500):                                  # identical pairs
        row = big(n)
        cases.append((row.copy(), row.copy()))
    for n in (6, 200):                                         # disjoint pairs
        cases.append((rng.integers(0, 100, n), rng.integers(100, 200, n + 3)))
    edited = []
    for rate in (0.05, 0.30):                                  # seeded substitutions, deletions, insertions
        for n in (40, 150, 600):
            ref = big(n)
            cases.append((R.edited_copy(rng, ref, rate, 32768), ref))
            edited.append(len(cases) - 1)
    while len(cases) < 300:                                    # P = 300: more than one pair per CU
        ref = rng.integers(0, 50, int(rng.integers(1, 120)))
        cases.append((R.edited_copy(rng, ref, 0.15, 50), ref))
    return cases[:300], edited


@functools.lru_cache(maxsize=None)
def problem():
    """(cand, ref int16 [P, MAXLEN] host tensors, lengths, restatement counts, edit, edited case numbers): built once."""
    cases, edited = build_cases()
    P = len(cases)
    cand = np.zeros((P, MAXLEN), dtype=np.int64)
    ref = np.zeros((P, MAXLEN), dtype=np.int64)
    Lc, Lr = np.zeros(P, dtype=np.int32), np.zeros(P, dtype=np.int32)
    for p, (c, r) in enumerate(cases):
        Lc[p], Lr[p] = len(c), len(r)
        cand[p, :len(c)], ref[p, :len(r)] = c, r
        if p % 2:
            cand[p, len(c):], ref[p, len(r):] = POISON, POISON
        else:                                                  # the other side's tokens, tiled over the tail
            cand[p, len(c):] = np.resize(r if len(r) else [POISON], MAXLEN - len(c))
            ref[p, len(r):] = np.resize(c if len(c) else [POISON], MAXLEN - len(r))
    counts, edit, _, _ = R.overlap_counts(cand, ref, Lc, Lr)
    for p in edited:
        assert counts[p, 3] > 0, 'an edited candidate keeps a 4-gram'
    t16 = lambda a: torch.from_numpy(a.astype(np.int16))       # noqa: E731
    return t16(cand), t16(ref), torch.from_numpy(Lc), torch.from_numpy(Lr), counts, edit, edited


def launch(P=None):
    """Both kernels over the first P pairs into sentinel-guarded outputs."""
    cand, ref, Lc, Lr, _, _, _ = problem()
    P = cand.shape[0] if P is None else P
    full5, out5 = S.matrix(P, 5, 5, torch.int32, fill=-1)
    full1, out1 = S.flat(P, torch.int32, fill=-1)
    args = (S.g(cand[:P]), S.g(ref[:P]), S.g(Lc[:P]), S.g(Lr[:P]))
    K.ngram_overlap(*args, out=out5)
    K.edit_distance(*args, out=out1)
    torch.cuda.synchronize()
    return out5, out1, full5, full1


def test_counts_equal_the_restatement_on_every_case():
    _, _, _, _, counts, edit, _ = problem()
    out5, out1, full5, full1 = launch()
    assert S.intact(full5, rows=300, cols=5) and S.intact(full1)
    got5, got1 = out5.cpu().numpy().astype(np.int64), out1.cpu().numpy().astype(np.int64)
    bad = np.nonzero((got5 != counts).any(axis=1) | (got1 != edit))[0]
    for p in bad[:10]:
        print(f'pair {p}: got {got5[p]} edit {got1[p]}, want {counts[p]} edit {edit[p]}')
    assert len(bad) == 0


def test_one_pair_and_determinism():
    _, _, _, _, counts, edit, _ = problem()
    out5, out1, full5, full1 = launch(1)
    assert S.intact(full5, rows=1, cols=5) and S.intact(full1)
    assert out5.cpu().numpy().tolist() == counts[:1].tolist() and out1.cpu().numpy().tolist() == edit[:1].tolist()
    a5, a1, _, _ = launch()
    b5, b1, _, _ = launch()
    assert torch.equal(a5, b5) and torch.equal(a1, b1)


def test_narrow_matrices_and_every_edit_instantiation():
    """Widths 5, 128, 129 and 513 (the three strip capacities of the edit kernel and an odd, 2-byte-aligned row),
    with different widths on the two sides."""
    cand, ref, Lc, Lr, counts, edit, _ = problem()
    for wc, wr in ((5, 7), (128, 300), (129, 64), (513, 2048)):
        rows = [p for p in range(300) if Lc[p] <= wc and Lr[p] <= wr][:40]
        assert len(rows) >= 20
        c, r = cand[rows, :wc].contiguous(), ref[rows, :wr].contiguous()
        args = (S.g(c), S.g(r), S.g(Lc[rows]), S.g(Lr[rows]))
        assert K.ngram_overlap(*args).cpu().numpy().tolist() == counts[rows].tolist(), (wc, wr)
        assert K.edit_distance(*args).cpu().numpy().tolist() == edit[rows].tolist(), (wc, wr)


def test_lengths_above_the_width_are_clamped():
    cand, ref, _, _, _, _, _ = problem()
    c, r = cand[:24, :70].contiguous(), ref[:24, :33].contiguous()
    over = torch.full((24,), 5000, dtype=torch.int32)
    under = torch.full((24,), -3, dtype=torch.int32)
    counts, edit, Lc, Lr = R.overlap_counts(c.numpy(), r.numpy(), over.numpy(), over.numpy())
    assert (Lc == 70).all() and (Lr == 33).all()
    assert K.ngram_overlap(S.g(c), S.g(r), S.g(over), S.g(over)).cpu().numpy().tolist() == counts.tolist()
    assert K.edit_distance(S.g(c), S.g(r), S.g(over), S.g(over)).cpu().numpy().tolist() == edit.tolist()
    assert K.ngram_overlap(S.g(c), S.g(r), S.g(under), S.g(over)).cpu().numpy().tolist() == [[0] * 5] * 24
    assert K.edit_distance(S.g(c), S.g(r), S.g(under), S.g(over)).cpu().numpy().tolist() == [33] * 24


def test_host_refusals():
    lib = _native.lib
    for fn in (lib.svae_ngram_overlap, lib.svae_edit_distance):
        assert fn(16, MAXLEN + 1, 16, 8, 16, 16, 1, 16, None) == 1       # width above SVAE_TEXT_MAX_LEN
        assert fn(16, 8, 16, 0, 16, 16, 1, 16, None) == 1
        assert fn(16, 8, 16, 8, 16, 16, 0, 16, None) == 1                 # P < 1
        for null in range(6):                                            # every pointer operand
            a = [16, 8, 16, 8, 16, 16, 1, 16, None]
            a[(0, 2, 4, 5, 7, 7)[null]] = None
            assert fn(*a) == 1
    wide = torch.zeros(2, MAXLEN + 1, dtype=torch.int16, device='cuda')
    ok = torch.zeros(2, 8, dtype=torch.int16, device='cuda')
    lens = torch.ones(2, dtype=torch.int32, device='cuda')
    with pytest.raises(ValueError, match='SVAE_TEXT_MAX_LEN'):
        K.ngram_overlap(wide, ok, lens, lens)
    with pytest.raises(ValueError, match='SVAE_TEXT_MAX_LEN'):
        K.edit_distance(ok, wide, lens, lens)
    with pytest.raises(ValueError, match='SVAE_TEXT_MAX_LEN'):
        score_reconstructions(wide, ok)
    with pytest.raises((ValueError, RuntimeError), match='no CPU fallback'):
        K.ngram_overlap(ok.cpu(), ok, lens, lens)
    with pytest.raises((ValueError, RuntimeError), match='no CPU fallback'):
        score_reconstructions(ok.cpu().long(), ok)
    for bad in (-1, 32768):
        ids = torch.full((2, 8), 5, dtype=torch.int64, device='cuda')
        ids[1, 3] = bad
        with pytest.raises(ValueError, match='outside 0..32767'):
            score_reconstructions(ids, ok)
    with pytest.raises(ValueError):
        score_reconstructions(ok[:, :4].float(), ok)
    with pytest.raises(ValueError):
        score_reconstructions(ok, ok[:1])


def test_scores_and_metrics_equal_the_restatement():
    cand, ref, Lc, Lr, counts, edit, _ = problem()
    for dtype in (torch.int16, torch.int64):
        s = score_reconstructions(S.g(cand).to(dtype), S.g(ref).to(dtype), S.g(Lc).long(), S.g(Lr))
        assert s.matches.cpu().numpy().tolist() == counts[:, :4].tolist()
        assert s.exact.cpu().numpy().tolist() == counts[:, 4].tolist() and s.edit.cpu().numpy().tolist() == edit.tolist()
        assert s.totals.cpu().numpy().tolist() == R.totals(Lc.numpy()).tolist()
    lc, lr = Lc.numpy().astype(np.int64), Lr.numpy().astype(np.int64)
    for max_n in (1, 2, 4):
        for smooth in (False, True):
            want = R.sentence_bleu(counts[:, :4], lc, lr, max_n, smooth)
            np.testing.assert_allclose(s.bleu(max_n, smooth), want, rtol=1e-12, atol=0)
        assert s.corpus_bleu(max_n) == pytest.approx(R.corpus_bleu(counts[:, :4], lc, lr, max_n), rel=1e-12)
    assert s.corpus_bleu(4) > 0 and (s.bleu() == 0).any() and (s.bleu() > 0.5).any()
    assert s.token_accuracy() == pytest.approx(R.token_accuracy(counts[:, 4], lr), rel=1e-12)
    assert s.ter() == pytest.approx(R.ter(edit, lr), rel=1e-12)
    summ = s.summary()
    assert summ['bleu2'] == s.corpus_bleu(2) and summ['pairs'] == 300 and summ['mean_ref_len'] == lr.mean()
    assert score_reconstructions(S.g(cand), S.g(ref), S.g(Lc), S.g(Lr), edit=False).edit is None
    both = ReconstructionScores.cat([s, s])
    assert len(both) == 600 and both.corpus_bleu() == pytest.approx(s.corpus_bleu(), rel=1e-12)


def test_default_lengths_follow_trim_samples():
    """A candidate ends after its first end token (full width without one); a reference without an end token ends at
    its first zero."""
    ids = torch.tensor([[7, 2, 5, 2, 0, 0], [7, 8, 9, 4, 6, 5], [7, 8, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0]], device='cuda')
    s = score_reconstructions(ids, ids)
    assert s.cand_len.tolist() == R.default_lengths(ids.cpu().numpy()).tolist() == [2, 6, 6, 6]
    assert s.ref_len.tolist() == R.default_lengths(ids.cpu().numpy(), zero_pad=True).tolist() == [2, 6, 2, 0]
    s3 = score_reconstructions(ids, ids, end_token=5)
    assert s3.cand_len.tolist() == [3, 6, 6, 6] and s3.ref_len.tolist() == [3, 6, 2, 0]
