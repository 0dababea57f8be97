"""Reconstruction end to end on the `tiny` preset with its initial weights and synthetic data: TransformerVAE.autoencode
against `sample` on the posterior mean, score_reconstructions on its output against the CPU restatement
(tests/textscore_ref.py), reference_rows' frame, and the reconstruct.py tool. All comparisons of ids and counts are
exact.

Row counts stay within one 64-row block of the decoder's narrow linears (24 rows here, 64 and 5 in the tool), so the
streaming decoder and `sample` add in the same order (tests/test_sample_stream_gpu.py has the rule).
"""
import functools
import json
import os
import sys

import numpy as np
import pytest
import torch

import textscore_ref as R

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import (ReconstructionScores, TextDataModule, TransformerVAE, TransformerVAEHparams, reference_rows,
                            score_reconstructions)
    from sparse_vae.core.padded_tensor import PaddedTensor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, B = 48, 24


def tool_modules():
    sys.path.insert(0, ROOT)
    try:
        import reconstruct as tool
        from train import build_config
    finally:
        sys.path.remove(ROOT)
    return tool, build_config


@functools.lru_cache(maxsize=None)
def model():
    _, build_config = tool_modules()
    m = TransformerVAE(TransformerVAEHparams(**build_config(['preset=tiny'])['model']), device='cuda')
    m.eval()
    return m


@functools.lru_cache(maxsize=None)
def batch():
    """24 synthetic documents of 20..40 tokens ([CLS] ... [SEP], zero padded)."""
    return TextDataModule(dataset_name='synthetic', seq_len=40, batch_size=B, padded=True).synthetic_batch(3, device='cuda')


@functools.lru_cache(maxsize=None)
def greedy():
    """autoencode at temperature 0: computed once, never modified."""
    ids, posterior = model().autoencode(batch(), max_length=T, temperature=0.0)
    return ids, posterior


def test_greedy_autoencode_equals_sample_on_the_posterior_mean():
    ids, posterior = greedy()
    assert ids.dtype == torch.int16 and ids.shape == (B, T - 1) and ids.is_cuda
    assert posterior.loc.shape == (B, 1, 64) and torch.equal(posterior.loc, model().encode(batch()).loc)
    want = model().sample(T, B, z=posterior.loc, temperature=0.0)
    assert torch.equal(ids.long(), want)


def test_default_max_length_is_the_batch_width_plus_one():
    """Two rows at the collated width of 512 (pad_pack's multiple): 511 decode steps of the tiny model."""
    raw = batch()['token_ids'].as_raw()
    two = {'token_ids': PaddedTensor.from_raw(raw[:2].contiguous()), 'num_tokens': batch()['num_tokens'][:2]}
    ids, _ = model().autoencode(two, temperature=0.0)
    assert raw.shape[1] == 512 and ids.shape == (2, 512)
    assert torch.equal(ids[:, :T - 2], greedy()[0][:2, :T - 2])      # the same rows, decoded further


def test_self_scoring_is_perfect():
    ids, _ = greedy()
    s = score_reconstructions(ids, ids)
    lc = R.default_lengths(ids.cpu().numpy())
    assert s.cand_len.tolist() == lc.tolist() and (lc >= 4).all()
    ref_len = s.ref_len.cpu().numpy()
    np.testing.assert_allclose(s.bleu()[ref_len == lc], 1.0, rtol=1e-12)
    full = score_reconstructions(ids, ids, cand_lengths=s.cand_len, ref_lengths=s.cand_len)
    np.testing.assert_allclose(full.bleu(), 1.0, rtol=1e-12)
    assert full.corpus_bleu() == pytest.approx(1.0, rel=1e-12) and full.edit.tolist() == [0] * B
    assert full.token_accuracy() == 1.0 == float(lc.sum()) / float(full.ref_len.sum())
    assert full.exact.tolist() == lc.tolist()


def test_scoring_against_the_originals_equals_the_restatement():
    ids, _ = greedy()
    ref, ref_len = reference_rows(batch())
    s = score_reconstructions(ids, ref, ref_lengths=ref_len)
    lc = R.default_lengths(ids.cpu().numpy())
    counts, edit, Lc, Lr = R.overlap_counts(ids.cpu().numpy(), ref.cpu().numpy(), lc, ref_len.cpu().numpy())
    assert s.matches.cpu().numpy().tolist() == counts[:, :4].tolist() and s.exact.tolist() == counts[:, 4].tolist()
    assert s.edit.tolist() == edit.tolist() and s.cand_len.tolist() == Lc.tolist() and s.ref_len.tolist() == Lr.tolist()
    assert s.corpus_bleu() == pytest.approx(R.corpus_bleu(counts[:, :4], Lc, Lr), rel=1e-12, abs=0)
    assert s.ter() == pytest.approx(R.ter(edit, Lr), rel=1e-12)
    # the default reference length (the first end token) is what reference_rows counts
    assert score_reconstructions(ids, ref).ref_len.tolist() == ref_len.tolist()


def test_sample_posterior_is_keyed_by_the_seed():
    kw = dict(max_length=T, sample_posterior=True, temperature=0.0)
    a, _ = model().autoencode(batch(), seed=5, **kw)
    b, _ = model().autoencode(batch(), seed=5, **kw)
    c, _ = model().autoencode(batch(), seed=6, **kw)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, greedy()[0])


def test_reference_rows_drop_the_start_token_and_keep_the_end_token():
    known = {'token_ids': PaddedTensor.from_raw(torch.tensor([[1, 5, 6, 2, 0, 0], [1, 7, 2, 0, 0, 0]], dtype=torch.int16)),
             'num_tokens': torch.tensor([4, 3])}
    ids, lengths = reference_rows(known)
    assert ids.tolist() == [[5, 6, 2, 0, 0], [7, 2, 0, 0, 0]] and lengths.tolist() == [3, 2]
    assert lengths.dtype == torch.int32
    raw, n = batch()['token_ids'].as_raw(), batch()['num_tokens']
    ids, lengths = reference_rows(batch())
    assert torch.equal(ids, raw[:, 1:]) and lengths.tolist() == (n - 1).tolist() and (raw[:, 0] == 1).all()
    rows = torch.arange(B, device='cuda')
    assert (ids[rows, lengths.long() - 1] == 2).all()            # the last counted token is the end token
    assert (ids[rows, lengths.long()] == 0).all() or int(lengths.max()) == ids.shape[1]


def test_autoencode_raises_below_kl_weight_one():
    m = model()
    m.hparams.kl_weight = 0.5
    try:
        with pytest.raises(RuntimeError, match='kl_weight'):
            m.autoencode(batch(), max_length=T)
    finally:
        m.hparams.kl_weight = 1.0


def test_reconstruct_py_end_to_end(tmp_path, capsys):
    """The tool on the tiny preset (64 documents of 64..128 tokens per batch, two batches, a 31-token window): every
    key is written, the printed figures are summary() of the saved counts, and the rows are autoencode's."""
    tool, _ = tool_modules()
    weights, out = tmp_path / 'w.pt', tmp_path / 'r.npz'
    torch.save(model().state_dict(), weights)
    argv = ['--preset', 'tiny', 'data.padded=True', '--weights', str(weights), '--max-length', '32', '--seed', '9']
    capsys.readouterr()
    figures = tool.main(argv + ['--max-batches', '2', '--out', str(out), '--json'])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    got = np.load(out)
    for key in ('ids', 'lengths', 'matches', 'totals', 'exact', 'edit', 'ref_len', 'hparams'):
        assert key in got.files, key
    assert got['ids'].dtype == np.int16 and got['ids'].shape == (128, 31) and got['matches'].shape == (128, 4)
    assert 'd_model' in str(got['hparams']) and '"temperature": 0.7' in str(got['hparams'])
    again = ReconstructionScores(got['matches'], got['totals'], got['exact'], got['edit'], got['lengths'],
                                 got['ref_len']).summary()
    assert printed == figures and printed['documents'] == 128 and printed['truncated'] == 128
    for key, value in again.items():
        assert printed[key] == value, key
    assert (got['ref_len'] == 31).all()                           # every original was cut to the window
    assert got['lengths'].tolist() == R.default_lengths(got['ids']).tolist()
    data = TextDataModule(dataset_name='synthetic', seq_len=128, batch_size=64, padded=True)
    first = next(iter(data.test_dataloader()))
    torch.manual_seed(9)
    want, _ = model().autoencode(first, max_length=32, seed=9, top_k=0, top_p=0.9, repetition_penalty=1.2)
    assert np.array_equal(got['ids'][:64], want.cpu().numpy())
    ref, ref_len = reference_rows(first)
    counts, edit, _, _ = R.overlap_counts(got['ids'][:64], ref[:, :31].numpy(), got['lengths'][:64],
                                          ref_len.clamp(max=31).numpy())
    assert got['matches'][:64].tolist() == counts[:, :4].tolist() and got['edit'][:64].tolist() == edit.tolist()

    # interpolation between rows 0 and 3 under greedy decoding: five rows, the ends are the two reconstructions
    rows = tool.main(argv + ['--max-batches', '1', '--temperature', '0', '--interpolate', '0', '3', '--steps', '5'])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('[')]
    assert rows.shape == (5, 31) and len(lines) == 5
    ends, _ = model().autoencode(first, max_length=32, temperature=0.0)
    assert np.array_equal(rows[0], ends[0].cpu().numpy()) and np.array_equal(rows[4], ends[3].cpu().numpy())
    with pytest.raises(SystemExit):
        tool.main(argv + ['--max-batches', '1', '--interpolate', '0', '9999'])
    with pytest.raises(SystemExit):
        tool.main(argv[:-4] + ['--max-length', '4000'])
