"""The evaluation reductions of csrc/elementwise.hip one kernel at a time: svae_ce_seq_logprob (the per-sequence
log p(x|z) behind test_step and the IW-NLL estimate) on synthetic per-tile statistics, and with the stats-only head
GEMM in front of it in the engine's call form; svae_mutual_info (mi_marginal + mi_final) with injected noise, its
workspace's per-sample partials included. Against the float64 restatements of tests/eval_ref.py. The bounds are
eval_ref's: 4 x the f32-vs-f64 deviation of the same formulas on these inputs, measured on the CPU by test_eval_ref.py,
plus the documented error of __expf / __logf at the magnitudes involved (eval_ref.ce_intrinsic / mi_intrinsic). Every
output lies in a sentinel buffer."""
import pytest
import torch

import eval_ref as R
from sentinels import SENTINEL, dev, flat, g, intact, report

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae import _native as N

f32, bf16 = torch.float32, torch.bfloat16


# ================================================================================================ ce_seq_logprob
@pytest.mark.parametrize('V,nseq,seq', R.CE_CASES)
def test_ce_seq_logprob_from_synthetic_statistics(V, nseq, seq):
    """ntile 1 and 3 (fewer tiles than lanes), 65 (a second lane trip of one tile), 256 (four whole trips); seq 5, 7,
    4 and 9 (the four waves take unequal numbers of rows); label-0 rows, a sequence of nothing but label 0 (exactly
    0.0), a tile at (-inf, 0)."""
    c = R.ce_case(V, nseq, seq)
    ntile = c['part'].shape[1]
    ref = R.seq_logprob(c['logits'], c['labels'], seq)
    full, out = flat(nseq)
    K.ce_seq_logprob(g(c['part']), ntile, g(c['label_logit']), g(c['labels']), nseq * seq, seq, out)
    torch.cuda.synchronize()
    assert intact(full)
    got = out.cpu()
    assert got[1].item() == 0.0 and ref[1].item() == 0.0
    report(f'ce_seq_logprob V={V}', R.deviation(got, ref),
           R.bound('seq_logprob', R.ce_intrinsic(c['part'], c['labels'], seq, ref)))


def test_ce_seq_logprob_rejects_ragged_rows():
    c = R.ce_case(128, 3, 5)
    full, out = flat(3)
    with pytest.raises(RuntimeError, match='svae_ce_seq_logprob failed with status'):
        K.check(K.lib.svae_ce_seq_logprob(g(c['part']).data_ptr(), 1, g(c['label_logit']).data_ptr(),
                                          g(c['labels']).data_ptr(), 14, 5, out.data_ptr(), K.stream()),
                'svae_ce_seq_logprob')
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all())


def test_head_gemm_statistics_then_seq_logprob():
    """engine.seq_log_prob's pair: the vocabulary GEMM with epi = EPI_CE_STATS and C = None (no logits stored), then
    ce_seq_logprob, at T = 2 x 40, d = 64, V = 1024; against float64 log_softmax of the bf16-rounded operands."""
    nseq, seq, d, V = R.COMPOSITE
    c = R.composite_case()
    T, ntile = nseq * seq, V // R.CE_TILE
    ref, part_ref = R.composite_eval()
    pfull, part = flat(T * ntile * 2)
    lfull, ll = flat(T)
    full, out = flat(nseq)
    lab = g(c['labels'])
    K.gemm(g(c['hh']), g(c['W']), None, T, V, d, epi=N.EPI_CE_STATS, bias=g(c['bias']), aux=part, labels=lab,
           label_logit=ll)
    K.ce_seq_logprob(part, ntile, ll, lab, T, seq, out)
    torch.cuda.synchronize()
    assert intact(pfull) and intact(lfull) and intact(full)
    report('head GEMM statistics + ce_seq_logprob', R.deviation(out.cpu(), ref),
           R.bound('composite', R.ce_intrinsic(part_ref, c['labels'], seq, ref, tile_exp=True)))


# ================================================================================================ mutual_info
def _mutual_info(stats, eps, kl, B, Z, S, seed=0):
    wfull, ws = flat(2 * S * B)
    ofull, out = flat(1)
    K.mutual_info(g(stats), g(kl), B, Z, seed, out, ws, eps=g(eps) if eps is not None else None, S=S)
    torch.cuda.synchronize()
    assert intact(wfull) and intact(ofull)                        # nothing past ws[2 S B - 1]
    return out.cpu()[0], ws.cpu()[:S * B], ws.cpu()[S * B:]


@pytest.mark.parametrize('B,Z,S,regime', R.MI_CASES)
def test_mutual_info_against_float64(B, Z, S, regime):
    """(1, 1, 1): -log B = 0, one thread with a posterior; (2, 64, 10): the training shape's kind; (300, 70, 3): 44
    threads fold a second posterior into their online logsumexp; (5, 300, 2): a second trip of the sample's fill loop;
    (64, 4096, 1): the latent limit. 'spread': one posterior carries each logsumexp and the others underflow, in the
    block's combination and (B = 300) in a thread's own rescaling. The workspace's halves, marginal[s][i] and
    sum_z x[s][i]^2, are compared element by element as well as the scalar they reduce to."""
    stats, eps, kl = R.mi_case(B, Z, S, regime)
    ref = R.mutual_info(stats, eps, kl)
    intr = R.mi_intrinsic(stats, eps, ref)
    out, marginal, sumsq = _mutual_info(stats, eps, kl, B, Z, S)
    for what, got in (('marginal', marginal), ('sumsq', sumsq), ('out', out)):
        report(f'mutual_info {B}x{Z}x{S} {regime} {what}', R.deviation(got, ref[what]),
               R.bound(R.mi_key(Z, what), intr[what]))


def test_mutual_info_rejects_a_latent_past_the_limit():
    B, Z, S = 2, R.MI_MAX_Z + 1, 1
    wfull, ws = flat(2 * S * B)
    ofull, out = flat(1)
    with pytest.raises(RuntimeError, match='svae_mutual_info failed with status'):
        K.mutual_info(torch.zeros(B, 2 * Z, device=dev), torch.zeros(1, device=dev), B, Z, 0, out, ws,
                      eps=torch.zeros(S, B, Z, device=dev), S=S)
    torch.cuda.synchronize()
    assert bool((wfull == SENTINEL).all()) and bool((ofull == SENTINEL).all())


def test_mutual_info_in_kernel_draw_is_a_function_of_the_seed():
    B, Z, S = 2, 64, 10
    stats, _, kl = R.mi_case(B, Z, S, 'narrow')
    a = _mutual_info(stats, None, kl, B, Z, S, seed=1234)
    b = _mutual_info(stats, None, kl, B, Z, S, seed=1234)
    c = _mutual_info(stats, None, kl, B, Z, S, seed=1235)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))      # equal seeds: bit-equal, partials included
    assert bool(torch.isfinite(a[1]).all()) and bool(torch.isfinite(a[2]).all())
    assert a[0].item() != c[0].item() and bool((a[2] != c[2]).all())       # another seed: every sample differs
