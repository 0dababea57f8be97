"""The P-head cross-entropy kernels one by one (svae.h "P-head cross entropy"): svae_ce_label_logit, the
SVAE_EPI_CE_PROB head GEMM, svae_ce_prob_finalize[_fix], svae_ce_prob_bwd_prep, the SVAE_EPI_ROWSCALE_GATHER dX GEMM,
the k-weighted dW GEMM and svae_embedding_bwd_ce, at ragged shapes, against the float64 restatements of
tests/head_ref.py:
  T = 300 / 297 rows   a second 256-row tile of 44 / 41 rows; T % 32 != 0; T % 4 == 0 / 1
  V = 1024/1160/1096   aligned; a second half tile of 8 columns; no second half and a wave of 8 columns
  D = 64 / 200 / 576   one trip of the one-wave-per-row walk; idle lanes; a second trip
Each kernel is fed the reference of its inputs, not the previous kernel's output. The bounds are head_ref's: 4 x the
f32-vs-f64 deviation of the same formulas on these inputs, measured on the CPU by test_head_ref.py; bf16 outputs get
half a bf16 ulp on top. Every output buffer carries sentinels past its last row and column."""
import pytest
import torch

import head_ref as R
from sentinels import SENTINEL, dev, flat, g, intact, matrix, ratio, report

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae import _native as N

f32, bf16, i32 = torch.float32, torch.bfloat16, torch.int32


SHAPES = pytest.mark.parametrize('T,V,D', R.KERNEL_SHAPES)


# ================================================================================================ label logit
@SHAPES
@pytest.mark.parametrize('variant', ['plain', 'no_bias', 'strided'])
def test_label_logit(T, V, D, variant):
    k = R.kernel_case(T, V, D, 1)
    bias = None if variant == 'no_bias' else k['bias']
    hh = g(k['hh'])
    if variant == 'strided':                                  # ldh = D + 24; a walk with stride D lands on the 1e4
        wide = torch.full((T, D + 24), 1.0e4, dtype=bf16, device=dev)
        wide[:, :D] = hh
        hh = wide[:, :D]
    full, out = flat(T)
    K.ce_label_logit(hh, g(k['W']), None if bias is None else g(bias), g(k['lab']), T, D, out)
    torch.cuda.synchronize()
    ref = R.label_logit(k['hh'], k['W'], bias, k['lab'])
    assert intact(full)
    assert bool((out.cpu()[k['lab'] == 0] == 0).all())
    report('label_logit', R.deviation(out.cpu(), ref), R.bound('label_logit'))


# ================================================================================================ CE_PROB GEMM
def _ce_prob_gemm(k, ldc_extra=24):
    T, (V, D) = k['lab'].numel(), k['W'].shape
    ntile = -(-V // 128)
    Pfull, P = matrix(T, V, V + ldc_extra, bf16)
    pfull, part = flat(ntile * T)
    K.gemm(g(k['hh']), g(k['W']), Pfull, T, V, D, ldc=V + ldc_extra, epi=N.EPI_CE_PROB, bias=g(k['bias']), aux=part,
           labels=g(k['lab']), row_a=g(k['c']))
    torch.cuda.synchronize()
    return Pfull, P, pfull, part.view(ntile, T)


@SHAPES
def test_ce_prob_gemm(T, V, D):
    k = R.kernel_case(T, V, D, 1)
    ref = R.kernel_ref(T, V, D, k['nchunks'])
    Pfull, P, pfull, part = _ce_prob_gemm(k)
    assert intact(Pfull, T, V) and intact(pfull)              # nothing past column V - 1 or row T - 1
    live = k['lab'] != 0
    P, part = P.cpu(), part.cpu()
    assert bool((P[~live] == 0).all()) and bool((part[:, ~live] == 0).all())
    ratio('P', R.bf16_exp_within(P[live], ref['P'][live], R.bound('P')))
    d = R.kernel_deviations({'part': part}, ref, k['lab'])
    report('part', d['part'], R.bound('part'))
    report('part_last', d['part_last'], R.bound('part_last'))


# ================================================================================================ finalize
def _finalize(part, off, lab, T, L, nchunks, cl, fix=None):
    bufs = [flat(T), flat(T), flat(nchunks), flat(1)]
    (lf, lse), (rf, rl), (cf, cw), (nf, nll) = bufs
    K.ce_prob_finalize(part, part.shape[0], off, lab, T, L, nchunks, cl, lse, rl, cw, nll, fix=fix)
    torch.cuda.synchronize()
    assert all(intact(b[0]) for b in bufs)
    return lse.cpu(), rl.cpu(), cw.cpu(), nll.cpu()[0]


CHUNKED = pytest.mark.parametrize('T,V,D,nchunks,chunk_len', [(T, V, D, n, None) for T, V, D in R.KERNEL_SHAPES
                                                             for n in R.NCHUNKS] + [R.LONG_LAST_CHUNK])


@CHUNKED
def test_finalize(T, V, D, nchunks, chunk_len):
    k = R.kernel_case(T, V, D, nchunks, chunk_len)
    ref = R.kernel_ref(T, V, D, nchunks, chunk_len)
    lse, rl, cw, nll = _finalize(g(k['part']), g(k['c']), g(k['lab']), T, k['L'], nchunks, k['chunk_len'])
    dead = k['lab'] == 0
    assert bool((lse[dead] == 0).all()) and bool((rl[dead] == 0).all())
    for key, got in (('lse', lse), ('row_loss', rl), ('chunk_w', cw), ('nll', nll)):
        report(key, R.deviation(got, ref[key]), R.bound(key))


def test_finalize_unrolled_loop_with_tail():
    """ntile = 65 (V = 8320): thread slice 0 takes one unrolled trip of 8 tiles and then tile 64; synthetic sums."""
    part, off, lab = R.finalize_case()
    ref = R.finalize_eval()
    lse, rl, cw, nll = _finalize(g(part), g(off), g(lab), 300, 100, 3, R.chunk_len_of(100, 3))
    for key, got in (('fin_lse', lse), ('fin_row_loss', rl), ('fin_nll', nll)):
        report(key, R.deviation(got, ref[key]), R.bound(key))
    report('fin_chunk_w', R.deviation(cw, ref['fin_chunk_w']), R.bound('chunk_w'))


# ================================================================================================ saturation fix-up
@pytest.mark.parametrize('kind', ['mixed', 'many', 'none'])
def test_finalize_fix(kind):
    """Rows at 60 (not flagged, P ~ e^60), 74 and 78 (flagged, P finite) and 100 nats (flagged, overflowed): the exact
    flagged set; flagged rows' P, lse, row_loss and offset = the row maximum; everything else bit-unchanged against a
    run without the fix-up. 'many': 150 flagged rows, so each of the 64 blocks recomputes a second and a third row."""
    k = R.fix_case(kind)
    ref = R.fix_eval(k)
    T, V, L, fl = k['lab'].numel(), k['W'].shape[0], k['L'], k['flagged']
    lab, part = g(k['lab']), g(k['part'])
    plain = _finalize(part, g(k['c']), lab, T, L, 1, k['chunk_len'])
    Pfull, P = matrix(T, V, V + 24, bf16)
    P.copy_(g(k['P']))
    sfull, sat = flat(T + 1, i32, fill=-1)
    off = g(k['c']).clone()
    lse, rl, cw, nll = _finalize(part, off, lab, T, L, 1, k['chunk_len'],
                                 fix=(g(k['hh']), g(k['W']), g(k['bias']), P, sat))
    assert intact(Pfull, T, V) and intact(sfull)
    sat, off, P = sat.cpu(), off.cpu(), P.cpu()
    assert sat[0].item() == fl.numel() == sum(gap > 70 for gap in k['gaps'].values())
    assert sorted(sat[1:1 + fl.numel()].tolist()) == fl.tolist()
    keep = torch.ones(T, dtype=torch.bool)
    keep[fl] = False
    assert torch.equal(P[keep].view(torch.int16), k['P'][keep].view(torch.int16))
    for got, want in ((lse, plain[0]), (rl, plain[1]), (off, k['c'])):
        assert torch.equal(got[keep].view(i32), want[keep].view(i32))
    assert torch.equal(cw, plain[2])
    if fl.numel():
        # the maximum is one non-zero product plus a zero bias: exact in f32
        assert torch.equal(off[fl].double(), ref['fix_off'][fl])
        ratio('fix_P', R.bf16_exp_within(P[fl], ref['fix_P'], R.bound('fix_P')))
        assert bool((P[fl, R.SAT_HOT] == 1).all())
    got = dict(fix_lse=lse, fix_row_loss=rl, fix_nll=nll, fix_P=ref['fix_P'])
    for key, v in R.fix_deviations(got, ref).items():
        if key != 'fix_P':
            report(key, v, R.bound(key))
    report('fix_chunk_w', R.deviation(cw, ref['fix_chunk_w']), R.bound('chunk_w'))


# ================================================================================================ backward prologue
@CHUNKED
def test_bwd_prep(T, V, D, nchunks, chunk_len):
    k = R.kernel_case(T, V, D, nchunks, chunk_len)
    ref = R.kernel_ref(T, V, D, nchunks, chunk_len)
    hh, lab = g(k['hh']), g(k['lab'])
    gs = torch.full((1,), R.GSCALE, device=dev)
    for with_dbias in (True, False):
        hfull, hh_out = flat(T * D, bf16)
        (rfull, r), (qfull, q), (dfull, db) = flat(T), flat(T), flat(V, fill=0.0)
        K.ce_prob_bwd_prep(hh, g(k['lse']), g(k['c']), g(k['chunk_w']), lab, gs, T, k['L'], nchunks, k['chunk_len'], D,
                           hh_out.view(T, D), r, q, db if with_dbias else None)
        torch.cuda.synchronize()
        assert intact(hfull) and intact(rfull) and intact(qfull) and intact(dfull)
        want = (r[:, None] * hh.float()).to(bf16)             # from the kernel's own r_out, in f32
        assert torch.equal(hh_out.view(T, D).view(torch.int16), want.view(torch.int16))
        dead = lab == 0
        assert bool((q[dead] == 0).all()) and bool((r[dead] == 0).all()) and bool((hh_out.view(T, D)[dead] == 0).all())
        report('q', R.deviation(q.cpu(), ref['q']), R.bound('q'))
        report('r', R.deviation(r.cpu(), ref['r']), R.bound('r'))
        if with_dbias:
            report('dbias_scatter', R.deviation(db.cpu(), ref['dbias_scatter']), R.bound('dbias_scatter'))
        else:
            assert bool((db == 0).all())


# ================================================================================================ ROWSCALE_GATHER GEMM
def _rowscale_gather(k, Nn, ldc):
    """dX's GEMM on kernel_case's operands, N = the first Nn columns of W."""
    T, V = k['P'].shape
    W = k['W'][:, :Nn]
    Wt = g(W.t().contiguous())                                # B stored [N][K]
    full, out = matrix(T, Nn, ldc, bf16)
    gather = g(k['W'])                                        # rows of ldg = D, the first Nn columns used
    K.gemm(g(k['P']), Wt, full, T, Nn, V, ldc=ldc, epi=N.EPI_ROWSCALE_GATHER, labels=g(k['lab']), row_a=g(k['r']),
           row_b=g(k['q_gather']), gather=gather, ldg=k['W'].shape[1])
    torch.cuda.synchronize()
    return full, out


@SHAPES
def test_rowscale_gather_gemm(T, V, D):
    k = R.kernel_case(T, V, D, 3)
    ref = R.kernel_ref(T, V, D, k['nchunks'])['dhh']
    full, out = _rowscale_gather(k, D, D + 8)
    assert intact(full, T, D)
    out, live = out.cpu(), k['lab'] != 0
    assert bool((out[~live] == 0).all())
    zero_b = live & (k['q_gather'] == 0)
    assert zero_b.sum() >= 30 and bool((k['r'][zero_b] != 0).all())   # row_b == 0 on labelled rows: the product alone
    ratio('dhh, row_b == 0', R.bf16_within(out[zero_b], ref[zero_b], R.bound('dhh')))
    ratio('dhh', R.bf16_within(out[live], ref[live], R.bound('dhh')))


def test_rowscale_gather_rejects_n_not_multiple_of_8():
    """The epilogue loads the gather row in 16-byte pieces of 8 columns, so a 4-column tail (N % 8 == 4) would be
    stored without its gather term: svae_gemm refuses the shape (svae.h) and writes nothing."""
    k = R.kernel_case(300, 1160, 200, 3)
    T, V = k['P'].shape
    full = torch.full((T, 200), SENTINEL, dtype=bf16, device=dev)
    Wt = g(k['W'][:, :196].t().contiguous())
    args = dict(ldc=200, epi=N.EPI_ROWSCALE_GATHER, labels=g(k['lab']), row_a=g(k['r']), row_b=g(k['q_gather']),
                gather=g(k['W']), ldg=200)
    with pytest.raises(RuntimeError, match='svae_gemm failed with status'):
        K.gemm(g(k['P']), Wt, full, T, 196, V, **args)
    torch.cuda.synchronize()
    assert bool((full == torch.tensor(SENTINEL, dtype=bf16)).all())
    K.gemm(g(k['P']), g(k['W'][:, :192].t().contiguous()), full, T, 192, V, **args)     # the next N down is served
    torch.cuda.synchronize()
    ref = R.rowscale_gather(k['P'], k['W'][:, :192], k['r'], k['q_gather'], k['W'][:, :192], k['lab'])
    live = k['lab'] != 0
    ratio('dhh, N = 192', R.bf16_within(full.cpu()[live, :192], ref[live], R.bound('dhh')))
    assert bool((full[:, 192:] == torch.tensor(SENTINEL, dtype=bf16)).all())


# ================================================================================================ dW GEMM
@SHAPES
def test_dw_gemm_with_weighted_row_sums(T, V, D):
    """dW = P^T (r . hh) with M = V, K = T (300 / 297: no multiple of anything), a_rowsum += P^T r."""
    k = R.kernel_case(T, V, D, 3)
    ref = R.kernel_ref(T, V, D, k['nchunks'])
    (wfull, dW), (sfull, rs) = flat(V * D, fill=0.0), flat(V, fill=0.0)
    K.gemm(g(k['P']), g(k['hh_r']), dW, V, D, T, a_t=True, b_t=True, lda=V, ldb=D, ldc=D, epi=N.EPI_F32_ACC,
           a_rowsum=rs, k_weight=g(k['r']))
    torch.cuda.synchronize()
    assert intact(wfull) and intact(sfull)
    report('dW', R.deviation(dW.view(V, D).cpu(), ref['dW']), R.bound('dW'))
    report('rowsum', R.deviation(rs.cpu(), ref['rowsum']), R.bound('rowsum'))


# ================================================================================================ embedding backward
@SHAPES
def test_embedding_bwd_ce(T, V, D):
    """dtable[ids[t]] += dout[t] - q[t-1] hh[t-1] for t % L != 0, with q non-zero on the row before each sequence
    start (it must not reach the next sequence's first token), zeros in q, repeated ids, random dout."""
    k = R.kernel_case(T, V, D, 3)
    ref = R.kernel_ref(T, V, D, k['nchunks'])['dtable']
    L, ids = k['L'], k['ids']
    assert bool((k['q_emb'][L - 1::L] != 0).all()) and (k['q_emb'] == 0).sum() > 40
    assert ids.unique().numel() < T - 40 and bool((ids[::L] == 1).all())
    full, dt = flat(V * D, fill=0.0)
    K.embedding_bwd_ce(g(ids), g(k['dout']), dt, T, D, L, g(k['hh']), g(k['q_emb']))
    torch.cuda.synchronize()
    assert intact(full)
    report('dtable', R.deviation(dt.view(V, D).cpu(), ref), R.bound('dtable'))


# ================================================================================================ whole chain
@pytest.mark.parametrize('nchunks', R.NCHUNKS)
@pytest.mark.parametrize('T,V,D', R.CHAIN_SHAPES)
def test_whole_chain_matches_float64_autograd(T, V, D, nchunks):
    """The kernels chained as engine.py chains them, fix-up on, one row at 60 nats and one at 100, against float64
    autograd elementwise. The bound holds the bf16 storage of P, r . hh and dhh (head_ref.head_chain)."""
    k = R.chain_case(T, V, D, nchunks)
    hh, W, bias, lab = g(k['hh']), g(k['W']), g(k['bias']), g(k['lab'])
    L, cl, ntile = k['L'], k['chunk_len'], -(-V // 128)
    off = torch.empty(T, device=dev)
    K.ce_label_logit(hh, W, bias, lab, T, D, off)
    P = torch.empty(T, V, dtype=bf16, device=dev)
    part = torch.empty(ntile, T, device=dev)
    K.gemm(hh, W, P, T, V, D, epi=N.EPI_CE_PROB, bias=bias, aux=part, labels=lab, row_a=off)
    lse, rl, cw, nll = (torch.empty(T, device=dev), torch.empty(T, device=dev), torch.empty(nchunks, device=dev),
                        torch.empty(1, device=dev))
    sat = torch.empty(T + 1, dtype=i32, device=dev)
    K.ce_prob_finalize(part, ntile, off, lab, T, L, nchunks, cl, lse, rl, cw, nll, fix=(hh, W, bias, P, sat))
    gs = torch.full((1,), R.GSCALE, device=dev)
    hh_r = torch.empty(T, D, dtype=bf16, device=dev)
    r, q = torch.empty(T, device=dev), torch.empty(T, device=dev)
    dbias, dW = torch.zeros(V, device=dev), torch.zeros(V, D, device=dev)
    K.ce_prob_bwd_prep(hh, lse, off, cw, lab, gs, T, L, nchunks, cl, D, hh_r, r, q, dbias)
    K.gemm(P, hh_r, dW, V, D, T, a_t=True, b_t=True, lda=V, ldb=D, ldc=D, epi=N.EPI_F32_ACC, a_rowsum=dbias,
           k_weight=r)
    dhh = torch.empty(T, D, dtype=bf16, device=dev)
    K.gemm(P, W.t().contiguous(), dhh, T, D, V, epi=N.EPI_ROWSCALE_GATHER, labels=lab, row_a=r, row_b=q, gather=W,
           ldg=D)
    K.embedding_bwd_ce(g(R.next_ids(k['lab'], L)), torch.zeros(T, D, device=dev), dW, T, D, L, hh, q)
    torch.cuda.synchronize()
    hot = sorted(row for row, gap in k['gaps'].items() if gap > 70)
    assert sat[0].item() == 1 and sat[1:2].tolist() == hot
    ref, live = k['ref'], k['lab'] != 0
    got = dict(nll=nll.cpu()[0], dW=dW.cpu(), dbias=dbias.cpu(), dhh=dhh.cpu())
    assert bool((got['dhh'][~live] == 0).all())
    d = R.chain_deviations(got, ref, k['lab'])
    for key in ('chain_nll', 'chain_dW', 'chain_dbias'):
        report(key, d[key], R.bound(key))
    ratio('chain_dhh', R.bf16_within(got['dhh'][live], ref['dhh'][live], R.bound('chain_dhh')))
