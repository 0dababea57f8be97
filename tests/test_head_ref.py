"""CPU checks of tests/head_ref.py, the float64 restatements the P-head kernel tests compare against:

* the restatements chained (label logit, P and its tile sums, finalize, backward prologue, dX, dW with the k-weighted
  row sums, the one-hot part through the embedding backward's formula) against float64 autograd of logits -> chunked
  F.cross_entropy(ignore_index=0) -> times gscale, at the GPU tests' shapes: nll, dhh, dW and dbias;
* the saturation fix-up's formulas: a row recomputed with the maximum as its offset gives the same loss and gradients;
* the conditions the GPU tests rely on, on the reference alone: labels in the ragged last tile and on column V - 1,
  repeated labels, padded tails, labelled rows in every chunk, a short last chunk, row sums well away from 2^100;
* the recorded f32-vs-f64 deviations (head_ref.F32_DEV): re-measured here on the GPU tests' own inputs; each constant
  has to lie within a quarter of its measurement.
"""
import functools

import pytest
import torch

import head_ref as R


# ------------------------------------------------------------------------------------------ against float64 autograd
@pytest.mark.parametrize('nchunks', R.NCHUNKS)
@pytest.mark.parametrize('T,V,D', R.CHAIN_SHAPES + ((300, 1024, 64),))
def test_restatements_match_float64_autograd(T, V, D, nchunks):
    for case in (R.head_case(T, V, D), R.sat_case('chain', T, V, D)[:4]):
        hh, W, bias, lab = case
        L = R.ROW_SHAPES[T]
        cl = R.chunk_len_of(L, nchunks)
        ref = R.head_autograd(hh, W, bias, lab, L, nchunks, cl)
        for fix in (False, True):
            got = R.head_chain(hh, W, bias, lab, L, nchunks, cl, fix=fix)
            assert abs(got['nll'].item() - ref['nll'].item()) < 1e-12 * ref['nll'].item()
            for k in ('dhh', 'dW', 'dbias'):
                assert R.deviation(got[k], ref[k]) < 1e-11, (k, fix)
            assert (got['dhh'][lab == 0] == 0).all()
    assert got['flagged'].numel() == 1                       # the chain case's 100-nat row went through fix_rows


def test_fixed_rows_give_the_same_loss_and_dlogits():
    """fix_rows changes the offset, not the row: lse and row_loss equal finalize's, and r . P (the softmax times q)
    is the same with (P, offset) = (exp(z - c), c) and (exp(z - max), max)."""
    hh, W, bias, lab, gaps = R.sat_case('mixed')
    L = R.ROW_SHAPES[300]
    c = R.label_logit(hh, W, bias, lab)
    f = R.prob_forward(hh, W, bias, lab, c, L, 1, L - 1)
    rows = torch.tensor(sorted(gaps))
    P, lse, rl, mx = R.fix_rows(hh, W, bias, lab, c, rows)
    assert torch.allclose(lse, f['lse'][rows], rtol=1e-13) and torch.allclose(rl, f['row_loss'][rows], rtol=1e-12)
    assert torch.allclose(P * (mx - lse).exp()[:, None], f['P'][rows] * (c - f['lse'])[rows].exp()[:, None], rtol=1e-10)
    assert (P.max(-1).values == 1).all() and (P.argmax(-1) == R.SAT_HOT).all()


# ------------------------------------------------------------------------------------------ the input conditions
@pytest.mark.parametrize('T,V,D', R.KERNEL_SHAPES)
def test_head_case_reaches_the_edges(T, V, D):
    hh, W, bias, lab = R.head_case(T, V, D)
    L = R.ROW_SHAPES[T]
    assert T == R.B_SEQ * L and T > 256 and T % 32 != 0 and (T % 4 == 0) == (T == 300)
    live = lab[lab != 0]
    assert live.min() >= 3 and live.max() == V - 1 and (lab == V - 1).sum() >= 3 and lab[2 * L + 60] == V - 1
    assert (live >= (V - 1) // 128 * 128).sum() >= 5                       # labels inside the last (ragged) tile
    assert (lab == 17).sum() >= 5                                          # a repeated label for the dbias scatter
    lb = lab.view(R.B_SEQ, L)
    assert (lb[:, L - 1] == 0).all() and (lb[1, 60:] == 0).all() and (lb[2, 90:] == 0).all()
    assert (lb[0, :L - 1] != 0).all()
    for n in R.NCHUNKS:
        cl = R.chunk_len_of(L, n)
        ch = R.chunk_of(T, L, n, cl)
        assert (n - 1) * cl < L and ch.max() == n - 1
        assert all(((ch == c) & (lab != 0)).sum() > 0 for c in range(n))   # every chunk has labelled rows
        assert ch.view(R.B_SEQ, L)[0, L - 1] == n - 1                      # the last chunk also holds position L - 1
        if n > 1 and (L - 1) % n:
            assert L - 1 - (n - 1) * cl < cl                               # ... and is the short one
    assert D % 8 == 0 and V % 8 == 0
    assert {v % 256 for v in R.VOCABS} == {0, 136, 72} and {d > 512 for d in R.DIMS} == {True, False}


@pytest.mark.parametrize('kind,nflag', [('mixed', 9), ('many', 150), ('none', 0), ('chain', 1)])
def test_sat_case_sums_are_decided_by_the_inputs(kind, nflag):
    """Every labelled row's float64 sum of P is below 2^97 or above 2^103 (flagged_rows asserts it), the flagged set
    is the rows planted at 74, 78 and 100 nats, P of the 60-, 74- and 78-nat rows is finite in f32 and of the 100-nat
    rows not."""
    hh, W, bias, lab, gaps = R.sat_case(kind)
    fl = R.flagged_rows(hh, W, bias, lab)
    assert fl.tolist() == sorted(r for r, g in gaps.items() if g > 70) and fl.numel() == nflag
    c = R.label_logit(hh, W, bias, lab)
    P = R.prob_forward(hh, W, bias, lab, c, 100, 1, 99)['P']
    for r, g in gaps.items():
        assert lab[r] != 0 and abs(P[r].max().log().item() - g) < 2.0
        assert torch.isfinite(P[r].float()).all().item() == (g < 88)
        assert torch.isfinite(P[r].sum().float()).item() == (g < 88)
    if kind == 'many':
        assert nflag > 2 * 64
    if kind == 'mixed':
        assert {int(r >= 256) for r in fl.tolist()} == {0, 1}               # flagged rows in both row tiles
        se = R.prob_forward(hh, W, bias, lab, c, 100, 1, 99)['se']
        assert sum(2.0 ** 103 < se[r].item() < 2.0 ** 109.5 for r in fl.tolist()) == 3   # the 74-nat rows
    k = R.fix_case(kind)
    assert torch.isinf(k['part'][:, fl]).any(0).tolist() == [gaps[r] > 88 for r in fl.tolist()]


def test_long_last_chunk_needs_the_clamp():
    """The last chunk runs to the end of the sequence whatever chunk_len is: with 3 chunks of length 20 at L = 100,
    labelled positions 60 ... 98 have position // chunk_len = 3 or 4 and belong to chunk 2."""
    T, V, D, n, cl = R.LONG_LAST_CHUNK
    k = R.kernel_case(*R.LONG_LAST_CHUNK)
    pos = torch.arange(T) % k['L']
    beyond = (pos // cl >= n) & (k['lab'] != 0)
    assert beyond.sum() > 60 and (R.chunk_of(T, k['L'], n, cl)[beyond] == n - 1).all()
    ref = R.kernel_ref(*R.LONG_LAST_CHUNK)
    assert (ref['q'][beyond] == R.GSCALE * k['chunk_w'][n - 1].double()).all()
    auto = R.head_autograd(k['hh'], k['W'], k['bias'], k['lab'], k['L'], n, cl)     # torch.split makes 5 chunks of 20
    assert abs(auto['nll'].item() - ref['nll'].item()) > 1e-3                        # ... so it is no reference here


def test_finalize_case_has_a_tail_past_the_unrolled_loop():
    part, off, lab = R.finalize_case()
    assert part.shape == (65, 300) and 65 > 57 and 65 % 8 != 0 and (part > 0).all()


# ------------------------------------------------------------------------------------------ the recorded deviations
@functools.lru_cache(maxsize=None)
def measured():
    worst = {}

    def take(d):
        for k, v in d.items():
            worst[k] = max(worst.get(k, 0.0), v)
    for case in [(T, V, D, n) for T, V, D in R.KERNEL_SHAPES for n in R.NCHUNKS] + [R.LONG_LAST_CHUNK]:
        k = R.kernel_case(*case)
        take(R.kernel_deviations(R.kernel_eval(k, torch.float32), R.kernel_ref(*case), k['lab']))
    take({k: R.deviation(R.finalize_eval(torch.float32)[k], v) for k, v in R.finalize_eval().items()
          if k in R.F32_DEV})
    for kind in ('mixed', 'many', 'none'):
        k = R.fix_case(kind)
        take(R.fix_deviations(R.fix_eval(k, torch.float32), R.fix_eval(k)))
    for T, V, D in R.CHAIN_SHAPES:
        for n in R.NCHUNKS:
            k = R.chain_case(T, V, D, n)
            lo = R.head_chain(k['hh'], k['W'], k['bias'], k['lab'], k['L'], n, k['chunk_len'], dtype=torch.float32,
                              store=torch.bfloat16, fix=True)
            assert lo['flagged'].numel() == 1
            take(R.chain_deviations(lo, k['ref'], k['lab']))
    return worst


@pytest.mark.parametrize('key', sorted(R.F32_DEV))
def test_recorded_deviation_is_the_measurement(key):
    m, const = measured()[key], R.F32_DEV[key]
    print(f'{key}: measured f32-vs-f64 deviation {m:.3e}, recorded {const:.3e}')
    assert abs(m / const - 1.0) <= 0.25, (key, m, const)


def test_every_measured_output_is_recorded():
    assert set(measured()) == set(R.F32_DEV)


def test_deviation_sees_one_wrong_row_and_bf16_within_allows_half_an_ulp():
    k = R.kernel_case(300, 1160, 200, 3)
    ref = R.kernel_eval(k)
    bad = {key: v.clone() for key, v in ref.items()}
    bad['q'][66] *= 1.001                                     # one row on a chunk boundary
    bad['part'][3, 259] *= 1.001                              # one tile sum of one row
    d = R.kernel_deviations(bad, ref, k['lab'])
    assert d['q'] > 2e-4 and d['part'] > 2e-4 and d['lse'] == 0.0
    bad['part'][9, 259] *= 1.001                              # the ragged tile's 8 columns: a sixteenth of a full tile
    assert R.kernel_deviations(bad, ref, k['lab'])['part'] > 4 * R.bound('part')
    P = ref['P'][k['lab'] != 0]
    assert R.bf16_exp_within(P.to(torch.bfloat16), P, 1e-6) <= 1.0
    off = P.to(torch.bfloat16).double()
    off[5, 1159] *= 1 + 2.0 ** -7
    assert R.bf16_exp_within(off, P, 1e-6) > 1.0
    dhh = ref['dhh'][k['lab'] != 0]
    assert R.bf16_within(dhh.to(torch.bfloat16), dhh, 1e-6) <= 1.0
    off = dhh.to(torch.bfloat16).double()
    off[7, 196:] += dhh[7].abs().max() * 2.0 ** -6
    assert R.bf16_within(off, dhh, 1e-6) > 1.0
