"""CPU checks of tests/attn_ref.py, the float64 restatement the attention kernel test compares against:

* the closed forms (O, lse, delta, dQ, dK, dV) against float64 autograd of softmax(s - 1e7 mask) v, with and without
  each mask (key padding, causal, SparseAttention's window) and the rotary, whose inverse is the transpose of
  oracle.rotary;
* the error measure: one wrong row, one wrong 16-row tile of a ragged tail and one head's last key block are each one
  large term of row_error, where the whole-tensor norm ratio of test_kernels_gpu.py stays below its bound;
* the case list: the union of dispatch() over CASES is every path name, every query row sees a key except in the batch
  entries a case declares, no reference takes more than a few seconds;
* the recorded constants (EMU_*, F32_*): re-measured here on the GPU test's own inputs; each has to lie within a
  quarter of its measurement.
"""
import functools
import math
import time

import pytest
import torch

import oracle
import attn_ref as R

f64 = torch.float64


# ------------------------------------------------------------------------------------------ against float64 autograd
def _autograd(q, k, v, do, pad, causal, window, rot, H):
    """float64 autograd of sum(dO o softmax(s - 1e7 mask) v) through the rotary of token-major x_q, x_k [B, L, d]."""
    xq, xk, xv = (t.to(f64).clone().requires_grad_() for t in (q, k, v))
    qr, kr = (R.rotate(xq, rot), R.rotate(xk, rot)) if rot is not None else (xq, xk)
    qh, kh, vh = R.heads(qr, H), R.heads(kr, H), R.heads(xv, H)
    s = qh @ kh.transpose(-1, -2) * qh.shape[-1] ** -0.5
    mask = R.hidden(q.shape[0], q.shape[1], k.shape[1], pad, causal, window)
    o = (s - 1e7 * mask.to(f64)).softmax(-1) @ vh
    (o * R.heads(do.to(f64), H)).sum().backward()
    lse = torch.logsumexp(s.detach() - 1e7 * mask.to(f64), -1)
    return dict(O=o.detach(), lse=lse, dQ=R.heads(xq.grad, H), dK=R.heads(xk.grad, H), dV=R.heads(xv.grad, H),
                q=qr.detach(), k=kr.detach())


@pytest.mark.parametrize('causal,window,padded,rot', [
    (False, 0, False, False), (False, 0, True, False), (True, 0, False, False), (True, 0, True, False),
    (True, 1, False, False), (True, 2, True, False), (False, 0, True, True), (True, 0, True, True),
    (True, 2, True, True)])
def test_closed_forms_match_float64_autograd(causal, window, padded, rot):
    B, H, Lk, hd = 2, 3, 108, 16
    Lq = Lk if causal else 41
    d = H * hd
    gen = torch.Generator().manual_seed(11 + Lq + window)
    q, do = torch.randn(B, Lq, d, generator=gen, dtype=f64), torch.randn(B, Lq, d, generator=gen, dtype=f64)
    k, v = torch.randn(B, Lk, d, generator=gen, dtype=f64), torch.randn(B, Lk, d, generator=gen, dtype=f64)
    pad = None
    if padded:
        pad = torch.zeros(B, Lk, dtype=torch.uint8)
        pad[0, 90:], pad[1, [5, 40, 64]] = 1, 1
    tab = None
    if rot:
        tab = R.rot_of(R.Case('t', 'self', B, H, Lq, Lk, hd, causal, window, None, None, False, 'bf16', True))
    ag = _autograd(q, k, v, do, pad, causal, window, tab, H)
    got = R.attention(R.heads(ag['q'], H) if rot else R.heads(q, H), R.heads(ag['k'], H) if rot else R.heads(k, H),
                      R.heads(v, H), R.heads(do, H), pad=pad, causal=causal, window=window, rot=tab)
    for key in ('O', 'lse', 'dQ', 'dK', 'dV'):
        err = (got[key] - ag[key]).abs().max().item() / ag[key].abs().max().item()
        assert err < 1e-12, (key, err)
    assert torch.allclose(got['delta'], (R.heads(do, H) * ag['O']).sum(-1), rtol=0, atol=1e-12)


def test_table_rotation_is_oracle_rotary_and_its_inverse_the_transpose():
    B, L, d = 2, 77, 32
    gen = torch.Generator().manual_seed(3)
    x, g = torch.randn(B, L, d, generator=gen, dtype=f64), torch.randn(B, L, d, generator=gen, dtype=f64)
    tab = R.rot_of(R.Case('t', 'self', B, 2, L, L, 16, True, 0, None, None, False, 'bf16', True))
    assert (R.rotate(x, tab) - oracle.rotary(x)).abs().max() < 1e-5           # (the table's factors are float32)
    assert abs((R.rotate(x, tab) * g).sum() - (x * R.rotate(g, tab, inverse=True)).sum()) < 1e-10
    assert (R.rotate(R.rotate(x, tab), tab, inverse=True) - x).abs().max() < 1e-6


def test_rows_without_a_key_are_zero_with_lse_minus_inf():
    c = R.BY_NAME['entry1_padded_self_L200']
    ref = R.reference(c.name)
    assert bool(torch.isinf(ref['lse'][1]).all()) and bool((ref['lse'][1] < 0).all())
    assert bool(torch.isfinite(ref['lse'][0]).all())
    for key in ('O', 'dQ', 'dK', 'dV'):
        assert bool((ref[key][1] == 0).all()) and bool(torch.isfinite(ref[key]).all())
        assert bool((ref['mag'][key][1] == 0).all())


# ------------------------------------------------------------------------------------------ the error measure
def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm()).item()


def test_row_error_sees_what_the_norm_ratio_averages_away():
    """One query row (or key row) half off; for dK and dV also the ragged tail of the last 16-row tile lost and one
    head's last key block a quarter off: each is past the GPU test's bound in row_error, while the whole-tensor norm
    ratio of test_kernels_gpu.py (1e-2 for O, 2e-2 for the gradients) does not notice."""
    name = 'self_L600_hd64'
    ref = R.reference(name)
    for key, bound_rel in (('O', 1e-2), ('dQ', 2e-2), ('dK', 2e-2), ('dV', 2e-2)):
        good = R.emulation(name)[key]
        assert R.row_error(good, ref[key], ref['mag'][key]) <= R.RECORDED[key] * 1.25
        faults = {'row': good.clone()}
        faults['row'][1, 0, 333] *= 1.5
        if key in ('dK', 'dV'):
            faults['tile'] = good.clone()
            faults['tile'][0, 1, 592:600] = 0.0
            faults['block'] = good.clone()
            faults['block'][1, 1, 512:] *= 1.25
        for what, bad in faults.items():
            err, rel = R.row_error(bad, ref[key], ref['mag'][key]), _rel(bad, ref[key])
            print(f'{key} {what}: row_error {err:.3e} (bound {R.bound(key):.3e}), norm ratio {rel:.3e} ({bound_rel})')
            assert err > R.bound(key) and rel < bound_rel, (key, what, err, rel)


def test_row_error_requires_exact_zeros_and_finite_values():
    name = 'isolated_self_L330'
    ref = R.reference(name)
    pad = R.inputs(name)['pad'].bool()
    for key in ('dK', 'dV'):
        assert bool((ref['mag'][key].transpose(1, 2)[pad] == 0).all())      # a padded key's rows have no magnitude
        bad = ref[key].clone()
        bad[0, 1, 64, 7] = 1e-30
        assert R.row_error(bad, ref[key], ref['mag'][key]) == math.inf
        bad = ref[key].clone()
        bad[1, 0, 100, 0] = math.nan
        assert R.row_error(bad, ref[key], ref['mag'][key]) == math.inf
        assert R.row_error(ref[key], ref[key], ref['mag'][key]) == 0.0
    lse = ref['lse'].clone()
    assert R.scalar_error(lse, ref['lse']) == 0.0
    lse[0, 0, 5] = -math.inf
    assert R.scalar_error(lse, ref['lse']) == math.inf


# ------------------------------------------------------------------------------------------ the case list
def test_cases_reach_every_path():
    reached = set()
    for c in R.CASES:
        paths = R.dispatch_of(c)
        assert paths <= R.PATHS, (c.name, paths - R.PATHS)
        reached |= paths
    assert reached == R.PATHS, sorted(R.PATHS - reached)


def test_cases_are_the_issue_shapes():
    by = R.BY_NAME
    assert all(c.B * c.H <= 6 for c in R.CASES) and len({c.name for c in R.CASES}) == len(R.CASES)
    for hd in (64, 96):
        assert f'bwd8<{hd},1>' in R.dispatch_of(by[f'self_L200_hd{hd}'])
        assert 'dq_reduce_bf16_rot' not in R.dispatch_of(by[f'self_L200_hd{hd}'])      # all of dQ is the direct store
        assert {f'bwd8<{hd},2>', 'dq_direct_rot', 'dq_reduce_bf16_rot'} <= R.dispatch_of(by[f'self_L600_hd{hd}'])
        assert {'split_kv'} <= R.dispatch_of(by[f'split_64x2100_hd{hd}'])
        assert {'split_kv', 'split_kv_empty_slice'} <= R.dispatch_of(by[f'split_64x2100_hd{hd}_pad1500'])
    assert 'bwd4<64>' in R.dispatch_of(by['learned_64x330_hd64'])
    assert 'bwd8<96,1>' in R.dispatch_of(by['learned_64x330_hd96'])
    assert {'delta_inkernel', 'fwd32'} <= R.dispatch_of(by['self_L200_hd64'])
    assert 'fwd16<64>' in R.dispatch_of(by['self_L4160_hd64'])
    assert {'bwd4<128>', 'delta_pass<16>'} <= R.dispatch_of(by['self_L130_hd128_o32'])
    assert 'delta_pass<8>' in R.dispatch_of(by['self_L130_hd16_o'])
    assert {'cls_split'} <= R.dispatch_of(by['window1_L320_hd64'])
    assert {'bwd8<64,2>', 'window_compact', 'cls_split'} <= R.dispatch_of(by['window1_L576_hd64'])
    assert {c.hd for c in R.CASES} >= {8, 16, 48, 64, 80, 96, 112, 128}
    # the masks: whole tiles, whole 256 / 512-key backward blocks and whole split-KV slices of padding; isolated keys
    pad = R.pad_of(by['short70_self_L600'])
    assert bool(pad[:, 128:].all()) and bool((pad[:, :63] == 0).all())
    assert R.pad_of(by['isolated_self_L330'])[0].nonzero().flatten().tolist() == [3, 64, 65, 255, 256, 329]
    assert bool(R.pad_of(by['lead128_cross_200x330'])[:, :128].all())
    assert bool(R.pad_of(by['split_64x2100_hd64_pad1500'])[:, 1500:].all())
    a, b = R.pad_of(by['self_L600_hd64'])
    assert 0 < a.sum() < b.sum() < 56                                                  # a different suffix per entry


@pytest.mark.parametrize('name', [c.name for c in R.CASES])
def test_every_query_sees_a_key_except_where_declared(name):
    c = R.BY_NAME[name]
    hid = R.hidden(c.B, c.Lq, c.Lk, R.pad_of(c), c.causal, c.window)
    blind = hid.all(-1)[:, 0]                                                              # [B, Lq]
    for b in range(c.B):
        assert bool(blind[b].all()) if R.ALL_PADDED.get(name) == b else not bool(blind[b].any()), (name, b)


def test_no_reference_takes_more_than_a_few_seconds():
    for c in R.CASES:
        x = R.inputs(c.name)
        t0 = time.perf_counter()
        R.attention(*R._hv(c, x), pad=x['pad'], causal=c.causal, window=c.window, rot=x['rot'])
        assert time.perf_counter() - t0 < 5.0, c.name


# ------------------------------------------------------------------------------------------ the recorded constants
@functools.lru_cache(maxsize=None)
def measured():
    worst = {}
    for c in R.CASES:
        for k, v in R.measure(c.name).items():
            worst[k] = max(worst.get(k, 0.0), v)
    return worst


@pytest.mark.parametrize('key', sorted(R.RECORDED))
def test_recorded_constant_is_the_measurement(key):
    m, const = measured()[key], R.RECORDED[key]
    print(f'{key}: measured {m:.3e}, recorded {const:.3e}')
    assert abs(m / const - 1.0) <= 0.25, (key, m, const)


def test_every_measured_output_is_recorded():
    assert set(measured()) == set(R.RECORDED)
