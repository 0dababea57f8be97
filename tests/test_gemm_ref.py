"""CPU checks of tests/gemm_ref.py, the restatements the GEMM kernel GPU tests compare against:

* route (gemm_run's choice among its four kernels) on rows derived from gemm_run as it stands, and that every case
  list names the kernel, tile count and persistence it was chosen for;
* the rotary restatement against oracle.rotary with engine.rotary_table; the float64 A-S 7.1.26 GELU against the erf
  form (its measured gap is recorded); dropout_keep's (m, N, n) indexing against test_ln_ref.py's scalar restatement;
  deviation against one wrong element; the inputs' visible differences;
* the bounds: deviation(float32 evaluation, float64 evaluation) of every epilogue's formula over the exact inputs of
  the GPU cases, the float32 K sum in the reverse order. tests/golden/gemm_bounds.json holds the measured figures:
  this test writes the file when it is absent (delete it and run this file to re-measure after a change of the cases)
  and otherwise requires the recorded figures to cover what it measures now within a quarter (the float32 sums run in
  whatever blocking the host's BLAS takes, so the last digit may differ between machines). The GPU tests read their
  bounds from the file.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch

import oracle
import gemm_ref as R
from test_ln_ref import _uniform_scalar

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16


# ------------------------------------------------------------------------------------------ route
ROUTE_ROWS = [
    ((300, 256, 192), {}, ('glds', 6, False)),
    ((4000, 3072, 520), {}, ('g256', 192, False)),
    ((8200, 2056, 520), {}, ('g256', 297, True)),
    ((64, 512, 2048), {}, ('skinny', 16, False)),
    ((256, 384, 4096), dict(a_t=1, b_t=1, epi='F32_ATOMIC', splits=4), ('g128', 24, False)),
    ((136, 132, 2056), {}, ('g128', 4, False)),
    ((4000, 3064, 520), dict(a_t=1, b_t=0, epi='BF16'), ('glds', 32 * 24, False)),
]


@pytest.mark.parametrize('shape,kw,want', ROUTE_ROWS)
def test_route_rows(shape, kw, want):
    assert R.route(*shape, n_cu=256, **kw) == want


def test_route_corners():
    assert R.route(65, 512, 2048)[0] == 'glds' and R.route(64, 512, 2048, b_t=1)[0] == 'glds'
    assert R.route(64, 512, 2048, epi='F32_ACC')[0] == 'glds' and R.route(64, 512, 2056, epi='ROTARY_BF16')[0] == 'g128'
    assert R.route(4000, 3072, 520, a_t=1, b_t=0, epi='F32_ACC')[0] == 'g256'          # the one a_t, !b_t gemm256 copy
    assert R.route(4000, 3072, 4096, a_t=1, b_t=0)[0] == 'g128'
    assert R.route(1536, 512, 32768, 1, 1, 'F32_ATOMIC', splits=16)[0] == 'g128'       # float atomics: never gemm256
    assert R.route(1536, 512, 32768, 1, 1, 'F32_ATOMIC', splits=16, slab=True) == ('g256', 192, False)
    assert R.route(512, 512, 512, epi='CE_PROB')[0] == 'g256' and R.route(512, 512, 512, 1, 1, 'F32_ACC', k_weight=True)[0] == 'g256'
    assert R.route(4000, 3072, 520, n_cu=128) == ('g256', 192, True)


def test_case_lists_route_where_they_claim():
    for name, shapes in R.ROUTES:
        for M, N, K, a_t, b_t in shapes:
            for epi in ('BF16', 'F32', 'GELU', 'GELU_BWD', 'DROPOUT_RESID'):
                assert R.route(M, N, K, a_t, b_t, epi)[0] == name, (M, N, K, a_t, b_t, epi)
            assert N % 4 == 0 and (K % 8 == 0 or (a_t and b_t)) and (not a_t or M % 8 == 0) and (not b_t or N % 8 == 0)
    assert R.route(*R.GLDS[-1][:3]) == ('glds', 21, False) and 21 % 8 == 5 and R.route(*R.G128[4][:3])[1] == 21
    assert [R.route(*s[:3])[1:] for s in R.G256] == [(192, False)] * 2
    assert R.route(*R.G256_PERSISTENT[0][:3]) == ('g256', 260, True)
    assert R.route(*R.G256_WIDE[0][:3]) == ('g256', 231, False) and -(-R.G256_WIDE[0][1] // 256) >= 32      # group = 4
    assert any(N % 8 == 4 for _, N, *_ in R.G256) and 12100 % 256 == 68
    for name, M, N, K, a_t, b_t in R.INT_CASES:
        assert R.route(M, N, K, a_t, b_t, 'F32')[0] == name
        # (the skinny kernel has no accumulating epilogue: F32_ACC at M <= 64 is the LDS-DMA kernel's)
        assert R.route(M, N, K, a_t, b_t, 'F32_ACC')[0] == ('glds' if name == 'skinny' else name)
    for name, M, N, K, a_t, b_t, rd, rc, rs in R.ROTARY_CASES:
        assert R.route(M, N, K, a_t, b_t, 'ROTARY_BF16')[0] == name and rd % 4 == 0 and rc % rd == 0 and rc < N
    assert R.route(16420, 1020, 136, epi='ROTARY_BF16')[2]
    for name, T, V, K, tiles, pers in R.CE_CASES:
        assert R.route(T, V, K, epi='CE_STATS') == (name, tiles, pers) and V % 128 and V % 8 == 4
    for name, M, N, K, hd, seq in R.DELTA_CASES:
        assert R.route(M, N, K, epi='BF16')[0] == name and M % seq == 0 and N % hd == 0 and hd % 16 == 0
    assert [R.route(M, N, K)[2] for _, M, N, K, *_ in R.DELTA_CASES[:4]] == [False, False, True, True]
    for name, M, N, K, batch in R.BATCH_CASES:
        assert R.route(M, N, K, batch=batch)[0] == name
    assert R.route(512, 512, 72, batch=48) == ('g256', 192, False)
    M, N, K = R.ATOMIC_SHAPE
    for splits in (1, 3):
        assert R.route(M, N, K, 0, 1, 'F32_ATOMIC', splits)[0] == 'glds'
        assert R.route(M, N, K, 1, 1, 'F32_ATOMIC', splits, a_rowsum=True)[0] == 'g128'
    assert R.route(M, N, K, 1, 1, 'F32_ATOMIC', 3, slab=True)[0] == 'g128'
    M, N, K, splits = R.SLAB_G256
    assert R.route(M, N, K, 1, 1, 'F32_ATOMIC', splits, slab=True) == ('g256', 195, False)
    assert -(-K // splits) <= 64 and K - 64 * (splits - 1) == 56


# ------------------------------------------------------------------------------------------ the formulas
@pytest.mark.parametrize('B,L,d', [(2, 96, 256), (3, 40, 136)])
def test_rotary_matches_the_oracle(B, L, d):
    from sparse_vae.engine import rotary_table
    x = torch.randn(B * L, 3 * d, generator=torch.Generator().manual_seed(d))
    tab = rotary_table(L, d)
    y = x.view(B, L, 3 * d)
    want = torch.cat([oracle.rotary(y[..., :d]), oracle.rotary(y[..., d:2 * d]), y[..., 2 * d:]], -1).view(B * L, 3 * d)
    got = R.epi_rotary(x, tab, 2 * d, d, L)
    assert got.dtype == f32 and (got - want).abs().max().item() <= 1e-6
    assert torch.equal(got[:, 2 * d:], x[:, 2 * d:])
    got64, S = R.epi_rotary(x.double(), tab, 2 * d, d, L, S=torch.ones(B * L, 3 * d, dtype=f64))
    assert (got64 - want.double()).abs().max().item() <= 1e-5
    c, s = tab[..., 0].double(), tab[..., 1].double()
    assert torch.allclose(S[:L, :d:2], c.abs() + s.abs()) and bool((S[:, 2 * d:] == 1).all())
    # position m % rot_seq, not m: the second sequence starts again at the table's row 0
    assert torch.allclose(got64[L:2 * L], R.epi_rotary(x[L:2 * L].double(), tab, 2 * d, d, L))


@functools.lru_cache(maxsize=None)
def gelu_gap():
    x = torch.linspace(-9, 9, 720001, dtype=f64)
    (g, gp), (ga, gpa) = R.gelu_erf(x), R.gelu_as(x)
    gap = (gpa - gp).abs().max().item()                     # g' = Phi + x phi: the two forms share phi
    assert (ga - g).abs().max().item() <= gap * 9 and bool(((ga - g).abs() <= gap * x.abs() + 1e-15).all())
    return gap


def test_gelu_forms():
    x = torch.linspace(-6, 6, 2001, dtype=f64).requires_grad_()
    y = torch.nn.functional.gelu(x)
    y.sum().backward()
    g, gp = R.gelu_erf(x.detach())
    assert torch.allclose(g, y.detach(), rtol=0, atol=1e-15) and torch.allclose(gp, x.grad, rtol=0, atol=1e-15)
    gap = gelu_gap()
    print(f'A-S 7.1.26 Phi against the erf form in float64: max gap {gap:.3e}')
    assert 1e-9 < gap <= 0.75e-7                            # the handbook's 1.5e-7 on erf is 0.75e-7 on Phi


def test_dropout_keep_indexes_by_m_N_n():
    for M, N, p in ((7, 132, 0.25), (3, 36, 0.1), (5, 1004, 0.25)):
        keep = R.dropout_keep(M, N, p, R.SEED)
        assert keep.shape == (M, N) and keep.dtype == torch.bool
        for m in range(M):
            for n in list(range(0, N, 13)) + [N - 4, N - 1]:
                assert bool(keep[m, n]) == (np.float32(_uniform_scalar(R.SEED, m * N + n)) >= np.float32(p)), (m, n)
    assert bool(R.dropout_keep(4, 36, 0.0, R.SEED).all())
    assert not torch.equal(R.dropout_keep(6, 132, 0.25, R.SEED), R.dropout_keep(6, 136, 0.25, R.SEED)[:, :132])


def test_deviation_sees_one_wrong_element():
    c = R.inputs(37, 100, 72)
    ref, S = R.gemm(c.A, c.W, 0.75, c.bias, c.resid)
    ref = R.epi_f32(ref, c.bias, c.resid)
    got = ref.float()
    assert R.deviation(got, ref, S)[0] < 2.0 ** -24
    got[29, 97] += 1e-3 * S[29, 97].float()
    d, at = R.deviation(got, ref, S)
    assert d > 0.9e-3 and at == (29, 97)
    got[3, 5] = float('nan')
    assert R.deviation(got, ref, S) == (float('inf'), (3, 5))
    ok = ref.to(bf16)
    assert R.bf16_excess(ok, ref, R.FLOOR, S)[0] <= 1.0
    ok[5, 50] = ok[5, 50] * (1 + 2.0 ** -6)                                # two bf16 ulps
    e, at = R.bf16_excess(ok, ref, R.FLOOR, S)
    assert e > 1.0 and at == (5, 50)


def test_inputs_differ_visibly_where_a_misread_would_land():
    c = R.inputs(136, 132, 72)
    for b in (c.bias, c.bias_mod):
        assert (b[4:] - b[:-4]).abs().min().item() > 0.15 and (b[8:] - b[:-8]).abs().min().item() > 0.15
        assert (b[128:] - b[:-128]).abs().min().item() > 0.15
    assert c.bias_mod.abs().max().item() < 2.3
    r = c.resid
    assert (r[1:] - r[:-1]).abs().median().item() > 1.0 and (r[:, 4:] - r[:, :-4]).abs().median().item() > 1.0
    gp = c.gp.float()
    assert (gp[1:] - gp[:-1]).abs().min().item() > 0.2 and (gp[:, 4:] - gp[:, :-4]).abs().min().item() > 0.2
    assert (gp[:, 8:] - gp[:, :-8]).abs().min().item() > 0.2 and -0.11 < gp.min().item() and gp.max().item() < 1.01
    assert len(c.c0.unique()) == 7 and torch.equal(c.Ai.float(), c.Ai.float().round()) and c.Ai.float().abs().max() == 2
    As, Bs = R.stored(R.inputs(136, 136, 72, 1, 1))
    assert As.shape == (72, 136) and Bs.shape == (72, 136) and As.is_contiguous()
    lab = R.ce_labels(300, 24580)
    assert lab.dtype == torch.int32 and {24579, 24576, 24575, 0, 127, 128, 255, 256} <= set(lab.tolist())
    assert lab[-1].item() == 24579 and 0 <= lab.min().item() and lab.max().item() < 24580


# ------------------------------------------------------------------------------------------ the bounds
ALPHA = 0.75


@functools.lru_cache(maxsize=None)
def measured():
    worst = dict.fromkeys(R.BOUND_KEYS, 0.0)

    def take(key, lo, hi, S):
        worst[key] = max(worst[key], R.deviation(lo, hi, S)[0])

    for _, M, N, K, a_t, b_t in R.REAL_CASES:
        c = R.inputs(M, N, K, a_t, b_t)
        hi, S = R.gemm(c.A, c.W, ALPHA)
        lo = R.acc(c.A, c.W, ALPHA, f32)
        take('acc', lo, hi, S)
        take('f32', R.epi_f32(lo, c.bias), R.epi_f32(hi, c.bias), S + c.bias.abs())
        take('f32', R.epi_f32(lo, c.bias, c.resid), R.epi_f32(hi, c.bias, c.resid), S + c.bias.abs() + c.resid.abs())
        Sx = S + c.bias_mod.abs()
        (gl, gpl), (gh, gph) = R.epi_gelu(lo, c.bias_mod), R.epi_gelu(hi, c.bias_mod)
        take('gelu.g', gl, gh, Sx)
        take('gelu.gp', gpl, gph, Sx + 1)
        take('gelu_bwd', R.epi_gelu_bwd(lo, c.gp), R.epi_gelu_bwd(hi, c.gp), S * c.gp.double().abs())
        for p in R.DROP_P:
            keep = R.dropout_keep(M, N, p, R.SEED)
            take('dropout', R.epi_dropout_resid(lo, c.resid, keep, p), R.epi_dropout_resid(hi, c.resid, keep, p),
                 S * R.dropout_scale(p) * keep + c.resid.abs())
        del hi, lo, S, Sx, gl, gpl, gh, gph
    from sparse_vae.engine import rotary_table
    for _, M, N, K, a_t, b_t, rd, rc, rs in R.ROTARY_CASES:
        c = R.inputs(M, N, K, a_t, b_t)
        hi, S = R.gemm(c.A, c.W, 1.0, c.bias_mod)
        tab = rotary_table(rs, rd)
        ref, Sr = R.epi_rotary(R.epi_f32(hi, c.bias_mod), tab, rc, rd, rs, S=S)
        take('rotary', R.epi_rotary(R.epi_f32(R.acc(c.A, c.W, 1.0, f32), c.bias_mod), tab, rc, rd, rs), ref, Sr)
    for _, T, V, K, _, _ in R.CE_CASES:
        c = R.inputs(T, V, K)
        hi, S = R.gemm(c.A, c.W, 1.0, c.bias_mod)
        hi, lo = R.epi_f32(hi, c.bias_mod), R.epi_f32(R.acc(c.A, c.W, 1.0, f32), c.bias_mod)
        take('ce.logit', lo, hi, S)
        lab = R.ce_labels(T, V)
        take('ce.lse', R.ce_stats(lo, lab)[0], R.ce_stats(hi, lab)[0], S.max(-1).values)
    for _, M, N, K, hd, seq in R.DELTA_CASES:
        c = R.inputs(M, N, K)
        cb = R.epi_bf16(R.acc(c.A, c.W), c.bias_mod).to(bf16)
        take('delta', R.delta(cb, c.resid, hd, seq, f32), R.delta(cb, c.resid, hd, seq),
             R.delta(cb, c.resid, hd, seq, absolute=True))
    return worst


def test_bounds_are_the_measurement():
    got, gap = measured(), gelu_gap()
    for k in R.BOUND_KEYS:
        print(f'{k}: f32-vs-f64 deviation {got[k]:.3e} -> GPU bound {max(R.TOL_FACTOR * got[k], R.FLOOR):.3e}')
    assert all(0 < v < 1e-5 for v in got.values()), got
    if not os.path.exists(R.BOUNDS_PATH):
        with open(R.BOUNDS_PATH, 'w') as f:
            json.dump({'what': 'max deviation (gemm_ref.deviation: |lo - hi| / S per element, S = |alpha| |A| |B| + '
                               '|bias| + |resid|) of the float32 evaluation of gemm_ref\'s epilogue formulas (K sum '
                               'reversed) from the float64 one over the GPU tests\' inputs, measured on the CPU by '
                               'test_gemm_ref.py; the GPU bound is max(4 x this, 2^-21), bf16 outputs carry 2^-8 |ref| '
                               'on top; gelu_as_vs_erf_gap: max |Phi_AS7.1.26 - Phi_erf| in float64, added times |x| '
                               'to the GELU bound and alone to the GELU\' bound',
                       'f32_vs_f64_deviation': {k: float(f'{got[k]:.3e}') for k in R.BOUND_KEYS},
                       'gelu_as_vs_erf_gap': float(f'{gap:.3e}')}, f, indent=1)
            f.write('\n')
        R._record.cache_clear()
    rec = R.recorded()
    assert set(rec) == set(R.BOUND_KEYS)
    for k in R.BOUND_KEYS:
        assert got[k] <= 1.25 * rec[k] and rec[k] <= 1.25 * got[k], (k, got[k], rec[k])
        assert R.bound(k) == max(4 * rec[k], 2.0 ** -21)
    assert abs(R.as_gap() / gap - 1.0) <= 1e-3
