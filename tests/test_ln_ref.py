"""CPU checks of tests/ln_ref.py, the restatements the LayerNorm kernel GPU tests compare against:

* ln_fwd / ln_bwd / ln_bwd_multi in float64 against F.layer_norm in float64 and its autograd, with dres, the zero_mod
  move and gmul;
* dropout_keep (the numpy restatement of common.h's rand_uniform4) against a scalar restatement in Python integers,
  its keep rate, p = 0, and that the mask depends only on (seed, flat index >> 2);
* the launch plans: the loop cases give some wave the rows they claim and some wave fewer, the widths reach every
  layout;
* the bounds: deviation(float32 restatement, float64 restatement) of mean, rstd, y, dx, dw, db on the exact inputs
  of every GPU case family. tests/golden/ln_bounds.json holds the measured figures: this test writes the file when it
  is absent (delete it and run this file to re-measure after a change of the cases) and otherwise requires every
  recorded figure to lie within a quarter of what it measures now (the float32 sums run in whatever order the host's
  torch takes, so the last digit may differ between machines). The GPU tests read their bounds from the file.
"""
import functools
import json
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import ln_ref as R

f64 = torch.float64


def _close(a, b, tol=1e-12):
    return R.deviation(a, b) <= tol


# ------------------------------------------------------------------------------------------ formulas vs autograd
def _autograd(x, ws, bs, dys):
    xr = x.double().clone().requires_grad_()
    wr = [w.double().clone().requires_grad_() for w in ws]
    br = [b.double().clone().requires_grad_() for b in bs]
    ys = [F.layer_norm(xr, (x.shape[1],), w, b, R.EPS) for w, b in zip(wr, br)]
    sum((y * dy.double()).sum() for y, dy in zip(ys, dys)).backward()
    return ys, xr.grad, [w.grad for w in wr], [b.grad for b in br]


@pytest.mark.parametrize('rows,D', [(5, 8), (75, 132), (111, 576)])
def test_ln_fwd_bwd_match_layer_norm_autograd(rows, D):
    c = R.inputs(rows, D)
    (yr,), dxr, (dwr,), (dbr,) = _autograd(c.x, c.ws, c.bs, c.dys)
    y, mean, rstd = R.ln_fwd(c.x, c.ws[0], c.bs[0])
    assert _close(y, yr.detach())
    xd = c.x.double()
    assert _close(mean, xd.mean(-1), 1e-13) and _close(rstd, (xd.var(-1, unbiased=False) + 1e-5).rsqrt(), 1e-13)
    dx, dw, db, zrow = R.ln_bwd(c.dys[0], c.x, c.ws[0])
    assert zrow is None and _close(dx, dxr) and _close(dw, dwr) and _close(db, dbr)
    dx, dw, db, _ = R.ln_bwd(c.dys[0], c.x, c.ws[0], dres=c.dres)
    assert _close(dx, dxr + c.dres.double()) and _close(dw, dwr) and _close(db, dbr)
    # the zero_mod move: the rows leave dx for zrow, the others and the affine gradients stay
    zm = 37 if rows > 37 else 2
    dx, dw, db, zrow = R.ln_bwd(c.dys[0], c.x, c.ws[0], dres=c.dres, zero_mod=zm)
    full = dxr + c.dres.double()
    moved = torch.arange(rows) % zm == 0
    assert zrow.shape == (-(-rows // zm), D) and _close(zrow, full[moved])
    assert bool((dx[moved] == 0).all()) and torch.equal(dx[~moved], R.ln_bwd(c.dys[0], c.x, c.ws[0], c.dres)[0][~moved])
    assert _close(dw, dwr) and _close(db, dbr)
    # gmul: (LN'(dy)) gmul; the affine gradients are the LayerNorm's own
    dx, dw, db, _ = R.ln_bwd(c.dys[0], c.x, c.ws[0], gmul=c.gp)
    assert _close(dx, dxr * c.gp.double()) and _close(dw, dwr) and _close(db, dbr)


@pytest.mark.parametrize('n', R.MULTI_N)
def test_ln_bwd_multi_matches_autograd_of_the_summed_heads(n):
    c = R.inputs(75, 132, n)
    ys, dxr, dwr, dbr = _autograd(c.x, c.ws, c.bs, c.dys)
    for j in range(n):
        assert _close(R.ln_fwd(c.x, c.ws[j], c.bs[j])[0], ys[j].detach())
    assert c.ws[-1].mean().item() > 0.9 * n and c.bs[-1].mean().item() > n - 1.5      # visibly different affines
    for dres in (None, c.dres):
        dx, grads = R.ln_bwd_multi(c.dys, c.x, c.ws, dres)
        assert _close(dx, dxr + (dres.double() if dres is not None else 0))
        for j in range(n):
            assert _close(grads[j][0], dwr[j]) and _close(grads[j][1], dbr[j])


# ------------------------------------------------------------------------------------------ the dropout mask
def _uniform_scalar(seed, idx):
    """rand_uniform4 for one flat element index, in Python integers."""
    m = (1 << 64) - 1
    z = (seed * 0x9E3779B97F4A7C15 + (idx >> 2) + 0x632BE59BD9B4E019) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    z ^= z >> 31
    return (((z >> (16 * (idx & 3))) & 0xFFFF) + 0.5) / 65536.0


def test_dropout_uniforms_match_the_scalar_restatement():
    for seed in (0, 1, 0x9E3779B97F4A7C15, (1 << 64) - 1):
        u = R.dropout_uniforms(seed, 7, 12)
        assert u.dtype.name == 'float32'
        for idx in range(84):
            assert float(u.flat[idx]) == _uniform_scalar(seed, idx), (seed, idx)
    u = R.dropout_uniforms(5, 3, 1 << 20)                   # far indices
    for idx in (3 * (1 << 20) - 1, (1 << 21) + 2):
        assert float(u.flat[idx]) == _uniform_scalar(5, idx)


@pytest.mark.parametrize('p', [0.1, 0.25, 0.5])
def test_dropout_keep_rate(p):
    n = 1 << 20
    keep = R.dropout_keep(0xC0FFEE + int(p * 100), 1024, 1024, p)
    kept = int(keep.sum())
    sigma = math.sqrt(n * p * (1 - p))
    print(f'dropout p={p}: kept {kept} of {n}, expected {n * (1 - p):.0f}, sigma {sigma:.0f}')
    assert keep.dtype == torch.bool and abs(kept - n * (1 - p)) <= 5 * sigma


def test_dropout_keep_depends_on_seed_and_flat_index_only():
    assert bool(R.dropout_keep(3, 16, 64, 0.0).all())                    # p = 0 keeps everything
    a = R.dropout_uniforms(9, 24, 40)
    assert (a.ravel() == R.dropout_uniforms(9, 40, 24).ravel()).all()    # the shape is no part of it
    assert (a.ravel() == R.dropout_uniforms(9, 1, 960).ravel()).all()
    assert (a.ravel()[:480] == R.dropout_uniforms(9, 12, 40).ravel()).all()
    assert (a != R.dropout_uniforms(10, 24, 40)).mean() > 0.99
    assert len(set(a.ravel()[:4].tolist())) > 1                          # four fields of one hash, not one repeated
    assert R.dropout_scale(0.0) == 1.0 and abs(R.dropout_scale(0.1) - 1 / 0.9) < 1e-7


# ------------------------------------------------------------------------------------------ plans and cases
def test_loop_cases_loop_and_widths_reach_every_layout():
    for rows, D, most in R.FWD_LOOP:
        assert R.fwd_rows_per_wave(rows, D) == (most - 1, most), (rows, D)
        assert R.fwd_rows_per_wave(rows - 8, D)[1] == most - 1           # and is the smallest such grid
    for rows, D, most in R.BWD_LOOP:
        assert R.bwd_rows_per_wave(rows) == (most - 1, most)
    for rows, D in R.MULTI_BWD_CASES[:3] + R.GELU_CASES[::2]:
        assert R.bwd_rows_per_wave(rows)[1] >= 2
    assert all(R.fwd_rows_per_wave(r, D) in ((1, 1), (0, 1)) and R.bwd_rows_per_wave(r)[1] == 1 for r, D in R.SMALL)
    assert {R.fwd_maxv(D) for D in R.WIDTHS} == {2, 3, 4, 5} == {R.fwd_maxv(D) for D in R.LOOP_WIDTHS} | {4}
    assert {R.bwd_maxv(D) for D in R.WIDTHS} == {2, 3, 4} == {R.bwd_maxv(D) for D in R.LOOP_WIDTHS}
    assert [R.fwd_maxv(D) for D in (132, 516, 772, 1020, 1024, 832)] == [3, 3, 5, 5, 4, 4]
    # every layout filled and partly filled: D == 256 MAXV fills every lane's every chunk
    for mv, full, part in ((2, 512, 64), (3, 768, 576), (4, 1024, 832)):
        assert R.fwd_maxv(full) == R.fwd_maxv(part) == R.bwd_maxv(full) == R.bwd_maxv(part) == mv
        assert full == 256 * mv and part in R.WIDTHS and full in R.WIDTHS
    assert all(D % 64 == 0 for D in R.ENGINE_WIDTHS) and all(D % 4 == 0 and D % 64 for D in R.LIB_WIDTHS)
    assert R.ZERO_MOD % 4 and all(r % R.ZERO_MOD == 0 for r, _ in R.ZSPLICE_CASES)
    header = open(os.path.join(os.path.dirname(R.BOUNDS_PATH), '..', '..', 'include', 'svae.h')).read()
    assert int(re.search(r'#define SVAE_LN_MULTI_MAX (\d+)', header).group(1)) == R.LN_MULTI_MAX
    assert int(re.search(r'#define SVAE_COLSUM_MAX (\d+)', header).group(1)) == R.COLSUM_MAX


def test_deviation_sees_one_wrong_element():
    ref = torch.randn(300, 132, generator=torch.Generator().manual_seed(3), dtype=f64)
    got = ref.float()
    assert R.deviation(got, ref) < 2.0 ** -24
    got[177, 77] += 1e-3
    assert R.deviation(got, ref) > 1e-4 and R.deviation(got, ref, rows=False) > 1e-4
    ok = ref.bfloat16()
    assert R.bf16_excess(ok, ref, R.FLOOR) <= 1.0
    ok[5, 5] = ok[5, 5] * (1 + 2.0 ** -6)                                # two bf16 ulps
    assert R.bf16_excess(ok, ref, R.FLOOR) > 1.0


# ------------------------------------------------------------------------------------------ the bounds
def _xs(c):
    return (c.x, c.x.bfloat16().float())                    # the kernels' two input types: f32, and bf16 exactly


@functools.lru_cache(maxsize=None)
def measured():
    worst = dict.fromkeys(R.BOUND_KEYS, 0.0)

    def take(key, lo, hi, rows):
        worst[key] = max(worst[key], R.deviation(lo, hi, rows=rows))

    for rows, D in R.FWD_CASES:
        n = R.LN_MULTI_MAX if (rows, D) in [c[:2] for c in R.FWD_LOOP] else 1     # the multi forward's loop cases
        c = R.inputs(rows, D, n)
        for x in _xs(c):
            for j in range(n):
                lo, hi = R.ln_fwd(x, c.ws[j], c.bs[j], torch.float32), R.ln_fwd(x, c.ws[j], c.bs[j])
                take('fwd.y', lo[0], hi[0], True)
                take('fwd.mean', lo[1], hi[1], False)
                take('fwd.rstd', lo[2], hi[2], False)
    for rows, D in R.BWD_CASES:
        c = R.inputs(rows, D)
        for x in _xs(c):
            for dres in (None, c.dres):
                lo = R.ln_bwd(c.dys[0], x, c.ws[0], dres, dtype=torch.float32)
                hi = R.ln_bwd(c.dys[0], x, c.ws[0], dres)
                take('bwd.dx', lo[0], hi[0], True)
                take('bwd.dw', lo[1], hi[1], False)
                take('bwd.db', lo[2], hi[2], False)
    for rows, D in R.GELU_CASES:
        c = R.inputs(rows, D)
        for x in _xs(c):
            take('gelu.out', R.ln_bwd(c.dys[0], x, c.ws[0], gmul=c.gp, dtype=torch.float32)[0],
                 R.ln_bwd(c.dys[0], x, c.ws[0], gmul=c.gp)[0], True)
    for rows, D in R.MULTI_BWD_CASES:
        for n in R.MULTI_N:
            c = R.inputs(rows, D, n)
            for dres in (None, c.dres):
                lo, hi = R.ln_bwd_multi(c.dys, c.x, c.ws, dres, torch.float32), R.ln_bwd_multi(c.dys, c.x, c.ws, dres)
                take('multi.dx', lo[0], hi[0], True)
                for (lw, lb), (hw, hb) in zip(lo[1], hi[1]):
                    take('multi.dw', lw, hw, False)
                    take('multi.db', lb, hb, False)
    return worst


def test_bounds_are_the_measurement():
    got = measured()
    for k in R.BOUND_KEYS:
        print(f'{k}: f32-vs-f64 deviation {got[k]:.3e} -> GPU bound {max(R.TOL_FACTOR * got[k], R.FLOOR):.3e}')
    assert all(0 < v < 1e-5 for v in got.values()), got
    if not os.path.exists(R.BOUNDS_PATH):
        with open(R.BOUNDS_PATH, 'w') as f:
            json.dump({'what': 'max deviation (ln_ref.deviation) of the float32 evaluation of ln_ref\'s formulas from '
                               'the float64 one over the GPU tests\' inputs, measured on the CPU by test_ln_ref.py; '
                               'the GPU bound is max(4 x this, 2^-21)',
                       'f32_vs_f64_deviation': {k: float(f'{got[k]:.3e}') for k in R.BOUND_KEYS}}, f, indent=1)
            f.write('\n')
        R.recorded.cache_clear()
    rec = R.recorded()
    assert set(rec) == set(R.BOUND_KEYS)
    for k in R.BOUND_KEYS:
        assert abs(got[k] / rec[k] - 1.0) <= 0.25, (k, got[k], rec[k])
        assert R.bound(k) == max(4 * rec[k], 2.0 ** -21)
