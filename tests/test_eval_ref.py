"""CPU checks of tests/eval_ref.py, the float64 restatements the fp32-mode and evaluation kernel GPU tests
(test_fp32_kernels_gpu.py, test_eval_kernels_gpu.py) compare against:

* the restatements against oracle/ (itself pinned to the reference's goldens): the GEMM epilogues against F.linear,
  F.gelu and oracle.rotary, attention against oracle.attention, LayerNorm against the oracle's, the per-sequence
  log-probability against the zeroed-column log_softmax of oracle.p_of_x_given_z, the mutual-information log against
  oracle.marginal_kl;
* the recorded f32-vs-f64 deviations (eval_ref.F32_DEV): re-measured here on the GPU tests' own inputs; each constant
  has to lie within a quarter of its measurement;
* for every family one representative mistake, switched on in the float32 restatement: its deviation has to leave
  the bound the GPU test holds the kernel to, so a kernel making it would fail.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import oracle
from oracle import svae_oracle
import eval_ref as R

f64, f32 = torch.float64, torch.float32


# ================================================================================================ ties to the oracle
def test_gemm_epilogues_match_torch_and_oracle_rotary():
    c = R.gemm_case('f32')
    want = F.linear(c['A'].double(), c['W'].double(), c['bias'].double()) + c['resid'].double()
    assert torch.allclose(R.gemm_eval('f32'), want, rtol=1e-13, atol=1e-13)
    c = R.gemm_case('gelu')
    want = F.gelu(F.linear(c['A'].double(), c['W'].double(), c['bias'].double()))
    assert torch.allclose(R.gemm_eval('gelu'), want, rtol=1e-13, atol=1e-14)
    # the engine's form, as test_kernels_gpu.py states it: [B, L, 3d] -> rotary(q) | rotary(k) | v
    c = R.gemm_case('rot_engine')
    d, L = 24, 13
    y = F.linear(c['A'].double(), c['W'].double(), c['bias'].double()).view(2, L, 3 * d)
    want = torch.cat([oracle.rotary(y[..., :d]), oracle.rotary(y[..., d:2 * d]), y[..., 2 * d:]], -1).view(2 * L, 3 * d)
    assert torch.allclose(R.gemm_eval('rot_engine'), want, rtol=1e-13, atol=1e-14)
    # the ragged form: positions wrap at 7, groups of 20 columns, columns 40 .. 60 untouched
    c = R.gemm_case('rot_ragged')
    y = F.linear(c['A'].double(), c['W'].double(), c['bias'].double())
    got = R.gemm_eval('rot_ragged')
    assert torch.equal(got[:, 40:], y[:, 40:])
    for m in (0, 6, 7, 16):
        for c0 in (0, 20):
            want = oracle.rotary(y[m:m + 1, c0:c0 + 20], start=m % 7)
            assert torch.allclose(got[m:m + 1, c0:c0 + 20], want, rtol=1e-13, atol=1e-14), (m, c0)
    # the table form the float32 restatement (and the kernel) evaluates is the same rotation, up to the table's f32
    for name in ('rot_ragged', 'rot_engine'):
        c, (_, _, _, _, ra) = R.gemm_case(name), R.GEMM_CASES[name]
        y = F.linear(c['A'].double(), c['W'].double(), c['bias'].double())
        assert R.deviation(R._rotary_table(y, c['rot'], *ra), R.gemm_eval(name)) < 1e-5
        assert R.deviation(R._rotary_table(y, c['rot'], *ra, flip=True), R.gemm_eval(name)) > 1e-2


def _unrotate(x, max_pos):
    """The inverse of oracle.rotary on [B, L, d]."""
    half = x.shape[-1] // 2
    ang = torch.arange(x.shape[-2], dtype=f64)[:, None] * max_pos ** (-torch.arange(half, dtype=f64) / half)
    c, s = ang.cos(), ang.sin()
    a, b = x[..., 0::2], x[..., 1::2]
    return torch.stack([a * c + b * s, b * c - a * s], -1).flatten(-2)


@pytest.mark.parametrize('name', ['engine', 'cross', 'win1_96', 'win2_100', 'hd130'])
def test_attention_matches_oracle(name):
    """oracle.attention with identity projections; it rotates q and k, so it is handed their inverse rotations."""
    B, H, Lq, Lk, hd, causal, window, _ = R.ATTN_CASES[name]
    c, d = R.attn_case(name), H * hd
    max_pos = 2 * window * 32 if window else 10000
    eye, zero = torch.eye(d, dtype=f64), torch.zeros(d, dtype=f64)
    p = {f'a.{n}.{k}': v for n in ('q_linear', 'k_linear', 'v_linear', 'output_linear')
         for k, v in (('weight', eye), ('bias', zero))}
    q_in, k_in = _unrotate(c['q'].double(), max_pos), _unrotate(c['k'].double(), max_pos)
    assert torch.allclose(oracle.rotary(k_in, max_pos=max_pos), c['k'].double(), atol=1e-13)
    pad = c['pad'].bool() if c['pad'] is not None else None
    want = oracle.attention(p, 'a.', q_in, k_in, c['v'].double(), pad, H, causal, window)
    got = R.attn_eval(name)
    assert got.shape == want.shape == (B, Lq, d)
    assert torch.allclose(got, want, rtol=1e-10, atol=1e-12)


def test_attention_dead_rows_are_the_fully_padded_element():
    for name in R.ATTN_CASES:
        dead = R.attn_dead_rows(name)
        if name == 'allpad':
            assert dead[1].all() and not dead[0].any() and dead.sum().item() == 5
        else:
            assert not dead.any(), name
    B, H, Lq, Lk, hd, *_ = R.ATTN_CASES['engine']
    assert (B * H * Lq) % 4 != 0
    assert bool((R.attn_eval('lk32768').abs() > 0).all())


def test_layernorm_matches_oracle():
    for rows, D in R.LN_SHAPES:
        x, w, b = R.ln_case(rows, D)
        want = svae_oracle._ln({'n.weight': w.double(), 'n.bias': b.double()}, 'n', x.double())
        assert torch.allclose(R.layernorm(x, w, b), want, rtol=1e-12, atol=1e-13), (rows, D)
    x, w, b = R.ln_case(5, 200, 'const')
    assert torch.equal(R.layernorm(x, w, b), b.double().expand(5, 200))
    assert torch.equal(R.layernorm(x, w, b, f32), b.expand(5, 200))      # ... and exactly b in f32 too


@pytest.mark.parametrize('V,nseq,seq', R.CE_CASES)
def test_seq_logprob_matches_the_zeroed_log_softmax(V, nseq, seq):
    c = R.ce_case(V, nseq, seq)
    lab = c['labels'].long()
    lp = c['logits'].log_softmax(-1)
    lp[:, 0] = 0.0                                             # oracle.p_of_x_given_z (continuous_autoencoder.py:85)
    want = lp.gather(1, lab[:, None])[:, 0].view(nseq, seq).sum(-1)
    got = R.seq_logprob(c['logits'], c['labels'], seq)
    assert torch.allclose(got, want, rtol=1e-13, atol=0)
    assert got[1].item() == 0.0 and bool((c['labels'].view(nseq, seq)[1] == 0).all())
    assert got[0].item() < 0 and math.isfinite(got[0].item())
    # the synthetic statistics are those of the logits: the kernel's formula in float64 from them (unrounded)
    part = R.ce_part(c['logits'])
    ll = c['logits'].gather(1, lab[:, None])[:, 0]
    assert torch.allclose(R.seq_logprob_from_part(part, ll, c['labels'], seq, f64), want, rtol=1e-12, atol=0)
    ntile = -(-V // 128)
    assert part.shape == (nseq * seq, ntile, 2)
    gone = (part[..., 0] == -math.inf) & (part[..., 1] == 0)
    assert gone.sum().item() == 1 and bool(gone[0, 1] if ntile > 1 else gone[1, 0])
    assert (c['labels'][0] != 0) and (c['labels'][1] == 0) and 0 < (c['labels'] == 0).sum() < nseq * seq


def test_composite_case_is_the_engines_call_form():
    ref, part = R.composite_eval()
    c = R.composite_case()
    nseq, seq, d, V = R.COMPOSITE
    logits = F.linear(c['hh'].double(), c['W'].double(), c['bias'].double())
    lp = logits.log_softmax(-1)
    lp[:, 0] = 0.0
    assert torch.allclose(ref, lp.gather(1, c['labels'].long()[:, None])[:, 0].view(nseq, seq).sum(-1), rtol=1e-13)
    assert part.shape == (nseq * seq, V // 128, 2) and bool((c['labels'][seq - 1::seq] == 0).all())


@pytest.mark.parametrize('B,Z,S,regime', R.MI_CASES)
def test_mutual_info_matches_oracle_marginal_kl(B, Z, S, regime):
    stats, eps, kl = R.mi_case(B, Z, S, regime)
    mu, lv = stats[:, :Z].double(), stats[:, Z:].double()
    want = kl.double()[0] - oracle.marginal_kl(mu, (0.5 * lv).exp(), eps.double())
    got = R.mutual_info(stats, eps, kl)
    assert abs(got['out'].item() - want.item()) <= 1e-11 * max(1.0, abs(want.item()))
    assert got['marginal'].shape == got['sumsq'].shape == (S * B,)
    if regime == 'spread':          # one posterior carries each logsumexp: the runner-up is e^-50 or less of it
        x = mu + eps.double() * (0.5 * lv).exp()
        logq = (-(x[:, :, None] - mu) ** 2 / (2 * lv.exp()) - 0.5 * lv - 0.5 * R.LOG_2PI).sum(-1)
        top = logq.topk(2, -1).values
        assert (top[..., 0] - top[..., 1]).min().item() > 50


# ================================================================================================ recorded deviations
@functools.lru_cache(maxsize=None)
def measured():
    m = {}
    for name in R.GEMM_CASES:
        m['gemm_' + name] = R.deviation(R.gemm_eval(name, f32), R.gemm_eval(name))
    m['attn'] = m['attn_long'] = 0.0
    for name in R.ATTN_CASES:
        live, key = ~R.attn_dead_rows(name), R.attn_key(name)
        m[key] = max(m[key], R.deviation(R.attn_eval(name, f32)[live], R.attn_eval(name)[live]))
    m['ln'] = max(R.deviation(R.layernorm(*R.ln_case(r, D), f32), R.layernorm(*R.ln_case(r, D)))
                  for r, D in R.LN_SHAPES)
    m['ln_offset'] = max(R.deviation(R.layernorm(*R.ln_case(r, D, 'offset'), f32),
                                     R.layernorm(*R.ln_case(r, D, 'offset')), rows=True) for r, D in R.LN_OFFSET_SHAPES)
    m['seq_logprob'] = 0.0
    for V, nseq, seq in R.CE_CASES:
        c = R.ce_case(V, nseq, seq)
        ref = R.seq_logprob(c['logits'], c['labels'], seq)
        for order in R.SUM_ORDERS:
            got = R.seq_logprob_from_part(c['part'], c['label_logit'], c['labels'], seq, order=order)
            m['seq_logprob'] = max(m['seq_logprob'], R.deviation(got, ref))
    m['composite'] = max(R.deviation(R.composite_eval(f32, order)[0], R.composite_eval()[0]) for order in R.SUM_ORDERS)
    for case in R.MI_CASES:
        lo, hi = R.mutual_info(*R.mi_case(*case), f32), R.mutual_info(*R.mi_case(*case))
        for k in ('out', 'marginal', 'sumsq'):
            key = R.mi_key(case[1], k)
            m[key] = max(m.get(key, 0.0), R.deviation(lo[k], hi[k]))
    return m


@pytest.mark.parametrize('key', sorted(R.F32_DEV))
def test_recorded_deviation_is_the_measurement(key):
    got, const = measured()[key], R.F32_DEV[key]
    print(f'{key}: measured f32-vs-f64 deviation {got:.3e}, recorded {const:.3e}')
    assert abs(got / const - 1.0) <= 0.25, (key, got, const)


def test_every_constant_is_measured():
    assert set(measured()) == set(R.F32_DEV)
    assert math.isclose(R.bound('ln'), 4 * R.F32_DEV['ln'])
    assert math.isclose(R.bound('ln', 1e-3), 4 * R.F32_DEV['ln'] + 1e-3)


# ================================================================================================ would a mistake show?
def _leaves(what, dev, limit):
    print(f'{what}: deviation {dev:.3e} against the bound {limit:.3e}')
    assert not dev <= limit, (what, dev, limit)               # (a NaN has left it too)


def test_a_dropped_k_tail_leaves_the_bound():
    for name in ('f32', 'gelu', 'rot_ragged', 'rot_engine'):   # K % 16 = 8 in all four
        assert R.GEMM_CASES[name][2] % 16 == 8
        _leaves(f'gemm {name}, K tail dropped', R.deviation(R.gemm_eval(name, f32, 'drop_k_tail'), R.gemm_eval(name)),
                R.bound('gemm_' + name))


def test_a_swapped_rotary_sign_leaves_the_bound():
    for name in ('rot_ragged', 'rot_engine'):
        _leaves(f'gemm {name}, rotary sign', R.deviation(R.gemm_eval(name, f32, 'rot_sign'), R.gemm_eval(name)),
                R.bound('gemm_' + name))


def test_a_causal_mask_off_by_one_leaves_the_bound():
    for name in ('engine', 'hd96', 'win2_100'):
        dev = R.deviation(R.attn_eval(name, f32, 'causal_ge'), R.attn_eval(name))
        _leaves(f'attention {name}, j >= qi masked', dev, R.bound(R.attn_key(name)))


def test_a_one_pass_variance_leaves_the_bound():
    for r, D in R.LN_OFFSET_SHAPES:
        x, w, b = R.ln_case(r, D, 'offset')
        dev = R.deviation(R.layernorm(x, w, b, f32, 'one_pass'), R.layernorm(x, w, b), rows=True)
        _leaves(f'layernorm {r}x{D}, one-pass variance', dev, R.bound('ln_offset'))


@pytest.mark.parametrize('V,nseq,seq', R.CE_CASES)
def test_counting_label0_rows_leaves_the_bound(V, nseq, seq):
    c = R.ce_case(V, nseq, seq)
    ref = R.seq_logprob(c['logits'], c['labels'], seq)
    got = R.seq_logprob_from_part(c['part'], c['label_logit'], c['labels'], seq, mutate='count_label0')
    intr = R.ce_intrinsic(c['part'], c['labels'], seq, ref)
    assert intr < R.bound('seq_logprob')                       # the intrinsics' allowance does not carry the bound
    _leaves(f'seq_logprob V={V}, label-0 rows counted', R.deviation(got, ref), R.bound('seq_logprob', intr))


@pytest.mark.parametrize('B,Z,S,regime', [c for c in R.MI_CASES if c[0] > 1])
def test_an_omitted_log_b_leaves_the_bound(B, Z, S, regime):
    stats, eps, kl = R.mi_case(B, Z, S, regime)
    ref = R.mutual_info(stats, eps, kl)
    got = R.mutual_info(stats, eps, kl, f32, 'no_log_b')
    intr = R.mi_intrinsic(stats, eps, ref)
    for k in ('out', 'marginal'):
        _leaves(f'mutual_info {B}x{Z}x{S} {regime} {k}, no -log B', R.deviation(got[k], ref[k]),
                R.bound('mi_' + k, intr[k]))
    # a 1 % error in Z log 2 pi, the other term the issue names, leaves it as well
    off = 0.01 * 0.5 * Z * R.LOG_2PI / (2 * abs(ref['out'].item()))
    _leaves(f'mutual_info {B}x{Z}x{S} {regime} out, Z log 2 pi off by 1 %', off,
            R.bound(R.mi_key(Z, 'out'), intr['out']))
