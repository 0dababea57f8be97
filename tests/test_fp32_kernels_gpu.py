"""The fp32 kernel mode of csrc/fp32.hip one kernel at a time (svae_gemm_f32, svae_attn_fwd_f32,
svae_layernorm_fwd_f32), against the float64 restatements of tests/eval_ref.py, at the shapes the engine never sends:
a K tail, odd N, ragged 64x64 tiles, padded leading dimensions, a rotary boundary inside a tile, head dimensions
above 64, idle waves, Lq != Lk and the 2-wave / 1-wave attention instances above 8192 / 16384 keys. The bounds are
eval_ref's: 4 x the f32-vs-f64 deviation of the same formulas on these inputs, measured on the CPU by
test_eval_ref.py. Every output lies in a sentinel buffer; operands with a padded leading dimension carry 1e4 in the
padding, so a walk with the wrong stride shows."""
import pytest
import torch

import eval_ref as R
from sentinels import SENTINEL, dev, flat, g, intact, matrix, report

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae import _native as N

f32 = torch.float32


def padded(t, ld):
    """A device copy of the 2-D `t` with leading dimension ld; the padding holds 1e4."""
    wide = torch.full((t.shape[0], ld), 1.0e4, dtype=t.dtype, device=dev)
    wide[:, :t.shape[1]] = t.to(dev)
    return wide[:, :t.shape[1]]


# ================================================================================================ gemm_f32, exact
@pytest.mark.parametrize('epilogue', ['plain', 'bias', 'resid', 'bias_resid'])
@pytest.mark.parametrize('M,Nn,Kk', R.GEMM_EXACT)
def test_gemm_f32_exact_on_integers(M, Nn, Kk, epilogue):
    """Integer operands: the result is exact in f32 in any order, so it is compared bit for bit. (1, 1, 1): one
    element of one tile; (65, 127, 17): a second row tile of one row, odd N (the last column pair has no partner),
    a K tail of 1; (64, 64, 16): exactly one tile and one K step; (130, 200, 72): three row tiles, four column tiles
    (the last 8 wide), a K tail of 8, every leading dimension padded by a different amount; (5, 130, 64): the
    z-projection form (engine.reconstruct_f32), rows scattered ldc = 7 N apart."""
    A, W, bias, resid = R.gemm_int_case(M, Nn, Kk)
    want = A.double() @ W.double().t()
    if 'bias' in epilogue:
        want = want + bias.double()
    if 'resid' in epilogue:
        want = want + resid.double()
    assert want.abs().max().item() < 2 ** 24
    strided = (M, Nn, Kk) == (130, 200, 72)
    scatter = (M, Nn, Kk) == (5, 130, 64)
    lda, ldw, ldc, ldr = (Kk + 5, Kk + 9, Nn + 3, Nn + 7) if strided else (Kk, Kk, Nn, Nn)
    rows = 7 * (M - 1) + 1 if scatter else M
    full, C = matrix(rows, Nn, ldc, f32)
    K.gemm_f32(padded(A, lda), padded(W, ldw), C, M, Nn, Kk, lda=lda, ldw=ldw, ldc=7 * Nn if scatter else ldc,
               bias=g(bias) if 'bias' in epilogue else None, resid=padded(resid, ldr) if 'resid' in epilogue else None,
               ldr=ldr if 'resid' in epilogue else 0)
    torch.cuda.synchronize()
    assert intact(full, rows, Nn)
    got = C.cpu()
    if scatter:
        between = torch.ones(rows, dtype=torch.bool)
        between[::7] = False
        assert bool((got[between] == SENTINEL).all())            # the rows in between keep their sentinel
        got = got[::7]
    assert torch.equal(got.double(), want)


# ================================================================================================ gemm_f32, numeric
@pytest.mark.parametrize('name', list(R.GEMM_CASES))
def test_gemm_f32_against_float64(name):
    """'f32' (70, 66, 1032): 64 K steps and a tail of 8, bias and residual; 'gelu' (37, 61, 72): erf GELU, odd N;
    'rot_ragged' (17, 61, 40), rot_cols 40, rot_d 20, rot_seq 7: rows wrap the table, the rotation ends inside the
    tile, columns 40 .. 60 pass through; 'rot_engine': N = 3d, rot_cols = 2d, rot_d = d = 24, M = 2 x 13."""
    M, Nn, Kk, epi, rot_args = R.GEMM_CASES[name]
    c = R.gemm_case(name)
    ref = R.gemm_eval(name)
    full, C = matrix(M, Nn, Nn + 3, f32)
    kw = {}
    if rot_args:
        kw = dict(rot=g(c['rot']), rot_cols=rot_args[0], rot_d=rot_args[1], rot_seq=rot_args[2])
    K.gemm_f32(g(c['A']), g(c['W']), C, M, Nn, Kk, ldc=Nn + 3, bias=g(c['bias']),
               resid=g(c['resid']) if c['resid'] is not None else None, ldr=Nn if c['resid'] is not None else 0,
               epi={'f32': N.EPI_F32, 'gelu': N.EPI_GELU, 'rotary': N.EPI_ROTARY_BF16}[epi], **kw)
    torch.cuda.synchronize()
    assert intact(full, M, Nn)
    got = C.cpu()
    if name == 'rot_ragged':                                      # past rot_cols: the plain product, not rotated
        report('gemm_f32 rot_ragged, columns past rot_cols', R.deviation(got[:, 40:], ref[:, 40:]),
               R.bound('gemm_' + name))
    report(f'gemm_f32 {name}', R.deviation(got, ref), R.bound('gemm_' + name))


@pytest.mark.parametrize('what', ['epilogue', 'odd_rot_cols', 'no_table'])
def test_gemm_f32_rejects(what):
    M, Nn, Kk = 17, 61, 40
    c = R.gemm_case('rot_ragged')
    full, C = matrix(M, Nn, Nn, f32)
    kw = {'epilogue': dict(epi=N.EPI_BF16),
          'odd_rot_cols': dict(epi=N.EPI_ROTARY_BF16, rot=g(c['rot']), rot_cols=39, rot_d=20, rot_seq=7),
          'no_table': dict(epi=N.EPI_ROTARY_BF16, rot=None, rot_cols=40, rot_d=20, rot_seq=7)}[what]
    with pytest.raises(RuntimeError, match='svae_gemm_f32 failed with status'):
        K.gemm_f32(g(c['A']), g(c['W']), C, M, Nn, Kk, bias=g(c['bias']), **kw)
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all())


# ================================================================================================ attn_fwd_f32
def _attention(name, form):
    """form 'packed': the engine's (reconstruct_f32): q | k | v rows of one [B L, 3d] matrix, o [B L, d]. 'separate':
    q, k, v, o each with a leading dimension of its own (d + 3, d + 5, d + 7, d + 2), 1e4 in the padding."""
    B, H, Lq, Lk, hd, causal, window, _ = R.ATTN_CASES[name]
    c, d = R.attn_case(name), H * hd
    pad = g(c['pad']) if c['pad'] is not None else None
    if form == 'packed':
        assert Lq == Lk
        qkv = g(torch.cat([c['q'], c['k'], c['v']], -1).view(B * Lq, 3 * d).contiguous())
        full, o = matrix(B * Lq, d, d, f32)
        K.attention_f32(qkv, qkv[:, d:], qkv[:, 2 * d:], o, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd, sq=3 * d, sk=3 * d,
                        sv=3 * d, so=d, bq=Lq * 3 * d, bk=Lk * 3 * d, bv=Lk * 3 * d, bo=Lq * d, key_pad=pad,
                        causal=causal, window=window)
    else:
        lq, lk, lv, lo = d + 3, d + 5, d + 7, d + 2
        q, k, v = padded(c['q'].view(-1, d), lq), padded(c['k'].view(-1, d), lk), padded(c['v'].view(-1, d), lv)
        full, o = matrix(B * Lq, d, lo, f32)
        K.attention_f32(q, k, v, o, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd, sq=lq, sk=lk, sv=lv, so=lo, bq=Lq * lq, bk=Lk * lk,
                        bv=Lk * lv, bo=Lq * lo, key_pad=pad, causal=causal, window=window)
    torch.cuda.synchronize()
    assert intact(full, B * Lq, d)
    return o.cpu().reshape(B, Lq, d)


@pytest.mark.parametrize('name,form', [('engine', 'packed'), ('engine', 'separate'), ('hd96', 'packed'),
                                       ('hd130', 'separate'), ('cross', 'separate'), ('win1_96', 'packed'),
                                       ('win2_96', 'packed'), ('win2_100', 'separate')])
def test_attention_f32_against_float64(name, form):
    """'engine': B H L = 2 x 3 x 37 = 222 queries, two idle waves in the last block, causal, suffix padding, hd 20;
    'hd96' / 'hd130': the output loop's second and third trip; 'cross': Lq 5, Lk 70, padded keys, not causal; 'win*':
    the block-sparse band + [CLS] block of oracle.sparse_mask at window 1 and 2, and at L = 100 its L % 32 != 0
    branch."""
    got = _attention(name, form)
    report(f'attention_f32 {name} {form}', R.deviation(got, R.attn_eval(name)), R.bound(R.attn_key(name)))


@pytest.mark.parametrize('name', R.ATTN_LONG)
def test_attention_f32_key_count_switch(name):
    """<= 8192 keys: 4 waves (queries) per block; <= 16384: 2 ('lk8193_q5': 5 queries, so the last block has an idle
    wave); beyond, up to 32768: 1. Each instance at its first and last key count."""
    got = _attention(name, 'separate')
    report(f'attention_f32 {name}', R.deviation(got, R.attn_eval(name)), R.bound(R.attn_key(name)))


def test_attention_f32_fully_padded_batch_element():
    """Every key of batch element 1 is padded: all its scores carry the -1e7 shift, which rounds them to whole
    numbers in f32, so those rows are not compared with float64; they must be finite and a convex combination of the
    v rows (each component within that component's range over the keys). Every other row is compared as usual."""
    name = 'allpad'
    B, H, Lq, Lk, hd, *_ = R.ATTN_CASES[name]
    got, ref, dead = _attention(name, 'separate'), R.attn_eval(name), R.attn_dead_rows(name)
    assert dead.sum().item() == Lq and bool(dead[1].all())        # the rows constructed, and no others
    v = R.attn_case(name)['v']
    lo, hi = v.min(1, keepdim=True).values, v.max(1, keepdim=True).values          # [B, 1, d]
    inside = (got >= lo) & (got <= hi)
    assert bool(torch.isfinite(got[dead]).all()) and bool(inside[dead].all())
    report('attention_f32 allpad, live rows', R.deviation(got[~dead], ref[~dead]), R.bound('attn'))


@pytest.mark.parametrize('what', ['window_without_causal', 'too_many_keys'])
def test_attention_f32_rejects(what):
    B, H, Lq, hd = 1, 1, 3, 8
    Lk, kw = (96, dict(causal=False, window=2)) if what == 'window_without_causal' else (R.ATTN_MAX_KEYS + 1, {})
    Lq = Lk if what == 'window_without_causal' else Lq
    q, k, v = torch.zeros(Lq, hd, device=dev), torch.zeros(Lk, hd, device=dev), torch.zeros(Lk, hd, device=dev)
    full, o = matrix(Lq, hd, hd, f32)
    with pytest.raises(RuntimeError, match='svae_attn_fwd_f32 failed with status'):
        K.attention_f32(q, k, v, o, B=B, H=H, Lq=Lq, Lk=Lk, hd=hd, sq=hd, sk=hd, sv=hd, so=hd, bq=Lq * hd, bk=Lk * hd,
                        bv=Lk * hd, bo=Lq * hd, **kw)
    torch.cuda.synchronize()
    assert bool((full == SENTINEL).all())


# ================================================================================================ layernorm_fwd_f32
def _layernorm(x, w, b):
    rows, D = x.shape
    full, y = flat(rows * D)
    K.layernorm_fwd_f32(g(x), g(w), g(b), y, rows, D)
    torch.cuda.synchronize()
    assert intact(full)
    return y.cpu().reshape(rows, D)


@pytest.mark.parametrize('rows,D', R.LN_SHAPES)
def test_layernorm_f32_against_float64(rows, D):
    """rows 1, 5, 7: the last block has one, one and three live waves of its four (5 and 7: it is the second block);
    D 1 and 20: idle lanes; 64: one trip; 200 and 768: a ragged fourth trip and twelve whole ones."""
    x, w, b = R.ln_case(rows, D)
    report(f'layernorm_f32 {rows}x{D}', R.deviation(_layernorm(x, w, b), R.layernorm(x, w, b)), R.bound('ln'))


@pytest.mark.parametrize('rows,D', R.LN_OFFSET_SHAPES)
def test_layernorm_f32_large_mean_small_spread(rows, D):
    """x = 1000 + 1e-2 N(0, 1): the variance is 1e-10 of the mean's square; E x^2 - (E x)^2 in f32 has nothing left."""
    x, w, b = R.ln_case(rows, D, 'offset')
    report(f'layernorm_f32 {rows}x{D} offset', R.deviation(_layernorm(x, w, b), R.layernorm(x, w, b), rows=True),
           R.bound('ln_offset'))


@pytest.mark.parametrize('rows,D', [(1, 1), (5, 200), (7, 768)])
def test_layernorm_f32_constant_rows_give_the_bias(rows, D):
    """Rows of one value (values whose D-fold sum is exact in f32 in any order): x - mean is 0, so y is b exactly."""
    x, w, b = R.ln_case(rows, D, 'const')
    assert torch.equal(_layernorm(x, w, b), b.expand(rows, D))
