"""Plain float64 restatements of the epilogues of csrc/gemm.hip's svae_gemm (BF16, F32 with bias / residual / the
dropout-masked bf16 copy, F32_ACC, F32_ATOMIC, GELU, GELU_BWD, DROPOUT_RESID, ROTARY_BF16, CE_STATS, the BF16 delta),
of gemm_run's choice among its four kernels (route), the inputs the GPU tests feed them, the case lists and the error
bounds those tests hold them to. Every formula is the operation's definition, not the kernel's code, and takes a
`dtype`: float64 is the reference, float32 the same formula at the kernels' precision with the K sum taken in the
reverse order (test_gemm_ref.py measures the distance between the two on the GPU tests' own inputs and records it in
tests/golden/gemm_bounds.json; the bounds are built from that record). The error measure divides every element's
error by its own scale S = |alpha| |A| |B| + |bias| + |resid| (what a rounding of the sum's terms is proportional
to), so one wrong element is one large term of the max and nothing is averaged or excluded. The tensors stay on the
device they came on. Nothing in this file runs product code."""
import functools
import json
import math
import os

import torch

import ln_ref
from ln_ref import dropout_scale

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'gemm_bounds.json')
SEED = 0x243F6A8885A308D3                                   # the dropout seed of every case (above 2^32)


# ---------------------------------------------------------------------------------------------- error measure
def deviation(got, ref, S):
    """-> (max over elements of |got - ref| / S, index of the worst element). A NaN anywhere in got is inf."""
    err = (got.double() - ref.double()).abs() / S.double().clamp_min(1e-300)
    err = torch.where(torch.isnan(err), torch.full_like(err, math.inf), err)
    flat = int(err.reshape(-1).argmax().item())
    idx = []
    for n in reversed(err.shape):
        idx.append(flat % n)
        flat //= n
    return err.max().item(), tuple(reversed(idx))


def bf16_excess(got, ref, bound_f32, S, extra=0.0):
    """ln_ref.bf16_excess with the element's own scale S in the place of rms_row + |ref|: max over elements of
    |got - ref| / (2^-8 |ref| + bound_f32 S + extra); within bound when <= 1. 2^-8 is bf16's unit roundoff, the
    second term the f32 error of the value that is rounded, `extra` an absolute allowance per element (a tensor or a
    number: the A-S GELU's gap). -> (excess, index of the worst element)."""
    ref = ref.double()
    allow = 2.0 ** -8 * ref.abs() + bound_f32 * S.double() + extra
    return deviation(got, ref, allow)


# ---------------------------------------------------------------------------------------------- the product
def acc(A, W, alpha=1.0, dtype=f64):
    """alpha A . W^T for A [.., M, K], W [.., N, K] (B = W^T). float32: the K sum runs in the reverse order."""
    if dtype == f64:
        return alpha * (A.double() @ W.double().transpose(-1, -2))
    return (A.float().flip(-1) @ W.float().flip(-1).transpose(-1, -2)) * torch.tensor(alpha, dtype=f32)


def gemm(A, W, alpha=1.0, bias=None, resid=None):
    """-> (alpha A . B in float64, S = |alpha| |A| . |B| + |bias| + |resid|), B = W^T."""
    S = abs(alpha) * (A.double().abs() @ W.double().abs().transpose(-1, -2))
    if bias is not None:
        S = S + bias.double().abs()
    if resid is not None:
        S = S + resid.double().abs()
    return acc(A, W, alpha), S


# ---------------------------------------------------------------------------------------------- the epilogues
def epi_f32(x, bias=None, resid=None):
    """F32 (and the value BF16 rounds): acc + bias + resid, each when given."""
    if bias is not None:
        x = x + bias.to(x.dtype)
    if resid is not None:
        x = x + resid.to(x.dtype)
    return x


def epi_bf16(x, bias=None):
    return epi_f32(x, bias)


def epi_f32_acc(x, c0):
    """F32_ACC: C += acc."""
    return c0.to(x.dtype) + x


def epi_f32_atomic(x, c0):
    """F32_ATOMIC: C += the sum of the K slices' products = acc."""
    return c0.to(x.dtype) + x


_SQRT1_2, _INV_SQRT_2PI = 0.7071067811865476, 0.3989422804014327


def gelu_erf(x):
    """-> (gelu(x), gelu'(x)) = (x Phi(x), Phi(x) + x phi(x)), Phi from the exact erf."""
    cdf = 0.5 * (1.0 + torch.special.erf(x * _SQRT1_2))
    pdf = _INV_SQRT_2PI * torch.exp(-0.5 * x * x)
    return x * cdf, cdf + x * pdf


def gelu_as(x):
    """The same with Phi(-|x|) = erfc(|x| / sqrt 2) / 2 by Abramowitz-Stegun 7.1.26, the form of common.h's
    gelu_pair (|erf error| <= 1.5e-7 by the handbook)."""
    z = x.abs() * _SQRT1_2
    t = 1.0 / (1.0 + 0.3275911 * z)
    poly = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429))))
    e = torch.exp(-z * z)
    half_erfc = 0.5 * poly * e
    cdf = torch.where(x >= 0, 1.0 - half_erfc, half_erfc)
    return x * cdf, cdf + x * _INV_SQRT_2PI * e


def epi_gelu(x, bias=None, form=gelu_erf):
    """GELU: -> (C, aux) = (gelu, gelu') of acc + bias."""
    return form(epi_f32(x, bias))


def epi_gelu_bwd(x, gp):
    """GELU_BWD: acc times the stored gelu'."""
    return x * gp.to(x.dtype)


def dropout_keep(M, N, p, seed):
    """-> bool [M, N] (CPU): the mask of rand_uniform4 at counter (m N + n) >> 2 (ln_ref's generator, not a second
    one)."""
    return ln_ref.dropout_keep(seed, M, N, p)


def epi_dropout_resid(x, resid, keep, p):
    """DROPOUT_RESID: keep acc / (1 - p) + resid, the scale as float32 forms it."""
    sc = torch.tensor(dropout_scale(p), dtype=x.dtype)
    return torch.where(keep, x * sc, torch.zeros_like(x)) + resid.to(x.dtype)


def epi_f32_copy(c, keep, p):
    """F32's aux: keep C / (1 - p) (its bf16 is what svae_dropout_bwd_cast makes of C)."""
    sc = torch.tensor(dropout_scale(p), dtype=c.dtype)
    return torch.where(keep, c * sc, torch.zeros_like(c))


def epi_rotary(x, tab, rot_cols, rot_d, rot_seq, S=None):
    """ROTARY_BF16: columns n < rot_cols rotate in pairs (2i, 2i+1) of each rot_d-wide block by the table's
    (cos, sin)[m % rot_seq][i], (a, b) -> (a c - b s, b c + a s); columns n >= rot_cols pass. tab [rot_seq, rot_d / 2,
    2]. S given: -> (out, S'), the rotated pair's scale S_a |c| + S_b |s| (S_b |c| + S_a |s|)."""
    M = x.shape[-2]
    nblk = rot_cols // rot_d
    pos = torch.arange(M, device=x.device) % rot_seq
    cs = tab.to(device=x.device, dtype=x.dtype)[pos]                     # [M, rot_d / 2, 2]
    c, s = cs[..., 0][:, None, :], cs[..., 1][:, None, :]                # [M, 1, rot_d / 2]

    def turn(v, c, s, sign):
        r = v[..., :rot_cols].reshape(M, nblk, rot_d // 2, 2)
        a, b = r[..., 0], r[..., 1]
        o = torch.stack([a * c + sign * b * s, b * c + a * s], -1).reshape(M, rot_cols)
        return torch.cat([o, v[..., rot_cols:]], -1)

    out = turn(x, c, s, -1.0)
    if S is None:
        return out
    return out, turn(S.to(x.dtype), c.abs(), s.abs(), 1.0)


def ce_stats(logits, labels):
    """CE_STATS: -> (logsumexp per row, the label's logit per row); the logits themselves are acc + bias."""
    return torch.logsumexp(logits, -1), logits.gather(-1, labels.long()[:, None])[:, 0]


def ce_lse_from_partials(part):
    """The row's logsumexp from the kernel's partials [T, tiles, 2] = (max, sum exp(x - max)) per 128-column tile."""
    return torch.logsumexp(part[..., 0].double() + part[..., 1].double().log(), -1)


def delta(cb, o32, hd, seq, dtype=f64, absolute=False):
    """The BF16 delta: per (row, head) the sum over the head's hd columns of bf16(C) o32, laid out
    [(b H + h) seq + q] for row m = b seq + q. absolute: the sum of the terms' magnitudes (its scale)."""
    M, Nn = cb.shape
    t = cb.to(dtype) * o32.to(dtype)
    if absolute:
        t = t.abs()
    t = t.view(M // seq, seq, Nn // hd, hd)
    if dtype == f32:
        t = t.flip(-1)                                      # (the float32 sum in the reverse order)
    return t.sum(-1).permute(0, 2, 1).reshape(-1)


# ---------------------------------------------------------------------------------------------- gemm_run's choice
SKINNY_EPIS = ('BF16', 'F32', 'GELU', 'GELU_BWD', 'DROPOUT_RESID')
P_HEAD_EPIS = ('CE_PROB', 'ROWSCALE_GATHER')


def route(M, N, K, a_t=0, b_t=0, epi='BF16', splits=1, batch=1, slab=False, k_weight=False, n_cu=256, a_rowsum=False):
    """-> ('skinny' | 'g128' | 'glds' | 'g256', tiles, persistent): the kernel gemm_run launches for a valid
    descriptor, the tiles (x batch x splits) it works on and whether gemm256's blocks walk more than one."""
    cdiv = lambda a, b: -(-a // b)
    if (M <= 64 and not a_t and not b_t and batch == 1 and splits == 1 and not a_rowsum and K % 8 == 0
            and epi in SKINNY_EPIS):
        return 'skinny', cdiv(N, 32), False
    kslice = cdiv(K, splits)
    blocks256 = cdiv(N, 256) * cdiv(M, 256) * batch * splits
    acc_epi = epi == 'F32_ACC'
    ok3 = not (a_t and not b_t) or acc_epi
    small = 'glds' if (kslice <= 2048 and not (a_t and b_t)) else 'g128'
    impl = 'g256' if (ok3 and blocks256 >= 192) else small
    if epi in P_HEAD_EPIS or k_weight:
        impl = 'g256' if ok3 else 'g128'
    epi_run = 'F32' if (epi == 'F32_ATOMIC' and splits > 1 and slab) else epi
    if impl == 'g256' and epi_run == 'F32_ATOMIC':
        impl = small
    if impl == 'g256':
        return impl, blocks256, blocks256 > n_cu
    return impl, cdiv(N, 128) * cdiv(M, 128) * batch * splits, False


# ---------------------------------------------------------------------------------------------- inputs
class Case:
    pass


def _mod_plane(M, N, a, b, mod):
    return ((torch.arange(M)[:, None] * a + torch.arange(N)[None, :] * b) % mod).float()


@functools.lru_cache(maxsize=2)
def inputs(M, N, K, a_t=0, b_t=0, batch=1):
    """The GPU tests' inputs (drawn on the CPU: the same on every device), logical A [M, K] and W [N, K] (B = W^T; a
    leading batch dimension when batch > 1) and their stored forms As ([K, M] when a_t), Bs ([K, N] when b_t):
      A bf16 N(0, 1), W bf16 0.1 N(0, 1); Ai, Wi integers in {-2 .. 2} (every f32 sum of products is exact);
      bias[n] = n / 8 + 0.05 N(0, 1): a column group off is off by >= 0.5, a 128-tile by 16;
      bias_mod[n] = ((37 n) % 101) / 25 - 2 + 0.02 N(0, 1): visibly different per column (4 columns off differ by
        1.9, 8 by 0.28, 128 by 0.44) but within [-2, 2], for
        the epilogues whose interesting range is small (GELU) or that sum exponentials over the row (CE_STATS);
      resid[m, n] = ((37 m + 11 n) % 101) / 25 - 2 + 0.1 N(0, 1): one row off is off by ~1.5, 4 columns by ~1.8;
      gp[m, n] bf16 = ((13 m + 7 n) % 23) / 20 - 0.1 in [-0.1, 1.0] (a GELU'): one row or 4 / 8 columns off differ
        by >= 0.25;
      c0[m, n] = (3 m + 5 n) % 7 - 3: the non-constant integer C that F32_ACC / F32_ATOMIC add onto."""
    gen = torch.Generator().manual_seed(1000003 * M + 1009 * N + 17 * K + 5 * batch + 2 * a_t + b_t)
    lead = (batch,) if batch > 1 else ()
    c = Case()
    c.M, c.N, c.K, c.a_t, c.b_t, c.batch = M, N, K, a_t, b_t, batch
    c.A = torch.randn(*lead, M, K, generator=gen).to(bf16)
    c.W = (0.1 * torch.randn(*lead, N, K, generator=gen)).to(bf16)
    c.Ai = torch.randint(-2, 3, (*lead, M, K), generator=gen).to(bf16)
    c.Wi = torch.randint(-2, 3, (*lead, N, K), generator=gen).to(bf16)
    c.bias = torch.arange(N).float() / 8 + 0.05 * torch.randn(N, generator=gen)
    c.bias_mod = (torch.arange(N) * 37 % 101).float() / 25 - 2 + 0.02 * torch.randn(N, generator=gen)
    c.resid = _mod_plane(M, N, 37, 11, 101) / 25 - 2 + 0.1 * torch.randn(M, N, generator=gen)
    c.gp = (_mod_plane(M, N, 13, 7, 23) / 20 - 0.1).to(bf16)
    c.c0 = _mod_plane(M, N, 3, 5, 7) - 3
    return c


def stored(c, integer=False):
    """-> (As, Bs): the operands in the layout the descriptor names."""
    A, W = (c.Ai, c.Wi) if integer else (c.A, c.W)
    return (A.transpose(-1, -2).contiguous() if c.a_t else A), (W.transpose(-1, -2).contiguous() if c.b_t else W)


def ce_labels(T, V):
    """Labels at the places a tiled search for the label's column can miss: the last valid column, every column of
    the last 4-column group, column 0, both sides of the 64- / 128- / 256-column boundaries, then a fixed spread."""
    edge = [V - 1, V - 2, V - 3, V - 4, V - 5, 0, 1, 63, 64, 127, 128, 255, 256, V - V % 256 - 1, V - V % 256,
            V - V % 128 - 1, V - V % 128]
    assert T >= 2 * len(edge) and all(0 <= e < V for e in edge)
    lab = [(7919 * i + 13) % V for i in range(T)]
    lab[:len(edge)] = edge
    lab[T - len(edge):] = edge[::-1]                        # and in the last rows (the ragged last tile row)
    return torch.tensor(lab, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------- the case lists
# (M, N, K, a_t, b_t): the smallest shapes at which each kernel's loops and edges are live
SKINNY = ((1, 36, 8, 0, 0),            # one k-step, wave 0 alone works, the second block has 4 valid columns
          (37, 100, 72, 0, 0),         # 3 k-steps, 13 idle waves, the last k-step a quarter valid
          (64, 64, 1056, 0, 0))        # 33 k-steps, 3 per wave, waves 11-15 empty
# K 8 / 72 / 200: shorter than the 3-stage pipeline of BK 32, 3 K-tiles with a tail, 7 with a tail
GLDS = tuple((136, 136 if b_t else 132, k, a_t, b_t) for a_t, b_t in ((0, 0), (0, 1), (1, 0)) for k in (8, 72, 200)) + (
    (384, 868, 72, 0, 0),)             # 3 x 7 = 21 blocks: the XCD remap with remainder 5
G128 = tuple((136, 136, k, 1, 1) for k in (71, 72, 200)) + ((136, 132, 2056, 0, 0), (384, 868, 2056, 0, 0))
G256 = ((12100, 1004, 72, 0, 0),       # 48 x 4 = 192 tiles, last tile row 68 rows, last column tile ends in 4 columns
        (12100, 1004, 200, 0, 0))
G256_PERSISTENT = ((16420, 1004, 72, 0, 0),)     # 65 x 4 = 260 tiles on 256 CUs: four blocks take a second tile
G256_WIDE = ((1540, 8196, 72, 0, 0),)            # 7 x 33 = 231 tiles, group = 4: a band of 4 tile rows, then of 3
ROUTES = (('skinny', SKINNY), ('glds', GLDS), ('g128', G128), ('g256', G256 + G256_PERSISTENT + G256_WIDE))
REAL_CASES = tuple((r,) + s for r, shapes in ROUTES for s in shapes)
INT_CASES = (('skinny',) + SKINNY[1], ('glds',) + GLDS[2], ('glds',) + GLDS[-1], ('g128',) + G128[2],
             ('g128',) + G128[4], ('g256',) + G256[0], ('g256',) + G256_PERSISTENT[0], ('g256',) + G256_WIDE[0])
DROP_P = (0.0, 0.25)                   # DROPOUT_RESID
COPY_P = (0.0, 0.1)                    # F32 + aux
# (route, M, N, K, a_t, b_t, rot_d, rot_cols, rot_seq)
ROTARY_CASES = (('glds', 200, 408, 72, 0, 0, 136, 272, 40), ('glds', 200, 408, 72, 0, 0, 136, 272, 5),
                ('g128', 200, 408, 72, 1, 1, 136, 272, 40),
                ('g256', 12100, 1020, 136, 0, 0, 340, 680, 40), ('g256', 12100, 1020, 136, 0, 0, 340, 680, 5),
                ('g256', 16420, 1020, 136, 0, 0, 340, 680, 40))
# (route, T, V, K, tiles, persistent at 256 CUs)
CE_CASES = (('g256', 300, 24580, 72, 194, False), ('g256', 700, 24580, 72, 291, True), ('glds', 300, 1156, 72, 30, False))
# (route, M, N, K, hd, seq)
DELTA_CASES = (('g256', 16140, 768, 72, 64, 20), ('g256', 16140, 768, 72, 96, 20), ('g256', 21780, 768, 72, 64, 20),
               ('g256', 21780, 768, 72, 96, 20), ('skinny', 60, 64, 72, 16, 20), ('glds', 140, 144, 72, 16, 20))
BATCH_CASES = (('g256', 512, 512, 72, 48), ('glds', 136, 136, 72, 3), ('g128', 136, 136, 2056, 3))
ATOMIC_SHAPE = (136, 136, 200)         # splits 3: glds slices 96 + 96 + 8, g128 slices 128 + 72 + an empty one
SLAB_G256 = (1032, 520, 824, 13)       # 5 x 3 tiles x 13 splits = 195 blocks of gemm256, the last slice 56 deep


# ---------------------------------------------------------------------------------------------- bounds
TOL_FACTOR = 4.0
FLOOR = 2.0 ** -21       # four float32 ulps: the device's rcp / exp2 / log2 and fused multiply-adds
BOUND_KEYS = ('acc', 'f32', 'gelu.g', 'gelu.gp', 'gelu_bwd', 'dropout', 'rotary', 'ce.logit', 'ce.lse', 'delta')


@functools.lru_cache(maxsize=None)
def _record():
    with open(BOUNDS_PATH) as f:
        return json.load(f)


def recorded():
    """The f32-vs-f64 deviations test_gemm_ref.py measured and wrote (tests/golden/gemm_bounds.json)."""
    return _record()['f32_vs_f64_deviation']


def as_gap():
    """The recorded max |Phi_AS - Phi_erf| of the float64 A-S form: g may differ by this times |x|, g' by this."""
    return _record()['gelu_as_vs_erf_gap']


def bound(key):
    """What an f32 value is held to on the GPU: 4 x the recorded deviation of the same formula, never below FLOOR."""
    return max(TOL_FACTOR * recorded()[key], FLOOR)
