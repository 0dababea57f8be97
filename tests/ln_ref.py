"""Plain torch / numpy restatements of the LayerNorm kernels of csrc/layernorm.hip (svae_layernorm_fwd / _fwd_multi,
svae_layernorm_bwd / _bwd_drop / _bwd_gelu / _bwd_multi), of the dropout mask every kernel draws from
common.h's rand_uniform4, and of the launchers' row plans; the inputs the GPU tests feed the kernels, the case lists
and the error bounds those tests hold them to. Every formula takes a `dtype`: float64 is the reference, float32 the
same formulas at the kernels' precision (test_ln_ref.py measures the distance between the two on the GPU tests' own
inputs and records it in tests/golden/ln_bounds.json; the bounds are built from that record). The tensors stay on the
device they came on. Nothing in this file runs product code."""
import functools
import json
import os

import numpy as np
import torch

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16
EPS = 1e-5
LN_MULTI_MAX = 4                  # SVAE_LN_MULTI_MAX (include/svae.h); test_ln_ref.py checks it against the header
COLSUM_MAX = 8                    # SVAE_COLSUM_MAX
BOUNDS_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'ln_bounds.json')


# ---------------------------------------------------------------------------------------------- error measure
def deviation(got, ref, rows=True):
    """max over elements of |got - ref| / (rms(ref) + |ref|) (optim_ref.deviation): relative where the reference is
    of its typical size, absolute in units of that size where it cancels. rows: the rms is taken per row of a 2-D
    tensor, so every row is held to its own size; otherwise over the whole tensor (a vector of per-row statistics or
    of per-column gradients). One wrong element is one large term of the max: nothing is averaged."""
    got, ref = got.double(), ref.double()
    if not rows or ref.dim() < 2:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    atol = ref.pow(2).mean(-1, keepdim=True).sqrt()
    return ((got - ref).abs() / (atol + ref.abs())).max().item()


def bf16_excess(got, ref, bound_f32, extra=0.0):
    """The bf16 outputs' measure: max over elements of |got - ref| / (2^-8 |ref| + (bound_f32 + extra) (rms_row +
    |ref|)); within bound when <= 1. 2^-8 is bf16's unit roundoff (8 significand bits, round to nearest), the second
    term the f32 error of the value that is rounded. `extra`: derived f32 roundings the f32 bound's formula does not
    contain (the dropout scale: 1 / (1 - p) and the product, 2 * 2^-24)."""
    got, ref = got.double(), ref.double()
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    allow = 2.0 ** -8 * ref.abs() + (bound_f32 + extra) * (rms + ref.abs())
    return ((got - ref).abs() / allow.clamp_min(1e-300)).max().item()


# ---------------------------------------------------------------------------------------------- forward, backward
def _stats(x, dtype):
    x = x.to(dtype)
    mean = x.mean(-1, keepdim=True)
    var = (x - mean).pow(2).mean(-1, keepdim=True)              # biased
    return x, mean, (var + EPS).rsqrt()


def ln_fwd(x, w, b, dtype=f64):
    """-> (y, mean [rows], rstd [rows]): y = (x - mean) rstd w + b, rstd = (biased var + 1e-5)^-1/2."""
    x, mean, rstd = _stats(x, dtype)
    return (x - mean) * rstd * w.to(dtype) + b.to(dtype), mean[:, 0], rstd[:, 0]


def _ln_prime(g, xh, rstd):
    return rstd * (g - g.mean(-1, keepdim=True) - xh * (g * xh).mean(-1, keepdim=True))


def ln_bwd(dy, x, w, dres=None, zero_mod=0, gmul=None, dtype=f64):
    """The header of ln_bwd_kernel. -> (dx, dw, db, zrow):
      dx = dres + rstd (g - mean(g) - xh mean(g xh)), g = dy w, xh = (x - mean) rstd; dw = sum_r dy xh, db = sum_r dy;
      zero_mod > 0: rows r % zero_mod == 0 of dx are returned as zrow [ceil(rows / zero_mod), D] and zeroed in dx;
      gmul: dx = LN'(dy) gmul (the GELU backward of the linear before the head's LayerNorm; no dres)."""
    x, mean, rstd = _stats(x, dtype)
    dy = dy.to(dtype)
    xh = (x - mean) * rstd
    dx = _ln_prime(dy * w.to(dtype), xh, rstd)
    if gmul is not None:
        dx = dx * gmul.to(dtype)
    if dres is not None:
        dx = dx + dres.to(dtype)
    zrow = None
    if zero_mod > 0:
        zrow = dx[::zero_mod].clone()
        dx = dx.clone()
        dx[::zero_mod] = 0
    return dx, (dy * xh).sum(0), dy.sum(0), zrow


def ln_bwd_multi(dys, x, ws, dres=None, dtype=f64):
    """n LayerNorms of one input: dx = dres + sum_j LN'_j(dys[j]) -> (dx, [(dw_j, db_j)])."""
    dx = dres.to(dtype) if dres is not None else 0
    grads = []
    for dy, w in zip(dys, ws):
        d, dw, db, _ = ln_bwd(dy, x, w, dtype=dtype)
        dx = dx + d
        grads.append((dw, db))
    return dx, grads


# ---------------------------------------------------------------------------------------------- dropout mask
_M64 = (1 << 64) - 1


def mix64(z):
    """The splitmix64 finaliser (common.h mix64) on a numpy uint64 array; the products wrap modulo 2^64."""
    with np.errstate(over='ignore'):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dropout_uniforms(seed, rows, cols):
    """rand_uniform4 for every element of a [rows, cols] matrix (cols % 4 == 0): element (r, c) takes 16-bit field
    (r cols + c) % 4 of the hash of q = (r cols + c) >> 2, u = (field + 0.5) / 65536 in float32. -> float32 numpy."""
    assert cols % 4 == 0
    base = ((int(seed) & _M64) * 0x9E3779B97F4A7C15 + 0x632BE59BD9B4E019) & _M64
    with np.errstate(over='ignore'):
        r = mix64(np.arange(rows * cols // 4, dtype=np.uint64) + np.uint64(base))
    fields = np.stack([(r >> np.uint64(s)) & np.uint64(0xFFFF) for s in (0, 16, 32, 48)], axis=1)
    u = (fields.astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 65536.0)
    return u.reshape(rows, cols)


def dropout_keep(seed, rows, cols, p):
    """-> bool [rows, cols] (CPU): the elements the dropout of (seed, p) keeps, u >= p in float32."""
    return torch.from_numpy(dropout_uniforms(seed, rows, cols) >= np.float32(p))


def dropout_scale(p):
    """1 / (1 - p) as the kernels form it: float32 operands, one correctly rounded division."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


# ---------------------------------------------------------------------------------------------- the launchers' plans
def fwd_maxv(D):
    """ln_fwd_plan's layout: float4 chunks per lane (even: runs of 8 columns, odd: runs of 4)."""
    return 2 if (D % 8 == 0 and D <= 512) else 3 if D <= 768 else 4 if D % 8 == 0 else 5


def bwd_maxv(D):
    return 2 if D <= 512 else 3 if D <= 768 else 4


def _rows_per_wave(rows, blocks):
    nw = 4 * blocks
    return rows // nw, -(-rows // nw)


def fwd_rows_per_wave(rows, D):
    """-> (fewest, most) rows a wave of the forward's grid takes (ln_fwd_plan: min(ceil(rows / 4), 2048 blocks for
    D <= 768, 1024 above), 4 waves each, wave v takes rows v, v + waves, ...)."""
    return _rows_per_wave(rows, min((rows + 3) // 4, 2048 if D <= 768 else 1024))


def bwd_rows_per_wave(rows):
    """The same for the backward kernels (svae_layernorm_nblk: min(ceil(rows / 4), 1024) blocks)."""
    return _rows_per_wave(rows, bwd_nblk(rows))


def bwd_nblk(rows):
    return min((rows + 3) // 4, 1024)


# ---------------------------------------------------------------------------------------------- cases and inputs
ENGINE_WIDTHS = (64, 320, 512, 576, 768, 832, 1024)         # d % 64 == 0; 320, 576, 832 fill their last run partly
LIB_WIDTHS = (8, 132, 516, 772, 1020)                       # D % 4 == 0 only
WIDTHS = ENGINE_WIDTHS + LIB_WIDTHS
SMALL_ROWS = (1, 5, 333)
LOOP_WIDTHS = (64, 132, 576, 772, 1024)                     # one per layout class


def fwd_loop_rows(D):
    return (8192 if D <= 768 else 4096) + 5                 # the smallest grid at which a wave takes a second row


FWD_LOOP = tuple((fwd_loop_rows(D), D, 2) for D in LOOP_WIDTHS) + ((16384 + 3, 64, 3),)   # (rows, D, most rows / wave)
BWD_LOOP = tuple((4096 + 7, D, 2) for D in LOOP_WIDTHS) + ((2 * 4096 + 3, 64, 3),)
SMALL = tuple((r, D) for D in WIDTHS for r in SMALL_ROWS)
FWD_CASES = SMALL + tuple(c[:2] for c in FWD_LOOP)
BWD_CASES = SMALL + tuple(c[:2] for c in BWD_LOOP)
MULTI_BWD_CASES = ((4096 + 7, 64), (4096 + 7, 576), (4096 + 7, 1024), (333, 772))
MULTI_N = (1, 2, LN_MULTI_MAX)
GELU_CASES = ((4096 + 7, 576), (333, 132), (2 * 4096 + 3, 64))
ZERO_MOD = 37                                               # not a multiple of a block's 4 rows
ZSPLICE_CASES = ((333, 64), (333, 132), (333, 576), (333, 1024))


class Case:
    pass


@functools.lru_cache(maxsize=4)
def inputs(rows, D, n=1, integer_dy=False):
    """The GPU tests' inputs (drawn on the CPU: the same on every device). x = 2 randn + 0.5 + an offset of
    ((37 r) % 101) / 25 - 2 per row (neighbouring rows and rows one grid stride apart differ, so a row read from the
    wrong place shows in mean[r]); LayerNorm j: w = (j + 1) (1 + 0.1 randn), b = 0.1 randn + j (visibly different per
    j; j = 0 is the usual near-identity affine); dy bf16 N(0, 1) (integer_dy: integers in {-2 .. 2}, every f32 sum of
    which is exact); dres f32 N(0, 1); gp bf16 in [-0.1, 1.1] (a GELU')."""
    gen = torch.Generator().manual_seed(100003 * rows + 11 * D + n + 7 * int(integer_dy))
    c = Case()
    off = (torch.arange(rows) * 37 % 101).float() / 25 - 2
    c.x = torch.randn(rows, D, generator=gen) * 2 + 0.5 + off[:, None]
    c.ws = [(1 + 0.1 * torch.randn(D, generator=gen)) * (j + 1) for j in range(n)]
    c.bs = [0.1 * torch.randn(D, generator=gen) + j for j in range(n)]
    if integer_dy:
        c.dys = [torch.randint(-2, 3, (rows, D), generator=gen).to(bf16) for _ in range(n)]
    else:
        c.dys = [torch.randn(rows, D, generator=gen).to(bf16) for _ in range(n)]
    c.dres = torch.randn(rows, D, generator=gen)
    c.gp = (torch.rand(rows, D, generator=gen) * 1.2 - 0.1).to(bf16)
    return c


# ---------------------------------------------------------------------------------------------- bounds
TOL_FACTOR = 4.0
FLOOR = 2.0 ** -21       # four float32 ulps: the device's rsqrtf and division, which the CPU restatement does not have
BOUND_KEYS = ('fwd.mean', 'fwd.rstd', 'fwd.y', 'bwd.dx', 'bwd.dw', 'bwd.db', 'multi.dx', 'multi.dw', 'multi.db',
              'gelu.out')


@functools.lru_cache(maxsize=None)
def recorded():
    """The f32-vs-f64 deviations test_ln_ref.py measured and wrote (tests/golden/ln_bounds.json)."""
    with open(BOUNDS_PATH) as f:
        return json.load(f)['f32_vs_f64_deviation']


def bound(key):
    """What an f32 output is held to on the GPU: 4 x the recorded deviation of the same formulas, never below FLOOR."""
    return max(TOL_FACTOR * recorded()[key], FLOOR)
