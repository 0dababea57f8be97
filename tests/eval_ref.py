"""Plain torch restatements of the fp32-mode kernels of csrc/fp32.hip (svae_gemm_f32, svae_attn_fwd_f32,
svae_layernorm_fwd_f32) and of the evaluation reductions of csrc/elementwise.hip (svae_ce_seq_logprob,
svae_mutual_info), the inputs the GPU tests feed them and the error bounds those tests hold them to. Every formula
takes a `dtype`: float64 is the reference, float32 the same formula at the kernels' precision, with the sums the
kernels take as one chain of additions (over K, over the head dimension, over the keys, over the latent) taken as a
chain here too, and their lane-strided tree reductions as such trees (chain, lane_sum). test_eval_ref.py measures the distance between the two on the GPU tests' own inputs; that distance
is what the bounds are built from. `mutate` turns one representative mistake on in the float32 form (test_eval_ref.py
holds each to leaving its bound). Everything is drawn and computed on the CPU. Nothing in this file runs product code
but engine.rotary_table, the host-side table the rotary GEMM epilogue is handed."""
import functools
import math

import torch

import oracle
from optim_ref import LOG2E, TOL_FACTOR, deviation

f64, f32 = torch.float64, torch.float32

# One unit in the last place of an f32 result, relative: the accuracy the CDNA ISA documents for v_exp_f32 and
# v_log_f32, the instructions behind __expf (v_exp_f32(x * log2 e)) and __logf (v_log_f32(x) * ln 2). The float32
# restatements below use correctly rounded exp2 / log; the kernels' results may differ from those by this much.
ULP = 2.0 ** -23


def _exp(x):
    """exp; in float32 as the kernels write it, exp2(x * log2 e) (optim_ref._exp)."""
    return x.exp() if x.dtype == f64 else torch.exp2(x * LOG2E)


def chain(terms, dim):
    """Sum over `dim`: float64 as torch sums, float32 as one chain of additions in index order (a kernel's
    `for (k...) acc += ...`), each rounded to f32."""
    if terms.dtype == f64:
        return terms.sum(dim)
    acc = None
    for t in terms.unbind(dim):
        acc = t.clone() if acc is None else acc + t
    return acc


def lane_sum(x, width=64):
    """Sum over the last dim: float64 as torch sums; float32 as the kernels' reductions go: `width` lanes each chain
    the elements width apart, then a tree over the lanes. (Spelled out so that the measured deviations do not depend
    on the order the host's torch build happens to sum in.)"""
    if x.dtype == f64:
        return x.sum(-1)
    n = x.shape[-1]
    trips = -(-n // width)
    p = torch.zeros(*x.shape[:-1], trips * width, dtype=x.dtype)
    p[..., :n] = x
    a = chain(p.view(*x.shape[:-1], trips, width), -2)
    while a.shape[-1] > 1:
        h = a.shape[-1] // 2
        a = a[..., :h] + a[..., h:]
    return a[..., 0]


def abs_deviation(err, ref, rows=False):
    """deviation() of an absolute error bound `err` (same shape as ref): max err / (atol + |ref|)."""
    err, ref = err.double(), ref.double()
    if not rows:
        err, ref = err.reshape(1, -1), ref.reshape(1, -1)
    atol = ref.pow(2).mean(-1, keepdim=True).sqrt()
    return (err / (atol + ref.abs())).max().item()


# ---------------------------------------------------------------------------------------------- svae_gemm_f32
GEMM_EXACT = ((1, 1, 1), (5, 130, 64), (65, 127, 17), (64, 64, 16), (130, 200, 72))


def gemm_int_case(M, N, K):
    """Integers in [-4, 4]: with K <= 72 every partial sum is below 2^24 in size and exact in f32 in any order.
    -> A [M, K], W [N, K], bias [N], resid [M, N], all f32."""
    gen = torch.Generator().manual_seed(100 * M + 10 * N + K)
    A, W = (torch.randint(-4, 5, s, generator=gen).float() for s in ((M, K), (N, K)))
    return A, W, torch.randint(-4, 5, (N,), generator=gen).float(), torch.randint(-4, 5, (M, N), generator=gen).float()


# name -> M, N, K, epilogue, (rot_cols, rot_d, rot_seq)
GEMM_CASES = {
    'f32':        (70, 66, 1032, 'f32', None),          # K: 64 steps of 16 and a tail of 8; ragged tiles in M and N
    'gelu':       (37, 61, 72, 'gelu', None),           # odd N, K tail of 8
    'rot_ragged': (17, 61, 40, 'rotary', (40, 20, 7)),  # rows wrap the table, rotation stops inside the tile, odd N
    'rot_engine': (26, 72, 24, 'rotary', (48, 24, 13)), # the engine's q|k|v form: N = 3d, rot_cols = 2d, rot_d = d
}


@functools.lru_cache(maxsize=None)
def gemm_case(name):
    """A ~ N(0, 1), W ~ N(0, 1 / K) (products of unit variance), bias ~ N(0, 1), resid ~ N(0, 1) (the F32 epilogue
    alone takes it, as in the engine). -> dict(A, W, bias, resid or None, rot or None)."""
    M, N, K, epi, rot = GEMM_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    A = torch.randn(M, K, generator=gen)
    W = torch.randn(N, K, generator=gen) / math.sqrt(K)
    bias = torch.randn(N, generator=gen)
    resid = torch.randn(M, N, generator=gen) if epi == 'f32' else None
    tab = None
    if rot:
        from sparse_vae.engine import rotary_table
        tab = rotary_table(rot[2], rot[1])
    return dict(A=A, W=W, bias=bias, resid=resid, rot=tab)


def gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))


def _rotary_f64(x, rot_cols, rot_d, rot_seq):
    """oracle.rotary on each rot_d-wide group of the first rot_cols columns; row m sits at position m % rot_seq."""
    M = x.shape[0]
    reps = -(-M // rot_seq)
    out = x.clone()
    for c0 in range(0, rot_cols, rot_d):
        blk = torch.zeros(reps * rot_seq, rot_d, dtype=x.dtype)
        blk[:M] = x[:, c0:c0 + rot_d]
        out[:, c0:c0 + rot_d] = oracle.rotary(blk.view(reps, rot_seq, rot_d)).reshape(-1, rot_d)[:M]
    return out


def _rotary_table(x, tab, rot_cols, rot_d, rot_seq, flip=False):
    """The epilogue's form: (a, b) -> (a cos + (-b) sin, b cos + a sin) with (cos, sin) = tab[m % rot_seq][(n % rot_d)
    / 2], the f32 table."""
    M = x.shape[0]
    cs = tab.to(x.dtype)[torch.arange(M) % rot_seq]                       # [M, rot_d / 2, 2]
    out = x.clone()
    for c0 in range(0, rot_cols, rot_d):
        a, b = x[:, c0:c0 + rot_d:2], x[:, c0 + 1:c0 + rot_d:2]
        c, s = cs[..., 0], cs[..., 1]
        out[:, c0:c0 + rot_d:2] = a * c + (b if flip else -b) * s
        out[:, c0 + 1:c0 + rot_d:2] = b * c + a * s
    return out


def gemm(A, W, bias=None, resid=None, epi='f32', rot=None, rot_args=None, dtype=f64, mutate=None):
    """epi(A . W^T + bias) + resid. float64: the rotary epilogue is oracle.rotary with float64 angles; float32: a
    k-ordered chain and the f32 table. mutate: 'drop_k_tail' (the last K % 16 columns are not read), 'rot_sign'."""
    A, W = A.to(dtype), W.to(dtype)
    if mutate == 'drop_k_tail':
        A, W = A[:, :A.shape[1] // 16 * 16], W[:, :W.shape[1] // 16 * 16]
    x = A @ W.t() if dtype == f64 else chain(A[:, None, :] * W[None, :, :], -1)
    if bias is not None:
        x = x + bias.to(dtype)
    if epi == 'gelu':
        x = gelu(x)
    elif epi == 'rotary':
        x = _rotary_f64(x, *rot_args) if dtype == f64 else _rotary_table(x, rot, *rot_args, flip=mutate == 'rot_sign')
    if resid is not None:
        x = x + resid.to(dtype)
    return x


def gemm_eval(name, dtype=f64, mutate=None):
    c = gemm_case(name)
    _, _, _, epi, rot_args = GEMM_CASES[name]
    return gemm(c['A'], c['W'], c['bias'], c['resid'], epi, c['rot'], rot_args, dtype, mutate)


# ---------------------------------------------------------------------------------------------- svae_attn_fwd_f32
# name -> B, H, Lq, Lk, hd, causal, window, pad: None | per-batch first padded key
ATTN_CASES = {
    'engine':     (2, 3, 37, 37, 20, True, 0, (30, 25)),      # B H L = 222: the last block has two idle waves
    'hd96':       (1, 2, 33, 33, 96, True, 0, None),          # the output loop runs twice for lanes < 32
    'hd130':      (1, 2, 33, 33, 130, True, 0, None),         # three times for lanes < 2
    'cross':      (2, 2, 5, 70, 12, False, 0, (60, 33)),
    'win1_96':    (1, 2, 96, 96, 16, True, 1, None),
    'win2_96':    (1, 2, 96, 96, 16, True, 2, None),
    'win2_100':   (1, 2, 100, 100, 16, True, 2, None),        # L % 32 != 0: oracle.sparse_mask's decoding-prefix branch
    'allpad':     (2, 2, 5, 40, 8, False, 0, (35, 0)),        # every key of batch element 1 is padded
    'lk8192':     (1, 1, 3, 8192, 8, False, 0, None),         # the last key count of the 4-wave instance
    'lk8193':     (1, 1, 3, 8193, 8, False, 0, None),         # the first of the 2-wave instance
    'lk8193_q5':  (1, 1, 5, 8193, 8, False, 0, None),         # ... with an idle wave in the last block
    'lk16384':    (1, 1, 3, 16384, 8, False, 0, None),
    'lk16385':    (1, 1, 3, 16385, 8, False, 0, None),        # the first of the 1-wave instance
    'lk32768':    (1, 1, 3, 32768, 8, False, 0, None),        # the limit
}
ATTN_MAX_KEYS = 32768


@functools.lru_cache(maxsize=None)
def attn_case(name):
    """q [B, Lq, H hd], k, v [B, Lk, H hd] ~ N(0, 1) (scores of unit variance); pad uint8 [B, Lk] or None."""
    B, H, Lq, Lk, hd, causal, window, padspec = ATTN_CASES[name]
    gen = torch.Generator().manual_seed(sum(map(ord, name)))
    q = torch.randn(B, Lq, H * hd, generator=gen)
    k, v = torch.randn(B, Lk, H * hd, generator=gen), torch.randn(B, Lk, H * hd, generator=gen)
    pad = None
    if padspec is not None:
        pad = torch.zeros(B, Lk, dtype=torch.uint8)
        for b, first in enumerate(padspec):
            pad[b, first:] = 1
    return dict(q=q, k=k, v=v, pad=pad)


def attn_mask(name, causal_ge=False):
    """bool [B, 1, Lq, Lk], True where a key is not visible: key_pad | causal | oracle.sparse_mask."""
    B, H, Lq, Lk, hd, causal, window, _ = ATTN_CASES[name]
    pad = attn_case(name)['pad']
    m = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool)
    if pad is not None:
        m = m | pad.bool()[:, None, None, :]
    if window:
        m = m | oracle.sparse_mask(Lq, window)
    elif causal:
        m = m | torch.ones(Lq, Lk, dtype=torch.bool).triu(1)
    if causal and causal_ge:
        m = m | torch.eye(Lq, Lk, dtype=torch.bool)
    return m


def heads(t, H):
    return t.view(t.shape[0], t.shape[1], H, -1).transpose(1, 2)          # [B, H, L, hd]


def attention(q, k, v, mask, dtype=f64):
    """softmax(q k^T hd^-1/2 - 1e7 mask) v (attention.py:83-100) on [B, H, L, hd]; -> [B, H, Lq, hd]. float32: the
    dot products and the weighted sum of v as chains over hd and over the keys, the weights' sum divided out last."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    scale = torch.tensor(q.shape[-1] ** -0.5, dtype=dtype)                # (the kernel is handed its f32 rounding)
    if dtype == f64:
        s = q @ k.transpose(-1, -2)
    else:
        s = chain(q[:, :, :, None, :] * k[:, :, None, :, :], -1)
    s = s * scale
    s = torch.where(mask, s - 1e7, s)
    e = (s - s.max(-1, keepdim=True).values).exp()
    if dtype == f64:
        return (e @ v) / e.sum(-1, keepdim=True)
    return chain(e[..., None] * v[:, :, None, :, :], -2) / lane_sum(e)[..., None]


def attn_eval(name, dtype=f64, mutate=None):
    """-> [B, Lq, H hd], the layout of the kernel's output. mutate: 'causal_ge' (j >= qi masked)."""
    c, H = attn_case(name), ATTN_CASES[name][1]
    o = attention(heads(c['q'], H), heads(c['k'], H), heads(c['v'], H), attn_mask(name, mutate == 'causal_ge'), dtype)
    return o.transpose(1, 2).reshape(o.shape[0], o.shape[2], -1)


def attn_dead_rows(name):
    """bool [B, Lq]: queries every key of which is masked (the -1e7 shift rounds their f32 scores to whole numbers:
    no float64 comparison there)."""
    return attn_mask(name).all(-1)[:, 0]


# ---------------------------------------------------------------------------------------------- svae_layernorm_fwd_f32
LN_SHAPES = ((1, 1), (1, 20), (7, 20), (5, 64), (5, 200), (1, 768), (7, 768))
LN_OFFSET_SHAPES = ((5, 200), (7, 768))
LN_CONSTANTS = (2.5, -3.0, 0.0, 1000.0, 0.125, -0.5, 64.0)      # D times each is exact in f32 in any order (D <= 768)


@functools.lru_cache(maxsize=None)
def ln_case(rows, D, kind='normal'):
    """x [rows, D], w, b [D]. 'normal': x ~ 2 N(0, 1) + 0.5; 'offset': every row 1000 + 1e-2 N(0, 1), where a
    one-pass variance E x^2 - (E x)^2 loses everything; 'const': row r holds LN_CONSTANTS[r] throughout (y = b)."""
    gen = torch.Generator().manual_seed(31 * rows + D)
    x = torch.randn(rows, D, generator=gen) * 2 + 0.5
    w, b = torch.randn(D, generator=gen) * 0.1 + 1, torch.randn(D, generator=gen) * 0.1
    if kind == 'offset':
        x = 1000 + 1e-2 * torch.randn(rows, D, generator=gen)
    elif kind == 'const':
        x = torch.tensor(LN_CONSTANTS[:rows])[:, None].expand(rows, D).contiguous()
    return x, w, b


def layernorm(x, w, b, dtype=f64, mutate=None):
    """(x - mean) / sqrt(var + 1e-5) * w + b, var the mean of (x - mean)^2. mutate: 'one_pass' (var = E x^2 -
    mean^2)."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    D = x.shape[-1]
    mean = lane_sum(x)[..., None] / D
    if mutate == 'one_pass':
        var = lane_sum(x * x)[..., None] / D - mean * mean
    else:
        var = lane_sum((x - mean).pow(2))[..., None] / D
    return (x - mean) * (1.0 / (var + 1e-5).sqrt()) * w + b


# ---------------------------------------------------------------------------------------------- svae_ce_seq_logprob
CE_TILE = 128
CE_CASES = ((128, 3, 5), (300, 2, 7), (128 * 65, 2, 4), (32768, 2, 9))      # V, sequences, seq


def ce_part(logits):
    """The head GEMM's CE statistics of f64 logits [rows, V]: per 128-wide tile (max, sum exp(x - max)), a tile with
    no finite entry (-inf, 0). -> f64 [rows, ntile, 2]."""
    rows, V = logits.shape
    ntile = -(-V // CE_TILE)
    x = torch.full((rows, ntile * CE_TILE), -math.inf, dtype=f64)
    x[:, :V] = logits
    x = x.view(rows, ntile, CE_TILE)
    mx = x.max(-1).values
    se = torch.where(mx.isinf(), torch.zeros_like(mx), (x - mx.clamp_min(-1e300)[..., None]).exp().sum(-1))
    return torch.stack([mx, se], -1)


@functools.lru_cache(maxsize=None)
def ce_case(V, nseq, seq):
    """logits f64 [nseq seq, V] ~ 3 N(0, 1); labels int32: a third of the rows 0, sequence 1 all 0; one whole tile
    -inf: tile 1 of row 0 (a live row whose label lies in tile 0), or with a single tile the whole of row 1, whose
    label is 0 (a row the kernel must not read into the sum). -> dict(logits, labels, part f32, label_logit f32)."""
    rows = nseq * seq
    gen = torch.Generator().manual_seed(V + 7 * seq)
    logits = torch.randn(rows, V, generator=gen, dtype=f64) * 3
    labels = torch.randint(1, V, (rows,), generator=gen, dtype=torch.int32)
    labels[torch.rand(rows, generator=gen) < 1 / 3] = 0
    labels[seq:2 * seq] = 0
    labels[0], labels[1], labels[2] = 1 + int(labels[0]) % (CE_TILE - 1), 0, max(1, int(labels[2]))
    if V > CE_TILE:
        logits[0, CE_TILE:min(V, 2 * CE_TILE)] = -math.inf
    else:
        logits[1] = -math.inf
    ll = logits.gather(1, labels.long()[:, None])[:, 0]
    return dict(logits=logits, labels=labels, part=ce_part(logits).float(), label_logit=ll.float())


def seq_logprob(logits, labels, seq):
    """continuous_autoencoder.py:82-88 in float64: sum over a sequence's rows with label != 0 of log_softmax[label]."""
    lse = logits.logsumexp(-1)
    val = logits.gather(1, labels.long()[:, None])[:, 0] - lse
    return torch.where(labels != 0, val, torch.zeros_like(val)).view(-1, seq).sum(-1)


def seq_logprob_from_part(part, label_logit, labels, seq, dtype=f32, mutate=None, order='torch'):
    """The kernel's formula from the per-tile statistics: lse = M + log sum_t s_t exp(m_t - M), M = max_t m_t; a tile
    at -inf adds 0. order: how a sequence's rows are added, 'torch' | 'fwd' | 'rev' (chains); SUM_ORDERS names all
    three: a sum of a handful of rows lands on its f32 neighbours by luck, so the measurement takes the worst of them.
    mutate: 'count_label0' (label-0 rows are summed too)."""
    part, ll = part.to(dtype), label_logit.to(dtype)
    m, s = part[..., 0], part[..., 1]
    M = m.max(-1, keepdim=True).values
    se = lane_sum(torch.where(m.isinf(), torch.zeros_like(s), s * _exp(m - M)))
    val = ll - (M[:, 0] + se.log())
    if mutate != 'count_label0':
        val = torch.where(labels != 0, val, torch.zeros_like(val))
    val = val.view(-1, seq)
    return val.sum(-1) if order == 'torch' else chain(val if order == 'fwd' else val.flip(-1), -1)


SUM_ORDERS = ('torch', 'fwd', 'rev')


def ce_intrinsic(part, labels, seq, ref, tile_exp=False):
    """What __expf and __logf may add to a sequence's sum, as a deviation. Per live row: every term of sum_t s_t
    exp(m_t - M) carries a relative error of ULP from v_exp_f32 (the product's rounding is in _exp already), so log of
    the sum moves by ULP; __logf = v_log_f32(se) ln 2 is off by ULP relative, |ln se| ULP absolute. tile_exp: the
    statistics come from the head GEMM's epilogue, whose tile sums are __expf terms too (ULP more on ln se)."""
    part = part.double()
    m, s = part[..., 0], part[..., 1]
    M = m.max(-1, keepdim=True).values
    se = torch.where(m.isinf(), torch.zeros_like(s), s * (m - M).exp()).sum(-1)
    row = ULP * ((2.0 if tile_exp else 1.0) + se.log().abs())
    row = torch.where(labels != 0, row, torch.zeros_like(row))
    return abs_deviation(row.view(-1, seq).sum(-1), ref)


COMPOSITE = (2, 40, 64, 1024)          # sequences, seq, d, V


@functools.lru_cache(maxsize=None)
def composite_case():
    """The stats-only head GEMM's operands: hh bf16 [T, d] ~ N(0, 1), W bf16 [V, d] ~ N(0, 1) / sqrt(d) * 2, bias f32
    [V] ~ 0.1 N(0, 1), labels with zeros (the last position of every sequence among them, as engine.seq_log_prob
    sets it)."""
    nseq, seq, d, V = COMPOSITE
    gen = torch.Generator().manual_seed(64 + 1024)
    hh = torch.randn(nseq * seq, d, generator=gen).bfloat16()
    W = (torch.randn(V, d, generator=gen) * 2 / math.sqrt(d)).bfloat16()
    bias = torch.randn(V, generator=gen) * 0.1
    labels = torch.randint(1, V, (nseq * seq,), generator=gen, dtype=torch.int32)
    labels[torch.rand(nseq * seq, generator=gen) < 0.2] = 0
    labels[seq - 1::seq] = 0
    return dict(hh=hh, W=W, bias=bias, labels=labels)


def composite_eval(dtype=f64, order='torch'):
    """float64: log_softmax of the logits of the bf16-rounded operands. float32: f32 logits by a k-ordered chain, their
    tile statistics in f32, then the kernel's formula. -> (per-sequence sums, the float64 statistics [T, ntile, 2])."""
    c, seq = composite_case(), COMPOSITE[1]
    logits = gemm(c['hh'].float(), c['W'].float(), c['bias'], dtype=dtype)
    if dtype == f64:
        return seq_logprob(logits, c['labels'], seq), ce_part(logits)
    x = logits.view(logits.shape[0], -1, CE_TILE)
    mx = x.max(-1).values
    part = torch.stack([mx, lane_sum(_exp(x - mx[..., None]))], -1)
    ll = logits.gather(1, c['labels'].long()[:, None])[:, 0]
    return seq_logprob_from_part(part, ll, c['labels'], seq, order=order), None


# ---------------------------------------------------------------------------------------------- svae_mutual_info
LOG_2PI = math.log(2 * math.pi)
MI_MAX_Z = 4096
# B, Z, S, regime. 'narrow': logvar uniform in [-1, 1], mu ~ N(0, 1). 'spread': logvar uniform in [-6, 2], mu ~ 3 N(0,
# 1)
# (posteriors several of their own standard deviations apart: one term dominates each logsumexp).
MI_CASES = ((1, 1, 1, 'narrow'), (2, 64, 10, 'narrow'), (2, 64, 10, 'spread'), (300, 70, 3, 'narrow'),
            (300, 70, 3, 'spread'), (5, 300, 2, 'narrow'), (64, 4096, 1, 'narrow'))


@functools.lru_cache(maxsize=None)
def mi_case(B, Z, S, regime):
    """-> stats f32 [B, 2Z] = (mu | logvar), eps f32 [S, B, Z] ~ N(0, 1), kl f32 [1] = the posterior's mean KL to the
    prior (what the training step hands the kernel)."""
    gen = torch.Generator().manual_seed(1000 * B + Z + S + len(regime))
    lo, hi, spread = (-1.0, 1.0, 1.0) if regime == 'narrow' else (-6.0, 2.0, 3.0)
    mu = torch.randn(B, Z, generator=gen) * spread
    lv = torch.rand(B, Z, generator=gen) * (hi - lo) + lo
    eps = torch.randn(S, B, Z, generator=gen)
    kl = (0.5 * (mu.double().pow(2) + lv.double().exp() - lv.double() - 1.0)).sum(-1).mean()
    return torch.cat([mu, lv], 1).contiguous(), eps, kl.float().reshape(1)


def mutual_info(stats, eps, kl, dtype=f64, mutate=None):
    """kl - marginal_kl (transformer_vae.py:59-61, math_utils.py:51-58): x[s][i] = mu_i + eps sd_i,
      log q_j(x) = sum_z -(x - mu_j)^2 / (2 var_j) - logvar_j / 2 - log sqrt(2 pi)        (a chain over z in float32)
      marginal[s][i] = logsumexp_j log q_j(x[s][i]) - log B,   sumsq[s][i] = sum_z x^2
      out = kl - (-(mean sumsq + Z log 2 pi) / 2 - mean marginal).
    -> dict(out 0-d, marginal [S B], sumsq [S B]), the last two in the order of the kernel's workspace.
    mutate: 'no_log_b'."""
    B, Z = stats.shape[0], stats.shape[1] // 2
    stats, eps = stats.to(dtype), eps.to(dtype)
    mu, lv = stats[:, :Z], stats[:, Z:]
    x = mu + eps * _exp(lv).sqrt()                                        # [S, B, Z]
    sumsq = lane_sum(x * x, 256)
    half_prec = 0.5 * _exp(-lv)
    marg = []
    for xs in x:                                                          # [B, Z]
        d = xs.t()[:, :, None] - mu.t()[:, None, :]                       # [Z, i, j]
        logq = chain(-(d * d) * half_prec.t()[:, None, :] - 0.5 * lv.t()[:, None, :] - 0.5 * LOG_2PI, 0)
        m = logq.max(-1, keepdim=True).values
        marg.append(m[:, 0] + lane_sum(_exp(logq - m), 256).log())
    marginal = torch.stack(marg)
    if mutate != 'no_log_b':
        marginal = marginal - math.log(B)
    n = sumsq.numel()
    sample_prob = -0.5 * (lane_sum(sumsq.flatten(), 256) / n + Z * LOG_2PI)
    return dict(out=kl.to(dtype)[0] - (sample_prob - lane_sum(marginal.flatten(), 256) / n), marginal=marginal.flatten(),
                sumsq=sumsq.flatten())


def mi_intrinsic(stats, eps, ref):
    """What the kernel's __expf / __logf may add, as deviations of {out, marginal, sumsq}, from float64 quantities.
      * sd = sqrt(__expf(logvar)): ULP relative on the exponential, half of it on sd: x moves by dx = ULP / 2 |eps sd|;
        sumsq by sum_z 2 |x| dx; log q_j by sum_z |x - mu_j| / var_j dx.
      * (x - mu_j)^2 * (0.5 __expf(-logvar_j)): ULP relative on every term of log q_j's quadratic part.
      * the logsumexp over j: a posterior's error enters with its softmax weight; the two __expf of the online
        combination add ULP each to the sum, __logf of the sum and of B |ln sum| ULP and ln B ULP.
      * out averages the marginal's errors and half the sumsq's."""
    B, Z = stats.shape[0], stats.shape[1] // 2
    stats, eps = stats.double(), eps.double()
    mu, lv = stats[:, :Z], stats[:, Z:]
    sd = (0.5 * lv).exp()
    x = mu + eps * sd
    dx = 0.5 * ULP * (eps * sd).abs()
    e_sq = (2 * x.abs() * dx).sum(-1)
    e_marg = torch.zeros(eps.shape[0], B, dtype=f64)
    for s in range(eps.shape[0]):
        for i0 in range(0, B, 16):                                        # [16, B, Z] at a time
            d = x[s, i0:i0 + 16, None, :] - mu[None]
            quad = d * d * 0.5 * (-lv).exp()
            logq = (-quad - 0.5 * lv - 0.5 * LOG_2PI).sum(-1)
            e_logq = ULP * quad.sum(-1) + (d.abs() * (-lv).exp() * dx[s, i0:i0 + 16, None, :]).sum(-1)
            lse = logq.logsumexp(-1)
            wgt = (logq - lse[:, None]).exp()
            e_marg[s, i0:i0 + 16] = (wgt * e_logq).sum(-1) + ULP * (2 + (lse - logq.max(-1).values).abs() + math.log(B))
    return dict(out=abs_deviation(e_marg.mean() + 0.5 * e_sq.mean(), ref['out']),
                marginal=abs_deviation(e_marg.flatten(), ref['marginal']),
                sumsq=abs_deviation(e_sq.flatten(), ref['sumsq']))


# ---------------------------------------------------------------------------------------------- recorded deviations
# Largest deviation() of the float32 evaluation of the formulas above from the float64 one over the GPU tests' inputs,
# measured on the CPU by test_eval_ref.py (which re-measures them and fails if one has moved by more than a quarter):
#   gemm_*:   gemm_eval(name) of the GEMM_CASES entry of that name;
#   attn:     attn_eval(name) over the ATTN_CASES of up to 100 keys, the rows of attn_dead_rows() left out;
#   attn_long: over those of 8192 keys and more (ATTN_LONG; the chain over the keys is what their deviation is made of);
#   ln:       layernorm over ln_case(rows, D) for LN_SHAPES; ln_offset: over ln_case(rows, D, 'offset'), per row;
#   seq_logprob: seq_logprob_from_part over CE_CASES, the worst of SUM_ORDERS; composite: composite_eval(), likewise;
#   mi_*:     mutual_info over the MI_CASES below the latent limit; mi_zmax_*: the case at Z = MI_MAX_Z (chains of 4096)
# The GPU bound is TOL_FACTOR times the constant (the kernels evaluate the same formulas in another, equally valid
# order), plus ce_intrinsic() / mi_intrinsic() where the kernel computes exp and log on the hardware's approximate
# units. Beside each: the largest value seen from the kernels on an MI355X.
F32_DEV = {
    'gemm_f32':         1.5e-06,   # kernels on an MI355X: 1.4e-6 (bound 6.00e-06)
    'gemm_gelu':        5.0e-07,   # kernels on an MI355X: 5.2e-7 (bound 2.00e-06)
    'gemm_rot_ragged':  2.7e-07,   # kernels on an MI355X: 2.1e-7 (bound 1.08e-06)
    'gemm_rot_engine':  3.7e-07,   # kernels on an MI355X: 4.1e-7 (bound 1.48e-06)
    'attn':             9.6e-07,   # kernels on an MI355X: 1.2e-6 (bound 3.84e-06)
    'attn_long':        3.2e-06,   # kernels on an MI355X: 3.9e-6 (bound 1.28e-05)
    'ln':               1.5e-07,   # kernels on an MI355X: 1.3e-7 (bound 6.00e-07)
    'ln_offset':        9.6e-03,   # kernels on an MI355X: 9.6e-3 (bound 3.84e-02)
    'seq_logprob':      4.2e-08,   # kernels on an MI355X: 4.2e-8 (bound 1.68e-07 + ce_intrinsic, 1.2e-8 .. 1.7e-8)
    'composite':        1.1e-07,   # kernels on an MI355X: 2.8e-8 (bound 4.40e-07 + ce_intrinsic, 2.8e-8)
    'mi_out':           9.1e-08,   # kernels on an MI355X: 4.6e-8 (bound 3.64e-07 + mi_intrinsic, 9e-9 .. 2.5e-7)
    'mi_marginal':      3.7e-07,   # kernels on an MI355X: 3.7e-7 (bound 1.48e-06 + mi_intrinsic, 5e-8 .. 2.1e-7)
    'mi_sumsq':         6.5e-08,   # kernels on an MI355X: 7.5e-8 (bound 2.60e-07 + mi_intrinsic, 8e-9 .. 4.8e-8)
    'mi_zmax_out':      5.7e-08,   # kernels on an MI355X: 5.7e-8 (bound 2.28e-07 + mi_intrinsic, 8.4e-8)
    'mi_zmax_marginal': 1.4e-06,   # kernels on an MI355X: 1.4e-6 (bound 5.60e-06 + mi_intrinsic, 4.4e-8)
    'mi_zmax_sumsq':    5.6e-08,   # kernels on an MI355X: 7.1e-8 (bound 2.24e-07 + mi_intrinsic, 3.7e-8)
}
ATTN_LONG = tuple(n for n in ATTN_CASES if ATTN_CASES[n][3] >= 8192)


def attn_key(name):
    return 'attn_long' if name in ATTN_LONG else 'attn'


def mi_key(Z, what):
    return ('mi_zmax_' if Z == MI_MAX_Z else 'mi_') + what


def bound(key, intrinsic=0.0):
    return TOL_FACTOR * F32_DEV[key] + intrinsic
