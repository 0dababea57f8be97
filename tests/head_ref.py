"""Plain torch restatements of the P-head cross-entropy kernels (svae.h "P-head cross entropy": svae_ce_label_logit,
the SVAE_EPI_CE_PROB head GEMM, svae_ce_prob_finalize[_fix], svae_ce_prob_bwd_prep, the SVAE_EPI_ROWSCALE_GATHER dX
GEMM, the k-weighted dW GEMM, svae_embedding_bwd_ce), the inputs the GPU tests feed them and the error bounds those
tests hold them to. Every formula takes a `dtype`: float64 is the reference, float32 the same formula at the
kernels' precision (exp written as exp2(x * log2 e), as the kernels write it); test_head_ref.py measures the
distance between the two, and that distance is what the bounds are built from. A float64 autograd evaluation of the
whole head (logits, chunked F.cross_entropy(ignore_index=0), times gscale) pins the restatements. Everything is
computed where its inputs live (the tests build and evaluate on the CPU). Nothing in this file runs product code.

Rows are t = b * L + p; labels[t] = 0 is an ignored row (every sequence's last position, and padding). The loss is
the mean over `nchunks` sequence chunks of the mean row loss of the chunk's labelled rows; chunk c holds positions
c * chunk_len ... of every sequence, the last chunk running to the end of the sequence."""
import functools

import torch
import torch.nn.functional as F

from optim_ref import LOG2E, TOL_FACTOR, deviation  # noqa: F401  (one error measure for every kernel test)

f64 = torch.float64
bf16 = torch.bfloat16
GSCALE = 0.75
SAT_LIMIT = 2.0 ** 100          # ce_prob_rows flags a labelled row whose sum of P is not below this


def _exp(x):
    return x.exp() if x.dtype == f64 else torch.exp2(x * LOG2E)


def _live(lab):
    return lab != 0


def chunk_of(rows, L, nchunks, chunk_len):
    """Chunk index of every row: min(position // chunk_len, nchunks - 1)."""
    return torch.clamp((torch.arange(rows) % L) // chunk_len, max=nchunks - 1)


# ---------------------------------------------------------------------------------------------- forward
def logits_of(hh, W, bias, dtype=f64):
    z = hh.to(dtype) @ W.to(dtype).t()
    return z if bias is None else z + bias.to(dtype)


def label_logit(hh, W, bias, lab, dtype=f64):
    """c[t] = hh[t] . W[lab[t]] + bias[lab[t]]; 0 where lab[t] == 0."""
    li = lab.long()
    c = (hh.to(dtype) * W.to(dtype)[li]).sum(-1)
    if bias is not None:
        c = c + bias.to(dtype)[li]
    return torch.where(_live(lab), c, torch.zeros_like(c))


def tile_sums(P, ntile=None):
    """Per (128-column tile, row) sums of P [rows, V], tile-major [ntile][rows]; the last tile may be partial."""
    rows, V = P.shape
    ntile = ntile or -(-V // 128)
    pad = torch.zeros(rows, ntile * 128, dtype=P.dtype)
    pad[:, :V] = P
    return pad.view(rows, ntile, 128).sum(-1).t().contiguous()


def finalize(part, off, lab, L, nchunks, chunk_len, dtype=f64):
    """part [ntile][rows] -> lse = off + log sum, row_loss = log sum (both 0 on ignored rows), chunk_w[c] = 1 /
    (labelled rows of chunk c * nchunks), nll = mean over chunks of the chunk's mean row loss, and the row sums."""
    live = _live(lab)
    se = part.to(dtype).sum(0)
    l = torch.where(live, se.log(), torch.zeros_like(se))
    lse = torch.where(live, off.to(dtype) + l, torch.zeros_like(se))
    ch = chunk_of(lab.numel(), L, nchunks, chunk_len)
    cnt = torch.zeros(nchunks, dtype=dtype).index_add_(0, ch, live.to(dtype))
    tot = torch.zeros(nchunks, dtype=dtype).index_add_(0, ch, l)
    return lse, l, 1.0 / (cnt * nchunks), (tot / cnt).sum() / nchunks, se


def prob_forward(hh, W, bias, lab, off, L, nchunks, chunk_len, dtype=f64):
    """-> dict: P = exp(logit - off) on labelled rows and 0 elsewhere (unrounded, `dtype`), part (its tile sums), lse,
    row_loss, chunk_w, nll, se (the row sums)."""
    x = logits_of(hh, W, bias, dtype) - off.to(dtype)[:, None]
    P = torch.where(_live(lab)[:, None], _exp(x), torch.zeros_like(x))
    part = tile_sums(P)
    lse, rl, cw, nll, se = finalize(part, off, lab, L, nchunks, chunk_len, dtype)
    return dict(P=P, part=part, lse=lse, row_loss=rl, chunk_w=cw, nll=nll, se=se)


def fix_rows(hh, W, bias, lab, off, rows, dtype=f64):
    """The saturation fix-up of `rows` (a LongTensor): P = exp(logit - max), lse = max + log sum P, row_loss = lse -
    off (off: the label logit), new offset = max. -> (P [len(rows), V], lse, row_loss, new_off)."""
    z = logits_of(hh[rows], W, bias, dtype)
    mx = z.max(-1).values
    P = _exp(z - mx[:, None])
    lse = mx + P.sum(-1).log()
    return P, lse, lse - off.to(dtype)[rows], mx


# ---------------------------------------------------------------------------------------------- backward
def bwd_prep(hh, lse, off, chunk_w, lab, gscale, L, nchunks, chunk_len, V, dtype=f64):
    """q = gscale * chunk_w[chunk] and r = q * exp(off - lse) (0 on ignored rows), r * hh (unrounded), and the one-hot
    column sums of dlogits: dbias[lab[t]] -= q[t]. -> (q, r, r * hh, dbias [V])."""
    live = _live(lab)
    ch = chunk_of(lab.numel(), L, nchunks, chunk_len)
    zero = torch.zeros(lab.numel(), dtype=dtype)
    q = torch.where(live, torch.as_tensor(gscale, dtype=dtype) * chunk_w.to(dtype)[ch], zero)
    r = torch.where(live, q * _exp(off.to(dtype) - lse.to(dtype)), zero)
    dbias = torch.zeros(V, dtype=dtype).index_add_(0, lab.long(), -q)
    return q, r, r[:, None] * hh.to(dtype), dbias


def rowscale_gather(A, Bm, row_a, row_b, gather, lab, alpha=1.0, dtype=f64):
    """C[m] = alpha * row_a[m] * (A[m] . Bm) - row_b[m] * gather[lab[m]], the second term where lab[m] != 0.
    A [M, K], Bm [K, N], gather [*, N]."""
    C = alpha * row_a.to(dtype)[:, None] * (A.to(dtype) @ Bm.to(dtype))
    g = row_b.to(dtype)[:, None] * gather.to(dtype)[lab.long()]
    return C - torch.where(_live(lab)[:, None], g, torch.zeros_like(g))


def dw_and_dbias(P, hh_r, r, ids=None, dout=None, hh=None, q=None, L=None, dtype=f64):
    """dW = P^T hh_r [V, D] (hh_r = r . hh as stored), the k-weighted row sums P^T r [V], and, with ids given, the
    one-hot part as svae_embedding_bwd_ce applies it onto a zero table: dtable[ids[t]] += dout[t] - q[t-1] * hh[t-1]
    (the second term for t % L != 0). -> (dW, rowsum, dtable or None)."""
    Pt = P.to(dtype).t()
    dW, rowsum = Pt @ hh_r.to(dtype), Pt @ r.to(dtype)
    if ids is None:
        return dW, rowsum, None
    g = dout.to(dtype).clone()
    inner = (torch.arange(ids.numel()) % L != 0).nonzero().flatten()
    g[inner] -= q.to(dtype)[inner - 1, None] * hh.to(dtype)[inner - 1]
    return dW, rowsum, torch.zeros(P.shape[1], g.shape[1], dtype=dtype).index_add_(0, ids.long(), g)


def next_ids(lab, L):
    """Token ids consistent with the labels: ids[t] = lab[t - 1] inside a sequence, 1 at its start."""
    ids = torch.ones_like(lab)
    inner = (torch.arange(lab.numel()) % L != 0).nonzero().flatten()
    ids[inner] = lab[inner - 1]
    return ids


# ---------------------------------------------------------------------------------------------- the whole head
def head_autograd(hh, W, bias, lab, L, nchunks, chunk_len, gscale=GSCALE):
    """float64 autograd of the head: logits, the mean over sequence chunks of F.cross_entropy(ignore_index=0), times
    gscale. -> dict nll, dhh, dW, dbias."""
    h, w, b = (t.double().clone().requires_grad_() for t in (hh, W, bias))
    B = lab.numel() // L
    z = (h @ w.t() + b).view(B, L, -1)[:, :L - 1]
    y = lab.view(B, L)[:, :L - 1].long()
    loss = torch.stack([F.cross_entropy(zc.flatten(end_dim=1), yc.flatten(), ignore_index=0)
                        for zc, yc in zip(z.split(chunk_len, dim=1), y.split(chunk_len, dim=1))]).mean()
    (loss * gscale).backward()
    return dict(nll=loss.detach(), dhh=h.grad, dW=w.grad, dbias=b.grad)


def head_chain(hh, W, bias, lab, L, nchunks, chunk_len, gscale=GSCALE, dtype=f64, store=None, fix=False):
    """The restatements chained as the engine chains the kernels. store = torch.bfloat16: P, r . hh and dhh pass
    through bf16 where the kernels store them in bf16 (the float32 evaluation of the chain is made this way: the
    storage format is part of the kernels' precision). fix: rows whose sum reaches SAT_LIMIT are recomputed by
    fix_rows. -> dict nll, dhh, dW, dbias, flagged."""
    st = (lambda t: t.to(store).to(dtype)) if store is not None else (lambda t: t)
    V = W.shape[0]
    off = label_logit(hh, W, bias, lab, dtype)
    f = prob_forward(hh, W, bias, lab, off, L, nchunks, chunk_len, dtype)
    P, part = f['P'], f['part']
    flagged = (_live(lab) & ~(f['se'] < SAT_LIMIT)).nonzero().flatten()
    if fix and flagged.numel():
        Pf, _, _, mx = fix_rows(hh, W, bias, lab, off, flagged, dtype)
        P, off = P.clone(), off.clone()
        P[flagged], off[flagged] = Pf, mx
        part = tile_sums(P)
    lse, rl, cw, nll, _ = finalize(part, off, lab, L, nchunks, chunk_len, dtype)
    if fix and flagged.numel():                  # the fix-up's row loss is against the label logit, not the new offset
        c = label_logit(hh, W, bias, lab, dtype)
        rl = torch.where(_live(lab), lse - c, torch.zeros_like(lse))
        ch = chunk_of(lab.numel(), L, nchunks, chunk_len)
        cnt = torch.zeros(nchunks, dtype=dtype).index_add_(0, ch, _live(lab).to(dtype))
        nll = (torch.zeros(nchunks, dtype=dtype).index_add_(0, ch, rl) / cnt).sum() / nchunks
    P = st(P)
    q, r, hh_r, dbias = bwd_prep(hh, lse, off, cw, lab, gscale, L, nchunks, chunk_len, V, dtype)
    dhh = st(rowscale_gather(P, W, r, q, W, lab, dtype=dtype))
    dW, rowsum, onehot = dw_and_dbias(P, st(hh_r), r, next_ids(lab, L), torch.zeros(lab.numel(), hh.shape[1]), hh, q,
                                      L, dtype)
    return dict(nll=nll, dhh=dhh, dW=dW + onehot, dbias=dbias + rowsum, flagged=flagged)


# ---------------------------------------------------------------------------------------------- inputs
B_SEQ = 3
ROW_SHAPES = {300: 100, 297: 99}                 # T -> L (B = 3)
VOCABS = (1024, 1160, 1096)                      # aligned; a second half tile of 8 columns; no second half, 8 columns
DIMS = (64, 200, 576)                            # one trip of the row walk; idle lanes; a second trip
NCHUNKS = (1, 3)
KERNEL_SHAPES = tuple((T, V, D) for T, V, D in ((300, 1024, 64), (300, 1160, 200), (297, 1096, 576), (300, 1160, 576),
                                                (297, 1160, 64), (300, 1096, 200)))
CHAIN_SHAPES = ((300, 1160, 200), (297, 1096, 576))
LONG_LAST_CHUNK = (300, 1160, 200, 3, 20)        # chunks of 20, 20 and 60 positions: position // chunk_len reaches 4
FINALIZE_NTILE = 65                              # V = 8320: ce_prob_rows' unrolled loop (ntile > 57) with a tail


def chunk_len_of(L, nchunks):
    return -(-(L - 1) // nchunks)


@functools.lru_cache(maxsize=None)
def head_case(T, V, D):
    """hh bf16 [T, D] ~ N(0, 1), W bf16 [V, D] ~ N(0, 4 / D) (logits of standard deviation 2), bias f32 [V] ~ 0.5 N(0,
    1), labels int32 [T] in [3, V): column V - 1, the first column of the last 128-column tile and a column used by
    five rows among them; 0 on every sequence's last position and on two padded tails. Drawn on the CPU."""
    L = ROW_SHAPES[T]
    gen = torch.Generator().manual_seed(100000 + 1000 * T + 7 * V + D)
    hh = torch.randn(T, D, generator=gen).to(bf16)
    W = (torch.randn(V, D, generator=gen) * (2.0 / D ** 0.5)).to(bf16)
    bias = 0.5 * torch.randn(V, generator=gen)
    lab = torch.randint(3, V, (B_SEQ, L), generator=gen, dtype=torch.int32)
    lab[0, 0], lab[1, 1], lab[2, 60] = V - 1, V - 1, V - 1     # row 2 L + 60: the second row tile
    lab[0, 5] = (V - 1) // 128 * 128
    lab[0, 7], lab[2, 40] = V - 3, V - 2
    lab[0, 10:13], lab[1, 20], lab[2, 70] = 17, 17, 17
    lab[:, L - 1] = 0
    lab[1, 60:], lab[2, 90:] = 0, 0
    return hh, W, bias, lab.view(T).contiguous()


SAT_HOT = 777
# unflagged with a large finite P; flagged, P finite, and still below 2^110 (a threshold moved up would miss it);
# flagged, P finite; flagged, overflowed
SAT_GAPS = (60.0, 74.0, 78.0, 100.0)


@functools.lru_cache(maxsize=None)
def sat_case(kind, T=300, V=1160, D=64):
    """Rows built as the saturation test of test_ce_chunked_gpu.py builds them: W[:, 0] = 0 except W[SAT_HOT] = e0,
    bias[SAT_HOT] = 0, and hh[t] = g * e0 on the chosen rows, whose logits are then the bias plus g in column SAT_HOT
    (a gap of g - bias[label] nats, |bias| < 2). kind 'mixed': 12 rows, three per gap of SAT_GAPS, spread over both row
    tiles; 'many': 150 rows alternating 78 and 100 (more than two rounds of the fix-up's 64 blocks) and 30 rows at 60;
    'none': 12 rows at 60; 'chain' (the whole-chain tests): one row at 60 and one at 100.
    -> (hh, W, bias, lab, gaps {row: g})."""
    hh, W, bias, lab = (t.clone() for t in head_case(T, V, D))
    W[:, 0] = 0
    W[SAT_HOT] = 0
    W[SAT_HOT, 0] = 1
    bias = bias.clamp(-1.9, 1.9)
    bias[SAT_HOT] = 0
    lab[lab == SAT_HOT] = SAT_HOT + 1
    live = (lab != 0).nonzero().flatten().tolist()
    if kind == 'mixed':
        rows = [live[i] for i in (0, 1, 2, 3, 50, 120, 121, 180, 190, 200, 201, len(live) - 1)]
        gaps = {r: SAT_GAPS[i % 4] for i, r in enumerate(rows)}
    elif kind == 'many':
        gaps = {r: (78.0, 100.0)[i % 2] for i, r in enumerate(live[:150])}
        gaps.update({r: 60.0 for r in live[150:180]})
    elif kind == 'chain':
        gaps = {live[3]: 60.0, live[len(live) // 2]: 100.0}
    else:
        gaps = {r: 60.0 for r in live[::20]}
    for r, g in gaps.items():
        hh[r] = 0
        hh[r, 0] = g
    return hh, W, bias, lab, gaps


def flagged_rows(hh, W, bias, lab):
    """The rows the fix-up has to list, decided in float64 with a margin of 2^3 either way of 2^100: asserts that no
    labelled row's sum lies in [2^97, 2^103], so rounding cannot move a row across the threshold."""
    off = label_logit(hh, W, bias, lab)
    se = prob_forward(hh, W, bias, lab, off, lab.numel(), 1, lab.numel())['se']
    live = _live(lab)
    assert bool(((se < 2.0 ** 97) | (se > 2.0 ** 103) | ~live).all())
    return (live & (se > 2.0 ** 103)).nonzero().flatten()


@functools.lru_cache(maxsize=None)
def finalize_case(T=300, ntile=FINALIZE_NTILE):
    """Synthetic tile sums for svae_ce_prob_finalize alone: part [ntile][T] uniform in [0.01, 2), each tile's values
    scaled by (1 + tile) so a tile taken twice or skipped moves the sum; offsets ~ 3 N(0, 1); head_case's labels."""
    gen = torch.Generator().manual_seed(4242 + ntile)
    part = (torch.rand(ntile, T, generator=gen) * 1.99 + 0.01) * (1 + torch.arange(ntile))[:, None]
    off = 3.0 * torch.randn(T, generator=gen)
    return part, off, head_case(T, 1160, 64)[3]


NORMAL_FLOOR = 2.0 ** -120     # 2^6 above the smallest normal number of f32 and bf16 (both 2^-126)


def exp_deviation(got, ref):
    """deviation() for P, a positive exponential spanning many orders of magnitude inside one row (a saturated row
    holds 1 beside e^-78): deviation() of got / ref from 1, i.e. half the relative error of each element, over the
    elements the formats hold as normal numbers (ref >= NORMAL_FLOOR; below it neither format promises a digit)."""
    got, ref = got.double(), ref.double()
    m = ref >= NORMAL_FLOOR
    return deviation(got[m] / ref[m], torch.ones_like(ref[m]))


def half_ulp_bf16(ref):
    """Half a unit in the last place of bf16 (8 significant bits) at |ref|: 2^(floor(log2 |ref|) - 8), between 2^-9
    and 2^-8 of |ref|; what round-to-nearest may move a value by."""
    return torch.exp2(torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** -126))) - 8)


def bf16_exp_within(got, ref, bound):
    """A bf16 P against its float64 value: |got - ref| <= half a bf16 ulp + 2 bound |ref| on normal elements (`bound`
    is one of exp_deviation(), half the relative error), got <= 2 NORMAL_FLOOR below them, exactly 0 where the
    reference is 0. -> the largest ratio of error to allowance."""
    got, ref = got.double(), ref.double()
    m = ref >= NORMAL_FLOOR
    worst = ((got[m] - ref[m]).abs() / (half_ulp_bf16(ref[m]) + 2 * bound * ref[m])).max().item() if m.any() else 0.0
    small = (ref < NORMAL_FLOOR) & (ref > 0)
    if small.any():
        worst = max(worst, (got[small] / (2 * NORMAL_FLOOR)).max().item())
    if (ref == 0).any():
        worst = max(worst, float('inf') if (got[ref == 0] != 0).any() else 0.0)
    return worst


def bf16_within(got, ref, bound, rows=True):
    """A bf16 output against its float64 value: |got - ref| <= half a bf16 ulp + bound (|ref| + rms(ref)): the
    rounding of the store, plus the float32 bound as deviation() measures it (with its absolute floor, per row of a
    2-D tensor). -> the largest ratio of error to allowance."""
    got, ref = got.double(), ref.double()
    if not rows:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    rms = ref.pow(2).mean(-1, keepdim=True).sqrt()
    allow = half_ulp_bf16(ref) + bound * (ref.abs() + rms)
    return ((got - ref).abs() / allow).max().item()


# ---------------------------------------------------------------------------------------------- per-kernel cases
def _f32(t):
    return t.to(torch.float32)


@functools.lru_cache(maxsize=None)
def kernel_case(T, V, D, nchunks, chunk_len=None):
    """Every kernel's inputs, each the float64 reference of what the previous kernel would deliver rounded to the
    format the kernel reads (so one kernel's error does not excuse the next), and nothing else. -> dict."""
    hh, W, bias, lab = head_case(T, V, D)
    L = ROW_SHAPES[T]
    cl = chunk_len or chunk_len_of(L, nchunks)
    c = _f32(label_logit(hh, W, bias, lab))
    fwd = prob_forward(hh, W, bias, lab, c, L, nchunks, cl)
    part = _f32(fwd['part'])
    lse, _, cw, _, _ = finalize(part, c, lab, L, nchunks, cl)
    lse, cw = _f32(lse), _f32(cw)
    q, r, hh_r, _ = bwd_prep(hh, lse, c, cw, lab, GSCALE, L, nchunks, cl, V)
    q, r = _f32(q), _f32(r)
    gen = torch.Generator().manual_seed(5 + T + V + D)
    live = (lab != 0).nonzero().flatten()
    q_gather = q.clone()
    q_gather[live[::7]] = 0                       # row_b == 0 on rows that carry a label
    q_emb = q.clone()
    q_emb[L - 1::L] = 0.37                        # non-zero on the row before each sequence start: must not leak
    return dict(hh=hh, W=W, bias=bias, lab=lab, L=L, nchunks=nchunks, chunk_len=cl, c=c, part=part, lse=lse,
                chunk_w=cw, q=q, r=r, P=fwd['P'].to(bf16), hh_r=hh_r.to(bf16), q_gather=q_gather, q_emb=q_emb,
                ids=next_ids(lab, L), dout=torch.randn(T, D, generator=gen))


def kernel_eval(k, dtype=f64):
    """Every kernel's outputs from kernel_case's inputs, in `dtype`. -> dict keyed as F32_DEV."""
    hh, W, bias, lab, L, n, cl = k['hh'], k['W'], k['bias'], k['lab'], k['L'], k['nchunks'], k['chunk_len']
    V = W.shape[0]
    fwd = prob_forward(hh, W, bias, lab, k['c'], L, n, cl, dtype)
    lse, rl, cw, nll, _ = finalize(k['part'], k['c'], lab, L, n, cl, dtype)
    q, r, hh_r, dbias = bwd_prep(hh, k['lse'], k['c'], k['chunk_w'], lab, GSCALE, L, n, cl, V, dtype)
    dW, rowsum, _ = dw_and_dbias(k['P'], k['hh_r'], k['r'], dtype=dtype)
    _, _, dtable = dw_and_dbias(k['P'][:1], k['hh_r'][:1], k['r'][:1], k['ids'], k['dout'], hh, k['q_emb'], L, dtype)
    return dict(label_logit=label_logit(hh, W, bias, lab, dtype), P=fwd['P'], part=fwd['part'], lse=lse, row_loss=rl,
                chunk_w=cw, nll=nll, q=q, r=r, hh_r=hh_r, dbias_scatter=dbias,
                dhh=rowscale_gather(k['P'], W, k['r'], k['q_gather'], W, lab, dtype=dtype), dW=dW, rowsum=rowsum,
                dtable=dtable)


@functools.lru_cache(maxsize=None)
def kernel_ref(T, V, D, nchunks, chunk_len=None):
    return kernel_eval(kernel_case(T, V, D, nchunks, chunk_len))


def kernel_deviations(got, ref, lab):
    """deviation() of each output of kernel_eval (or of the kernels) from the reference: matrices whose rows differ
    in scale per labelled row, everything else over the whole tensor."""
    live = (lab != 0).nonzero().flatten().to(ref['P'].device)
    d = {k: deviation(got[k], ref[k]) for k in ('label_logit', 'lse', 'row_loss', 'chunk_w', 'nll', 'q', 'r',
                                                'dbias_scatter', 'dW', 'rowsum', 'dtable') if k in got}
    if 'part' in got:                             # the last tile (ragged: 8 of 128 columns) on its own scale
        d['part_last'] = deviation(got['part'][-1], ref['part'][-1])
    if 'P' in got:
        d['P'] = exp_deviation(got['P'][live], ref['P'][live])
    for k, t in (('part', True), ('dhh', False)):
        if k in got:
            a, b = (x.t() if t else x for x in (got[k], ref[k]))
            d[k] = deviation(a[live], b[live], rows=True)
    return d


@functools.lru_cache(maxsize=None)
def finalize_eval(dtype=f64):
    part, off, lab = finalize_case()
    lse, rl, cw, nll, _ = finalize(part, off, lab, ROW_SHAPES[300], 3, chunk_len_of(100, 3), dtype)
    return dict(fin_lse=lse, fin_row_loss=rl, fin_chunk_w=cw, fin_nll=nll)


@functools.lru_cache(maxsize=None)
def fix_case(kind, nchunks=1):
    """svae_ce_prob_finalize_fix's inputs for sat_case(kind): the reference label logits, tile sums and P rounded to
    f32 / bf16 as the head GEMM delivers them (+inf where the exponent overflows), and the rows it has to flag."""
    hh, W, bias, lab, gaps = sat_case(kind)
    L = ROW_SHAPES[lab.numel()]
    c = _f32(label_logit(hh, W, bias, lab))
    fwd = prob_forward(hh, W, bias, lab, c, L, nchunks, chunk_len_of(L, nchunks))
    return dict(hh=hh, W=W, bias=bias, lab=lab, L=L, nchunks=nchunks, chunk_len=chunk_len_of(L, nchunks), c=c,
                part=_f32(fwd['part']), P=fwd['P'].to(bf16), gaps=gaps, flagged=flagged_rows(hh, W, bias, lab))


def fix_eval(k, dtype=f64):
    """Outputs of the finalize with the fix-up on fix_case's inputs: whole-length lse, row_loss and offsets (the flagged
    rows' from fix_rows, the others' from finalize), the flagged rows' P, chunk_w and nll."""
    lab, L, n, cl, fl = k['lab'], k['L'], k['nchunks'], k['chunk_len'], k['flagged']
    part = k['part'].to(dtype)
    part[:, fl] = 1.0                              # placeholders: these rows are replaced below
    lse, rl, cw, _, _ = finalize(part, k['c'], lab, L, n, cl, dtype)
    off = k['c'].to(dtype).clone()
    Pf = torch.zeros(0, k['W'].shape[0], dtype=dtype)
    if fl.numel():
        Pf, lf, rlf, mx = fix_rows(k['hh'], k['W'], k['bias'], lab, k['c'], fl, dtype)
        lse[fl], rl[fl], off[fl] = lf, rlf, mx
    ch = chunk_of(lab.numel(), L, n, cl)
    nll = (torch.zeros(n, dtype=dtype).index_add_(0, ch, rl) * cw).sum()
    return dict(fix_P=Pf, fix_lse=lse, fix_row_loss=rl, fix_off=off, fix_chunk_w=cw, fix_nll=nll)


def fix_deviations(got, ref):
    d = {k: deviation(got[k], ref[k]) for k in ('fix_lse', 'fix_row_loss', 'fix_nll')}
    if ref['fix_P'].numel():
        d['fix_P'] = exp_deviation(got['fix_P'], ref['fix_P'])
    return d


@functools.lru_cache(maxsize=None)
def chain_case(T, V, D, nchunks):
    hh, W, bias, lab, gaps = sat_case('chain', T, V, D)
    L = ROW_SHAPES[T]
    cl = chunk_len_of(L, nchunks)
    return dict(hh=hh, W=W, bias=bias, lab=lab, L=L, nchunks=nchunks, chunk_len=cl, gaps=gaps,
                ref=head_autograd(hh, W, bias, lab, L, nchunks, cl))


def chain_deviations(got, ref, lab):
    live = (lab != 0).nonzero().flatten().to(ref['dhh'].device)
    return {'chain_nll': deviation(got['nll'], ref['nll']), 'chain_dW': deviation(got['dW'], ref['dW']),
            'chain_dbias': deviation(got['dbias'], ref['dbias']),
            'chain_dhh': deviation(got['dhh'][live], ref['dhh'][live], rows=True)}


# ---------------------------------------------------------------------------------------------- recorded deviations
# Largest deviation() of the float32 evaluation of the formulas above from the float64 one, measured on the CPU by
# test_head_ref.py (which re-measures them and fails if one has moved by more than a quarter; the float32 matrix
# products are summed in whatever order the host's torch build takes, so the last digit may differ between machines)
# over the inputs the GPU tests use:
#   per kernel: KERNEL_SHAPES x NCHUNKS and LONG_LAST_CHUNK, each formula fed the float64 reference of its inputs
#               rounded to the kernel's input format; P by exp_deviation(), part and dhh per labelled row;
#   fin_*:      finalize_case (65 synthetic tiles);   fix_*: the sat_case kinds 'mixed', 'many' and 'none';
#   chain_*:    CHAIN_SHAPES x NCHUNKS with one 60-nat and one 100-nat row: head_chain in float32 with bf16 storage of
#               P, r . hh and dhh against head_autograd (the storage rounding is what these three are made of).
# The GPU bound is TOL_FACTOR times the constant; bf16 outputs (P, dhh) get half a bf16 ulp on top (bf16_within,
# bf16_exp_within). Beside each: the largest value seen from the kernels on an MI355X.
F32_DEV = {
    'label_logit':    1.7e-07,   # kernels on an MI355X: 1.7e-7 (bound 6.80e-07)
    'P':              1.5e-06,   # kernels on an MI355X: 0.997 of half an ulp + bound (bound 6.00e-06)
    'part':           1.3e-06,   # kernels on an MI355X: 1.5e-6 (bound 5.20e-06)
    'part_last':      1.7e-06,   # kernels on an MI355X: 6.5e-7 (bound 6.80e-06)
    'lse':            6.1e-08,   # kernels on an MI355X: 1.3e-7 (bound 2.44e-07)
    'row_loss':       3.3e-08,   # kernels on an MI355X: 9.6e-8 (bound 1.32e-07)
    'chunk_w':        1.9e-08,   # kernels on an MI355X: 1.9e-8 (bound 7.60e-08)
    'nll':            1.6e-07,   # kernels on an MI355X: 6.7e-8 (bound 6.40e-07)
    'fin_lse':        4.5e-08,   # kernels on an MI355X: 9.6e-8 (bound 1.80e-07)
    'fin_row_loss':   2.4e-08,   # kernels on an MI355X: 7.0e-8 (bound 9.60e-08)
    'fin_nll':        4.6e-08,   # kernels on an MI355X: 1.6e-8 (bound 1.84e-07)
    'fix_P':          3.6e-06,   # kernels on an MI355X: 0.991 of half an ulp + bound (bound 1.44e-05)
    'fix_lse':        5.3e-08,   # kernels on an MI355X: 1.0e-7 (bound 2.12e-07)
    'fix_row_loss':   2.9e-08,   # kernels on an MI355X: 8.7e-8 (bound 1.16e-07)
    'fix_nll':        1.3e-07,   # kernels on an MI355X: 1.6e-8 (bound 5.20e-07)
    'q':              1.6e-08,   # kernels on an MI355X: 1.6e-8 (bound 6.40e-08)
    'r':              3.4e-07,   # kernels on an MI355X: 3.5e-7 (bound 1.36e-06)
    'dbias_scatter':  5.7e-08,   # kernels on an MI355X: 5.7e-8 (bound 2.28e-07)
    'dhh':            1.3e-06,   # kernels on an MI355X: 0.998 of half an ulp + bound (bound 5.20e-06)
    'dW':             2.4e-06,   # kernels on an MI355X: 1.1e-6 (bound 9.60e-06)
    'rowsum':         5.2e-07,   # kernels on an MI355X: 2.0e-7 (bound 2.08e-06)
    'dtable':         3.0e-06,   # kernels on an MI355X: 3.4e-6 (f32 atomics, order varies) (bound 1.20e-05)
    'chain_nll':      5.5e-08,   # kernels on an MI355X: 5.5e-8 (bound 2.20e-07)
    'chain_dhh':      3.0e-03,   # kernels on an MI355X: 0.216 of half an ulp + bound (bound 1.20e-02)
    'chain_dW':       9.3e-03,   # kernels on an MI355X: 9.3e-3 (bound 3.72e-02)
    'chain_dbias':    2.4e-03,   # kernels on an MI355X: 2.4e-3 (bound 9.60e-03)
}


def bound(key):
    return TOL_FACTOR * F32_DEV[key]
