"""Typed wrappers over libsvae.so (include/svae.h). Tensor in, pointer out; every wrapper checks the
arguments it relies on and raises on a non-zero status. All work is enqueued on torch's current HIP
stream; nothing here synchronises."""
import ctypes
import os
from typing import NamedTuple

import torch

from . import _native as N
from ._native import lib, check, ptr, stream

bf16, f32 = torch.bfloat16, torch.float32

_gemm_desc = N.GemmDesc()


def _dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise RuntimeError('libsvae kernels need device tensors (no CPU fallback)')


def gemm(A, B, C, M, N_, K, *, a_t=False, b_t=False, lda=None, ldb=None, ldc=None, epi=N.EPI_BF16, bias=None,
         resid=None, ldr=0, aux=None, ldaux=0, alpha=1.0, splits=1, drop_p=0.0, seed=0, rot=None, rot_cols=0,
         rot_d=0, rot_seq=0, labels=None, label_logit=None, batch=1, sA=0, sB=0, sC=0, a_rowsum=None, k_weight=None,
         row_a=None, row_b=None, gather=None, ldg=0, delta=None, delta_o32=None, ld_o32=0, delta_hd=0, delta_seq=0):
    """C = epi(alpha * A . B) with A [M,K] (a_t: stored [K,M]) and B [K,N] (b_t: stored [K,N], else [N,K]).
    delta (BF16 epilogue): also the attention backward's delta = rowsum over each head of bf16(C) * delta_o32."""
    d = _fill_desc(_gemm_desc, A, B, C, M, N_, K, a_t=a_t, b_t=b_t, lda=lda, ldb=ldb, ldc=ldc, epi=epi, bias=bias,
                   resid=resid, ldr=ldr, aux=aux, ldaux=ldaux, alpha=alpha, splits=splits, drop_p=drop_p, seed=seed,
                   rot=rot, rot_cols=rot_cols, rot_d=rot_d, rot_seq=rot_seq, labels=labels, label_logit=label_logit,
                   batch=batch, sA=sA, sB=sB, sC=sC, a_rowsum=a_rowsum, k_weight=k_weight, row_a=row_a, row_b=row_b,
                   gather=gather, ldg=ldg)
    if delta is not None:
        _dev(delta, delta_o32)
        assert delta.dtype == f32 and delta_o32.dtype == f32 and delta.numel() >= M * (N_ // delta_hd)
    d.delta, d.delta_o32, d.ld_o32 = ptr(delta), ptr(delta_o32), ld_o32
    d.delta_hd, d.delta_seq = delta_hd, delta_seq
    check(lib.svae_gemm(ctypes.byref(d), stream()), 'svae_gemm')


def _fill_desc(d, A, B, C, M, N_, K, *, a_t=False, b_t=False, lda=None, ldb=None, ldc=None, epi=N.EPI_BF16,
               bias=None, resid=None, ldr=0, aux=None, ldaux=0, alpha=1.0, splits=1, drop_p=0.0, seed=0, rot=None,
               rot_cols=0, rot_d=0, rot_seq=0, labels=None, label_logit=None, batch=1, sA=0, sB=0, sC=0,
               a_rowsum=None, k_weight=None, row_a=None, row_b=None, gather=None, ldg=0):
    _dev(A, B, C)
    assert A.dtype == bf16 and B.dtype == bf16
    d.A, d.B = A.data_ptr(), B.data_ptr()
    d.lda = lda if lda is not None else (M if a_t else K)
    d.ldb = ldb if ldb is not None else (N_ if b_t else K)
    d.batch_stride_a, d.batch_stride_b = sA, sB
    d.M, d.N, d.K = M, N_, K
    d.batch, d.splits = batch, splits
    d.a_t, d.b_t = int(a_t), int(b_t)
    d.epi = epi
    d.C = ptr(C)          # None: CE statistics only (no logits stored)
    d.ldc = ldc if ldc is not None else N_
    d.batch_stride_c = sC
    d.bias = ptr(bias)
    d.resid = ptr(resid)
    d.ldr = ldr
    d.aux = ptr(aux)
    d.ldaux = ldaux
    d.alpha = alpha
    d.drop_p = drop_p
    d.seed = seed & 0xFFFFFFFFFFFFFFFF
    d.rot_tab = ptr(rot)
    d.rot_cols, d.rot_d, d.rot_seq = rot_cols, rot_d, rot_seq
    d.labels = ptr(labels)
    d.label_logit = ptr(label_logit)
    d.a_rowsum = ptr(a_rowsum)
    d.k_weight = ptr(k_weight)
    d.row_a, d.row_b = ptr(row_a), ptr(row_b)
    d.gather, d.ldg = ptr(gather), ldg
    d.delta, d.delta_o32, d.ld_o32, d.delta_hd, d.delta_seq = None, None, 0, 0, 0
    return d


_pair_desc = (N.GemmDesc(), N.GemmDesc())


def gemm_pair(g0, g1):
    """Two GEMMs in one launch (svae_gemm_pair): g0, g1 are (args, kwargs) of gemm() for two split-K slab weight
    gradients (a_t, b_t, epi F32_ATOMIC, splits >= 2, aux = slab workspace)."""
    d0 = _fill_desc(_pair_desc[0], *g0[0], **g0[1])
    d1 = _fill_desc(_pair_desc[1], *g1[0], **g1[1])
    check(lib.svae_gemm_pair(ctypes.byref(d0), ctypes.byref(d1), stream()), 'svae_gemm_pair')


def auto_splits(M, N_, K, target=512):
    """Split-K count for a dW GEMM. First choice: one round of 192..256 blocks of the 256x256 kernel (the
    library picks it at >= 192 blocks); otherwise ~`target` blocks of the 128x128 kernels."""
    t256 = -(-M // 256) * -(-N_ // 256)
    if t256 >= 192:
        return 1
    if t256 >= 4:   # fill the 256 CUs with one round of 256x256 blocks (1 per CU), K-slices >= 512
        # (the 512 x 512 dW over 32768 rows with bias row sums: 64 x 256^2 slices 50.7 us against 62.3 us for
        # 32 x 128^2 -- scripts/dw_split_probe.py with DW_RS=1, profiles/r02_dw_split_impl.log)
        s3 = min(256 // t256, max(1, K // 512))
        if t256 * s3 >= 192:
            return s3
    tiles = -(-M // 128) * -(-N_ // 128)
    if tiles >= 256 or K < 1024:
        return 1
    s = min(-(-target // tiles), K // 512)
    return max(1, s)


class DwJob(NamedTuple):
    """One weight-gradient GEMM, linear_dw's arguments: what linear_dw_pair and linear_dw_group take (a plain tuple
    of all nine in this order also does)."""
    dY: torch.Tensor
    X: torch.Tensor
    Wgrad: torch.Tensor
    rows: int
    n_out: int
    n_in: int
    ldy: int = None
    ldx: int = None
    bgrad: torch.Tensor = None


def linear_dw(dY, X, Wgrad, rows, n_out, n_in, ldy=None, ldx=None, bgrad=None):
    """Wgrad[n_out, n_in] += dY^T . X over `rows` rows (dY [rows, n_out] bf16, X [rows, n_in] bf16); with
    bgrad, also bgrad[n_out] += column sums of dY (the bias gradient, fused into the same pass over dY)."""
    s = auto_splits(n_out, n_in, rows)
    slab = _slab_workspace(s * n_out * n_in, dY.device) if s > 1 else None
    gemm(dY, X, Wgrad, n_out, n_in, rows, a_t=True, b_t=True, lda=ldy or n_out, ldb=ldx or n_in, ldc=n_in,
         epi=N.EPI_F32_ATOMIC if s > 1 else N.EPI_F32_ACC, splits=s, a_rowsum=bgrad, aux=slab)


def pair_splits(shapes):
    """Split-K counts (s0, s1) for two weight gradients launched together ((n_out, n_in, rows) each): one round of
    <= 256 256x256 blocks over both, every block's K-slice about the same length (rows / s, >= 512 rows), so a GEMM
    over many more rows than its partner is split further (C2's encoder pair of a 4096-row and a 32768-row dW: 4 and
    30 splits, 256 blocks, instead of 8 and 8, 96 blocks of which 64 ran 64 K-tiles). None when either would not
    split (then run them apart). SVAE_DW_PAIR_EQUAL=1: one common count (the round-3 rule), for A/B."""
    tiles = [-(-m // 256) * -(-n // 256) for m, n, _ in shapes]
    rows = [r for _, _, r in shapes]
    if not all(tiles):
        return None
    if os.environ.get('SVAE_DW_PAIR_EQUAL', '0') != '0':
        c = min([256 // sum(tiles)] + [r // 512 for r in rows])
        return (c, c) if c >= 2 else None
    cap = [r // 512 for r in rows]
    if min(cap) < 2:
        return None
    work = sum(t * r for t, r in zip(tiles, rows))
    slice_rows = max(512.0, work / 256.0)
    sp = [min(c, max(2, round(r / slice_rows))) for r, c in zip(rows, cap)]
    while sum(t * x for t, x in zip(tiles, sp)) > 256:
        # shorten the longest per-block slice's partner: drop a split where the slice is shortest
        i = min((k for k in range(2) if sp[k] > 2), key=lambda k: rows[k] / sp[k], default=None)
        if i is None:
            return None
        sp[i] -= 1
    # the kernel's K-slice is a multiple of 64 rows: count only the non-empty slices
    sp = [-(-r // (-(-(-(-r // x)) // 64) * 64)) for r, x in zip(rows, sp)]
    longest = max(r / x for r, x in zip(rows, sp))
    for k in range(2):   # no more slabs than the longest slice needs
        while sp[k] > 2 and rows[k] / (sp[k] - 1) <= longest:
            sp[k] -= 1
    return tuple(sp)


def linear_dw_pair(j0, j1):
    """Two linear_dw's (DwJobs) as one paired launch: each needs only ~half the split-K slices it would take alone
    to fill the chip (half the slab bytes written and reduced). Falls back to two linear_dw calls for shapes that
    would not split."""
    j0, j1 = DwJob._make(j0), DwJob._make(j1)
    sp = pair_splits([(j.n_out, j.n_in, j.rows) for j in (j0, j1)])
    if sp is None:
        linear_dw(*j0)
        linear_dw(*j1)
        return
    n0, n1 = sp[0] * j0.n_out * j0.n_in, sp[1] * j1.n_out * j1.n_in
    slab = _slab_workspace(n0 + n1, j0.dY.device)
    gs = []
    for j, aux, s in ((j0, slab[:n0], sp[0]), (j1, slab[n0:n0 + n1], sp[1])):
        gs.append(((j.dY, j.X, j.Wgrad, j.n_out, j.n_in, j.rows),
                   dict(a_t=True, b_t=True, lda=j.ldy or j.n_out, ldb=j.ldx or j.n_in, ldc=j.n_in,
                        epi=N.EPI_F32_ATOMIC, splits=s, a_rowsum=j.bgrad, aux=aux)))
    gemm_pair(*gs)


GROUP_SLICE_MAX = 16384   # rows of a grouped K slice at most: above it the split GEMMs run several rounds of these
GROUP_MIN_ROWS = 128      # a dW over fewer rows is not worth deferring (the engine launches it in place)


def group_schedule(shapes, ncu=256):
    """The fixed schedule of the grouped weight-gradient pass over GEMMs ((n_out, n_in, rows) each, in launch order):
    a list of linear_dw_group calls, each (indices, splits, slab) over the GEMMs it takes.

    Rounds of whole-K 256 x 256 tiles first, one call each: the GEMMs over the most rows, whole GEMMs in order while
    their tiles fit one per compute unit, a round kept only if it fills at least 3/4 of the chip (C2: one round, 5 1/3
    decoder layers, 256 tiles; C4 / C5, 12 layers of 108 tiles: five rounds of 252). A call never holds more whole-K
    tiles than compute units (a whole-K tile is the longest unit there is, so a partly filled second round inside a
    launch would cost a full tile time: asserted here, refused by svae_gemm_group). What no full round takes is cut
    into K slices of one common length, the work divided by the compute units, so that they fill the chip in one
    round as well (slices >= 512 rows, <= GROUP_SLICE_MAX), in the last call. The sliced GEMMs store slabs (also a
    GEMM that ends up with a single slice: slab = True)."""
    n = len(shapes)
    tiles = [-(-m // 256) * -(-k // 256) for m, k, _ in shapes]
    rows = [r for _, _, r in shapes]
    splits, slab = [0] * n, [True] * n
    rmax, calls = max(rows), []
    while True:
        used, rnd = 0, []
        for i in range(n):
            if splits[i] == 0 and rows[i] == rmax and used + tiles[i] <= ncu:
                rnd.append(i)
                used += tiles[i]
        if 4 * used < 3 * ncu:
            break
        for i in rnd:
            splits[i], slab[i] = 1, False
        calls.append(rnd)
    rest = [i for i in range(n) if splits[i] == 0]
    if rest:
        units = lambda sl: sum(tiles[i] * -(-rows[i] // sl) for i in rest)   # noqa: E731
        work = sum(tiles[i] * rows[i] for i in rest)
        sl = min(GROUP_SLICE_MAX, max(512, -(-work // (ncu * 64)) * 64))
        while sl < GROUP_SLICE_MAX and units(sl) > ncu:
            sl += 64
        for i in rest:
            s = -(-rows[i] // sl)
            kchunk = -(-(-(-rows[i] // s)) // 64) * 64   # the kernel's slice: a multiple of 64 rows
            splits[i] = -(-rows[i] // kchunk)            # (only the non-empty slices)
        if calls:
            calls[-1] = calls[-1] + rest
        else:
            calls.append(rest)
    for c in calls:
        assert sum(tiles[i] for i in c if not slab[i]) <= ncu, 'a second round of whole-K tiles in one launch'
    return [(c, [splits[i] for i in c], [slab[i] for i in c]) for c in calls]


class DwGroupState:
    """What svae_gemm_group keeps between calls, owned by the caller: the descriptor array, the device parameter
    table and the host copy of it (the table is uploaded only when its contents change)."""

    def __init__(self, device):
        self.device, self.n = device, 0

    def ensure(self, n):
        if n > self.n:
            self.n = max(n, 2 * self.n)
            self.bytes = lib.svae_gemm_group_table_bytes(min(self.n, N.GROUP_MAX))
            self.descs = (N.GemmDesc * self.n)()
            self.table = torch.empty(self.bytes, dtype=torch.uint8, device=self.device)
            self.host = ctypes.create_string_buffer(self.bytes)   # (zeroed)


def linear_dw_group(jobs, splits, state, slab=None, max_blocks=0):
    """linear_dw for every job (DwJobs) in one grouped pass
    (svae_gemm_group): the jobs with slab[i] false (default: splits[i] == 1) accumulate whole-K tiles straight into
    Wgrad in one launch; the others store splits[i] K slices into slabs in a second launch, added into Wgrad in slice
    order by one reduction launch. max_blocks > 0 caps the blocks per launch (they then walk several tiles each)."""
    jobs = [DwJob._make(j) for j in jobs]
    n = len(jobs)
    if n == 0:
        return
    if n > N.GROUP_MAX:
        raise RuntimeError(f'linear_dw_group: {n} GEMMs (at most {N.GROUP_MAX})')
    slab = [s > 1 for s in splits] if slab is None else slab
    need = sum(s * j.n_out * j.n_in for j, s, sb in zip(jobs, splits, slab) if sb)
    ws = _slab_workspace(need, jobs[0].dY.device) if need else None
    state.ensure(n)
    off = 0
    for i, (j, s, sb) in enumerate(zip(jobs, splits, slab)):
        aux = None
        if sb:
            aux = ws[off:off + s * j.n_out * j.n_in]
            off += s * j.n_out * j.n_in
        elif s != 1:
            raise RuntimeError('linear_dw_group: a GEMM without a slab has one split')
        _fill_desc(state.descs[i], j.dY, j.X, j.Wgrad, j.n_out, j.n_in, j.rows, a_t=True, b_t=True,
                   lda=j.ldy or j.n_out, ldb=j.ldx or j.n_in, ldc=j.n_in,
                   epi=N.EPI_F32_ATOMIC if sb else N.EPI_F32_ACC, splits=s, a_rowsum=j.bgrad, aux=aux)
    check(lib.svae_gemm_group(state.descs, n, max_blocks, state.table.data_ptr(), state.host, state.bytes, stream()),
          'svae_gemm_group')


_slabs = {}


def _slab_workspace(n, device):
    """f32 split-K slab workspace (grown on demand, reused stream-ordered by every dW GEMM)."""
    t = _slabs.get(device)
    if t is None or t.numel() < n:
        t = torch.empty(n, dtype=torch.float32, device=device)
        _slabs[device] = t
    return t


def resid_ln_fwd(x, y, h, rows, D, *, w=None, b=None, mean=None, rstd=None, xo=None, drop_p=0.0, seed=0, zrows=None,
                 zmod=0):
    """svae_resid_ln_fwd: v = x + dropout(y) (or zrows[r // zmod] on rows r % zmod == 0); xo = v; h = LN(v) (or bf16(v)
    without w / b)."""
    _dev(h, *(t for t in (x, y, xo, zrows, w, b, mean, rstd) if t is not None))
    assert h.dtype == bf16 and (y is None or y.dtype in (bf16, f32)) and (x is None or x.dtype == f32)
    # the kernel walks x / xo / zrows / h as dense rows of D elements (y has its own leading dimension)
    for t in (x, xo, zrows, h, w, b):
        assert t is None or t.is_contiguous(), 'resid_ln_fwd: x, xo, zrows, h, w, b must be contiguous'
    check(lib.svae_resid_ln_fwd(ptr(x), ptr(y), 1 if y is not None and y.dtype == bf16 else 0,
                                y.stride(0) if y is not None else 0, float(drop_p), int(seed) & (2 ** 64 - 1),
                                ptr(zrows), int(zmod), ptr(w), ptr(b), ptr(xo), h.data_ptr(), ptr(mean), ptr(rstd), rows,
                                D, stream()), 'svae_resid_ln_fwd')


def layernorm_fwd(x, w, b, y, mean, rstd, rows, D):
    _dev(x, w, b, y, mean, rstd)
    check(lib.svae_layernorm_fwd(x.data_ptr(), 0 if x.dtype == f32 else 1, w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                 mean.data_ptr(), rstd.data_ptr(), rows, D, stream()), 'svae_layernorm_fwd')


def layernorm_bwd(dy, x, w, mean, rstd, dres, dx, dx_bf, wgrad2, rows, D, part_ws, bf_drop=None, zsplice=None,
                  defer=None):
    """dx = dres + LN'(dy); wgrad2 (the adjacent [weight | bias] grads, 2D floats) += sum of affine grads.
    bf_drop = (p, seed, zero_mod): the bf16 copy dx_bf carries the next consumer's dropout backward and position-0
    zeroing (svae_layernorm_bwd_drop), replacing a dropout_bwd_cast pass over dx. zsplice = (L, zrow f32 | None,
    zrow_bf bf16 | None): rows r % L == 0 of dx go to zrow[r / L] / zrow_bf and are zeroed in dx (extract_rows)."""
    nblk = lib.svae_layernorm_nblk(rows)
    part = part_ws[: nblk * 2 * D]
    if bf_drop is None and zsplice is None:
        check(lib.svae_layernorm_bwd(dy.data_ptr(), x.data_ptr(), 0 if x.dtype == f32 else 1, w.data_ptr(),
                                     mean.data_ptr(), rstd.data_ptr(), ptr(dres), dx.data_ptr(), ptr(dx_bf),
                                     part.data_ptr(), nblk, rows, D, 0, stream()), 'svae_layernorm_bwd')
    else:
        p, seed, zmod = bf_drop if bf_drop is not None else (0.0, 0, 0)
        zm, zrow, zrow_bf = zsplice if zsplice is not None else (0, None, None)
        check(lib.svae_layernorm_bwd_drop(dy.data_ptr(), x.data_ptr(), 0 if x.dtype == f32 else 1, w.data_ptr(),
                                          mean.data_ptr(), rstd.data_ptr(), ptr(dres), dx.data_ptr(), ptr(dx_bf),
                                          part.data_ptr(), nblk, rows, D, int(zm), float(p),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF, int(zmod), ptr(zrow), ptr(zrow_bf),
                                          stream()), 'svae_layernorm_bwd_drop')
    if defer is not None:   # the caller sums the partials later, batched with other LayerNorms (colsum_multi)
        defer.append((part, nblk, 2 * D, 2 * D, wgrad2))
    else:
        colsum(part, nblk, 2 * D, 2 * D, wgrad2, accumulate=True)


def layernorm_bwd_gelu(dy, x, w, mean, rstd, gp, out_bf, wgrad2, rows, D, part_ws, defer=None):
    """out_bf = bf16(LN'(dy) * gp) (svae_layernorm_bwd_gelu: the head's LayerNorm backward with the GELU backward
    of the linear before it); wgrad2 += the affine grads (or deferred, as layernorm_bwd)."""
    nblk = lib.svae_layernorm_nblk(rows)
    part = part_ws[: nblk * 2 * D]
    check(lib.svae_layernorm_bwd_gelu(dy.data_ptr(), x.data_ptr(), 0 if x.dtype == f32 else 1, w.data_ptr(),
                                      mean.data_ptr(), rstd.data_ptr(), gp.data_ptr(), out_bf.data_ptr(),
                                      part.data_ptr(), nblk, rows, D, stream()), 'svae_layernorm_bwd_gelu')
    if defer is not None:
        defer.append((part, nblk, 2 * D, 2 * D, wgrad2))
    else:
        colsum(part, nblk, 2 * D, 2 * D, wgrad2, accumulate=True)


def _ptrs(ts):
    return (ctypes.c_void_p * N.LN_MULTI_MAX)(*[t.data_ptr() for t in ts])


def layernorm_fwd_multi(x, ws, bs, ys, mean, rstd, rows, D):
    """svae_layernorm_fwd_multi: ys[j] = bf16(LN(x) * ws[j] + bs[j]) for n <= LN_MULTI_MAX affines of one f32 x
    (the encoder middle layers' context LayerNorms), one pass; the shared mean / rstd."""
    n = len(ys)
    assert 0 < n <= N.LN_MULTI_MAX and len(ws) == n and len(bs) == n and x.dtype == f32
    _dev(x, mean, rstd, *ws, *bs, *ys)
    check(lib.svae_layernorm_fwd_multi(x.data_ptr(), _ptrs(ws), _ptrs(bs), _ptrs(ys), n, mean.data_ptr(),
                                       rstd.data_ptr(), rows, D, stream()), 'svae_layernorm_fwd_multi')


def layernorm_bwd_multi(dys, x, ws, mean, rstd, dres, dx, wgrads, rows, D, part_ws, defer=None):
    """svae_layernorm_bwd_multi: dx = dres + sum_j LN'_j(dys[j]) (dres may be dx); wgrads[j] (the adjacent
    [weight | bias] grads of LayerNorm j) += its affine grads, summed from part_ws (n slabs) now or by the caller's
    deferred colsum_multi (defer, as layernorm_bwd)."""
    n = len(dys)
    assert 0 < n <= N.LN_MULTI_MAX and len(ws) == n and len(wgrads) == n and x.dtype == f32
    _dev(x, mean, rstd, dx, *dys, *ws)
    nblk = lib.svae_layernorm_nblk(rows)
    parts = [part_ws[j * nblk * 2 * D:(j + 1) * nblk * 2 * D] for j in range(n)]
    assert parts[-1].numel() == nblk * 2 * D
    check(lib.svae_layernorm_bwd_multi(_ptrs(dys), x.data_ptr(), _ptrs(ws), mean.data_ptr(), rstd.data_ptr(),
                                       ptr(dres), dx.data_ptr(), _ptrs(parts), nblk, n, rows, D, stream()),
          'svae_layernorm_bwd_multi')
    for part, wg in zip(parts, wgrads):
        if defer is not None:
            defer.append((part, nblk, 2 * D, 2 * D, wg))
        else:
            colsum(part, nblk, 2 * D, 2 * D, wg, accumulate=True)


_colsum_segs = (N.ColsumSeg * N.COLSUM_MAX)()


def colsum_multi(segs):
    """svae_colsum_multi: [(inp f32, rows, cols, ld, out f32)] (<= 8), each out += column sums of its inp."""
    assert 0 < len(segs) <= N.COLSUM_MAX
    for i, (inp, rows, cols, ld, out) in enumerate(segs):
        _dev(inp, out)
        assert inp.dtype == f32 and out.dtype == f32
        _colsum_segs[i].inp, _colsum_segs[i].out = inp.data_ptr(), out.data_ptr()
        _colsum_segs[i].ld, _colsum_segs[i].rows, _colsum_segs[i].cols = ld, rows, cols
    check(lib.svae_colsum_multi(ctypes.addressof(_colsum_segs), len(segs), stream()), 'svae_colsum_multi')


def colsum(inp, rows, cols, ld, out, accumulate=True):
    check(lib.svae_colsum(inp.data_ptr(), 0 if inp.dtype == f32 else 1, rows, cols, ld, out.data_ptr(),
                          int(accumulate), stream()), 'svae_colsum')


_attn_desc = N.AttnDesc()


def attention(q, k, v, o, lse, *, B, H, Lq, Lk, hd, sq, sk, sv, so, bq, bk, bv, bo, key_pad=None, causal=False,
              window=0, scale=None, backward=False, dout=None, sdo=0, bdo=0, delta=None, dq=None, bdq=0, dk=None, dv=None,
              sdk=0, sdv=0, bdk=0, bdv=0, rot=None, rot_d=0, o32=None, so32=0, bo32=0, dq_part=None, dq_bf=None,
              ldq_bf=0, delta_ready=False, o_lo=None, so_lo=0, bo_lo=0):
    """Forward (o, lse[, o32 | o_lo]) or backward (dk, dv and dq: f32 `dq` or bf16 `dq_bf` with inverse rotary).
    o_lo: bf16 residual O - bf16(O) (written by the forward, read by the backward's delta pass; the 2-byte alternative
    to the f32 copy o32).
    dq_part: f32 workspace of attn_dq_part_elems(...) floats (allocated here when not given).
    window > 0 (causal): SparseAttention's sliding window of `window` 32-key blocks + the [CLS] block."""
    d = _attn_desc
    d.q, d.k, d.v, d.o = q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr()
    d.sq, d.sk, d.sv, d.so, d.bq, d.bk, d.bv, d.bo = sq, sk, sv, so, bq, bk, bv, bo
    d.key_pad = ptr(key_pad)
    d.lse = lse.data_ptr()
    d.B, d.H, d.Lq, d.Lk, d.hd, d.causal = B, H, Lq, Lk, hd, int(causal)
    d.window = int(window)
    d.delta_ready = int(bool(delta_ready))
    d.scale = hd ** -0.5 if scale is None else scale
    d.o32, d.so32, d.bo32 = ptr(o32), so32, bo32
    d.o_lo, d.so_lo, d.bo_lo = ptr(o_lo), so_lo, bo_lo
    if backward:
        d.fwd_ws, d.fwd_ws_elems = None, 0
        d.dout, d.sdo, d.bdo = dout.data_ptr(), sdo, bdo
        d.delta, d.bdq = delta.data_ptr(), bdq
        d.dk, d.dv, d.sdk, d.sdv, d.bdk, d.bdv = dk.data_ptr(), dv.data_ptr(), sdk, sdv, bdk, bdv
        d.rot_tab, d.rot_d = ptr(rot), rot_d
        if dq_part is None:
            dq_part = torch.empty(attn_dq_part_elems(B, H, Lq, Lk, hd, window), device=q.device, dtype=torch.float32)
        assert dq_part.numel() >= attn_dq_part_elems(B, H, Lq, Lk, hd, window) and dq_part.dtype == torch.float32
        d.dq_part, d.dq_bf, d.ldq_bf = dq_part.data_ptr(), ptr(dq_bf), ldq_bf
        d.dq = ptr(dq)
        check(lib.svae_attn_bwd(ctypes.byref(d), stream()), 'svae_attn_bwd')
    else:
        d.dout = None
        # few queries over a long key sequence: the split-KV workspace (the library decides; 0 floats = one pass)
        n = lib.svae_attn_fwd_ws_elems(B, H, Lq, Lk, hd, int(causal), int(window))
        if n > 0:
            ws = _fwd_workspace(n, q.device)
            d.fwd_ws, d.fwd_ws_elems = ws.data_ptr(), ws.numel()
        else:
            d.fwd_ws, d.fwd_ws_elems = None, 0
        check(lib.svae_attn_fwd(ctypes.byref(d), stream()), 'svae_attn_fwd')


_fwd_ws = {}


def _fwd_workspace(n, device):
    """f32 workspace of the split-KV attention forward (grown on demand, reused stream-ordered)."""
    t = _fwd_ws.get(device)
    if t is None or t.numel() < n:
        t = torch.empty(n, dtype=torch.float32, device=device)
        _fwd_ws[device] = t
    return t


def attn_dq_part_elems(B, H, Lq, Lk, hd, window=0):
    """Floats of the backward's dQ-partial workspace for this shape (window > 0: the sliding window's compact band
    planes)."""
    return lib.svae_attn_dq_part_elems_w(B, H, Lq, Lk, hd, int(window))


def dq_finalize(dq, out, ldo, rows, D, rot=None, seq=0):
    check(lib.svae_dq_finalize(dq.data_ptr(), out.data_ptr(), ldo, rows, D, ptr(rot), seq, stream()),
          'svae_dq_finalize')


def embedding_fwd(ids, table, out, rows, D, out2=None):
    if out2 is not None:
        _dev(ids, table, out, out2)
        check(lib.svae_embedding_fwd_dual(ids.data_ptr(), table.data_ptr(), out.data_ptr(), out2.data_ptr(), rows, D,
                                          stream()), 'svae_embedding_fwd_dual')
        return
    check(lib.svae_embedding_fwd(ids.data_ptr(), table.data_ptr(), out.data_ptr(), None, rows, D, stream()),
          'svae_embedding_fwd')


def embedding_bwd(ids, dout, dtable, rows, D):
    check(lib.svae_embedding_bwd(ids.data_ptr(), dout.data_ptr(), dtable.data_ptr(), rows, D, stream()),
          'svae_embedding_bwd')


def reparam_fwd(stats, eps, seed, ntok, z, z_bf, eps_out, raw_kl, kl_out, B, Z):
    check(lib.svae_reparam_kl_fwd(stats.data_ptr(), ptr(eps), seed & 0xFFFFFFFFFFFFFFFF, ntok.data_ptr(),
                                  z.data_ptr(), ptr(z_bf), ptr(eps_out), raw_kl.data_ptr(), kl_out.data_ptr(), B, Z,
                                  stream()), 'svae_reparam_kl_fwd')


def reparam_bwd(stats, eps, dz, ntok, gkl, dstats, B, Z):
    check(lib.svae_reparam_kl_bwd(stats.data_ptr(), eps.data_ptr(), ptr(dz), ntok.data_ptr(), gkl.data_ptr(),
                                  dstats.data_ptr(), B, Z, stream()), 'svae_reparam_kl_bwd')


def ce_red_ws(device, nchunks):
    """f32 workspace of the chunked-CE reductions (grown on demand)."""
    n = max(1024, lib.svae_ce_red_ws_elems(nchunks))
    t = _ce_red.get(device)
    if t is None or t.numel() < n:
        t = _ce_red[device] = torch.empty(n, dtype=f32, device=device)
    return t


_ce_red = {}


def ce_finalize(part, ntile, label_logit, labels, rows, seq, nchunks, chunk_len, lse, row_loss, chunk_w, nll):
    assert chunk_w.numel() >= nchunks and chunk_w.dtype == f32
    red = ce_red_ws(part.device, nchunks)
    check(lib.svae_ce_finalize(part.data_ptr(), ntile, label_logit.data_ptr(), labels.data_ptr(), rows, seq,
                               nchunks, chunk_len, lse.data_ptr(), row_loss.data_ptr(), chunk_w.data_ptr(),
                               nll.data_ptr(), red.data_ptr(), stream()), 'svae_ce_finalize')


def ce_weighted_nll(row_loss, labels, tok_w, rows, seq, nchunks, chunk_len, out):
    """Chunked mean of row_loss with per-target weights tok_w [V] (F.cross_entropy(weight=...)), into out[0]."""
    _dev(row_loss, labels, tok_w, out)
    assert tok_w.dtype == f32 and tok_w.is_contiguous()
    red = ce_red_ws(row_loss.device, nchunks)
    check(lib.svae_ce_weighted_nll(row_loss.data_ptr(), labels.data_ptr(), tok_w.data_ptr(), rows, seq, nchunks,
                                   chunk_len, out.data_ptr(), red.data_ptr(), stream()), 'svae_ce_weighted_nll')


def ce_chunking(B, L, V, chunk_numel=2 ** 30):
    """robust_cross_entropy's split (language_model.py:163-170) of logits [B, L-1, V]: cdiv(numel, 2^30) chunks
    requested along the sequence; torch.chunk makes ceil((L-1)/chunks)-long pieces, so fewer may result.
    Returns (nchunks, chunk_len)."""
    chunks = -(-(B * (L - 1) * V) // chunk_numel)
    chunk_len = -(-(L - 1) // chunks)
    return -(-(L - 1) // chunk_len), chunk_len


def ce_label_logit(hh, W, bias, labels, rows, D, out):
    _dev(hh, W, labels, out)
    check(lib.svae_ce_label_logit(hh.data_ptr(), hh.stride(0), W.data_ptr(), W.stride(0), ptr(bias), labels.data_ptr(),
                                  rows, D, out.data_ptr(), stream()), 'svae_ce_label_logit')


def ce_prob_finalize(part, ntile, row_off, labels, rows, seq, nchunks, chunk_len, lse, row_loss, chunk_w, nll,
                     fix=None):
    """fix = (hh, W, bias, P, sat_ws): recompute the rows whose P saturated (svae_ce_prob_finalize_fix); sat_ws
    int32 [1 + rows] holds their count (and rows) afterwards."""
    assert chunk_w.numel() >= nchunks and chunk_w.dtype == f32
    red = ce_red_ws(part.device, nchunks)
    if fix is None:
        check(lib.svae_ce_prob_finalize(part.data_ptr(), ntile, row_off.data_ptr(), labels.data_ptr(), rows, seq,
                                        nchunks, chunk_len, lse.data_ptr(), row_loss.data_ptr(), chunk_w.data_ptr(),
                                        nll.data_ptr(), red.data_ptr(), stream()), 'svae_ce_prob_finalize')
        return
    hh, W, bias, P, sat = fix
    _dev(hh, W, P, sat)
    assert sat.dtype == torch.int32 and sat.numel() >= rows + 1 and P.shape[0] >= rows
    check(lib.svae_ce_prob_finalize_fix(part.data_ptr(), ntile, row_off.data_ptr(), labels.data_ptr(), rows, seq,
                                        nchunks, chunk_len, lse.data_ptr(), row_loss.data_ptr(), chunk_w.data_ptr(),
                                        nll.data_ptr(), red.data_ptr(), hh.data_ptr(), hh.stride(0), W.data_ptr(),
                                        W.stride(0), ptr(bias), P.data_ptr(), P.stride(0), W.shape[0], hh.shape[1],
                                        sat.data_ptr(), stream()), 'svae_ce_prob_finalize_fix')


def ce_prob_bwd_prep(hh, lse, row_off, chunk_w, labels, gscale, rows, seq, nchunks, chunk_len, D, hh_out, r_out,
                     q_out, dbias=None):
    _dev(hh, lse, row_off, chunk_w, labels, gscale, hh_out, r_out, q_out)
    check(lib.svae_ce_prob_bwd_prep(hh.data_ptr(), hh.stride(0), lse.data_ptr(), row_off.data_ptr(),
                                    chunk_w.data_ptr(), labels.data_ptr(), gscale.data_ptr(), rows, seq, nchunks,
                                    chunk_len, D, hh_out.data_ptr(), r_out.data_ptr(), q_out.data_ptr(), ptr(dbias),
                                    stream()), 'svae_ce_prob_bwd_prep')


def embedding_bwd_ce(ids, dout, dtable, rows, D, seq, hh, q):
    check(lib.svae_embedding_bwd_ce(ids.data_ptr(), dout.data_ptr(), dtable.data_ptr(), rows, D, seq, hh.data_ptr(),
                                    q.data_ptr(), stream()), 'svae_embedding_bwd_ce')


def mutual_info(stats, kl, B, Z, seed, out, ws, eps=None, S=10):
    """out[0] = kl[0] - marginal_kl (math_utils.py:51-58) over S posterior samples; eps [S, B, Z] or in-kernel."""
    _dev(stats, kl, out, ws)
    assert ws.numel() >= 2 * S * B
    check(lib.svae_mutual_info(stats.data_ptr(), ptr(eps), seed & 0xFFFFFFFFFFFFFFFF, kl.data_ptr(), B, Z, S,
                               ws.data_ptr(), out.data_ptr(), stream()), 'svae_mutual_info')


def ce_seq_logprob(part, ntile, label_logit, labels, rows, seq, out):
    _dev(part, label_logit, labels, out)
    assert out.dtype == f32 and out.numel() == rows // seq and out.is_contiguous()
    check(lib.svae_ce_seq_logprob(part.data_ptr(), ntile, label_logit.data_ptr(), labels.data_ptr(), rows, seq,
                                  out.data_ptr(), stream()), 'svae_ce_seq_logprob')


def ce_grad(logits, ld, lse, chunk_w, labels, gscale, rows, V, seq, nchunks, chunk_len, dbias=None):
    check(lib.svae_ce_grad(logits.data_ptr(), ld, lse.data_ptr(), chunk_w.data_ptr(), labels.data_ptr(),
                           gscale.data_ptr(), ptr(dbias), rows, V, seq, nchunks, chunk_len, stream()), 'svae_ce_grad')


def prep_tokens(ids, pad, B, L, ids32, labels, padm=None, ntok=None, ntok_out=None):
    """svae_prep_tokens: ids int64 [B, L] -> ids32, next-token labels (0 at each sequence's end), the uint8
    padding mask (pad True: ids == 0; a bool tensor: copied; None / False: none) and the ntok copy."""
    assert ids.dtype == torch.int64 and ids.is_contiguous() and ids.numel() == B * L
    mode = 0 if pad is None or pad is False else (1 if pad is True else 2)
    if mode == 2:
        assert pad.dtype == torch.bool and pad.is_contiguous() and pad.numel() == B * L
    if ntok is not None:
        assert ntok.dtype == torch.int64 and ntok.is_contiguous() and ntok.numel() == B
    _dev(ids, ids32, labels)
    check(lib.svae_prep_tokens(ids.data_ptr(), pad.data_ptr() if mode == 2 else None, mode, B, L, ids32.data_ptr(),
                               labels.data_ptr(), ptr(padm), ptr(ntok), ptr(ntok_out), stream()), 'svae_prep_tokens')


def step_scalars(kl_weight, nll=None, kl=None, loss=None, gloss=None, gs=None):
    """svae_step_scalars: loss = nll + kl_weight * kl and / or gs = (gloss, gloss * kl_weight), f32 on the device."""
    for t in (nll, kl, loss, gloss, gs):
        assert t is None or (t.is_cuda and t.dtype == f32)
    check(lib.svae_step_scalars(ptr(nll), ptr(kl), ptr(gloss), float(kl_weight), ptr(loss), ptr(gs), stream()),
          'svae_step_scalars')


def dropout_bwd_cast(g, out, p, seed, rows, cols, ld_in=None):
    check(lib.svae_dropout_bwd_cast(g.data_ptr(), out.data_ptr(), p, seed & 0xFFFFFFFFFFFFFFFF, rows * cols, cols,
                                    ld_in or cols, stream()), 'svae_dropout_bwd_cast')


def cast_bf16(x, out, n=None):
    check(lib.svae_cast_bf16(x.data_ptr(), out.data_ptr(), n if n is not None else x.numel(), stream()),
          'svae_cast_bf16')


def transpose_blocks(src, dst, table, nblocks, total_tiles):
    check(lib.svae_transpose_blocks(src.data_ptr(), dst.data_ptr(), table.data_ptr(), nblocks, total_tiles, stream()),
          'svae_transpose_blocks')


def gelu_bwd(dx, gp, out, n):
    check(lib.svae_gelu_bwd(dx.data_ptr(), gp.data_ptr(), out.data_ptr(), n, stream()), 'svae_gelu_bwd')


def extract_rows(x, ld, rows, mod, D, out):
    check(lib.svae_extract_rows(x.data_ptr(), ld, rows, mod, D, out.data_ptr(), stream()), 'svae_extract_rows')


def zproj_bwd(g, z, W, dW, db, dz, B, d, Z):
    """z_projections backward (svae_zproj_bwd): dW += g^T z, db += sum_b g, dz += g W (g f32 [B, d]; z, W bf16)."""
    _dev(g, z, W, dW, db, dz)
    assert g.dtype == f32 and z.dtype == bf16 and W.dtype == bf16 and dW.dtype == f32 and dz.dtype == f32
    check(lib.svae_zproj_bwd(g.data_ptr(), z.data_ptr(), W.data_ptr(), dW.data_ptr(), db.data_ptr(), dz.data_ptr(),
                             B, d, Z, stream()), 'svae_zproj_bwd')


_zfwd_segs = (N.ZprojFwdSeg * N.ZPROJ_MAX)()


def zproj_fwd_multi(segs, z, B, d, Z):
    """svae_zproj_fwd_multi: segs = [(W bf16 [d, Z], bias f32 [d], out f32 [B, d])] (<= 32): out = z W^T + bias."""
    assert 0 < len(segs) <= N.ZPROJ_MAX
    _dev(z)
    assert z.dtype == bf16 and z.is_contiguous()
    for i, (W, bias, out) in enumerate(segs):
        _dev(W, bias, out)
        assert W.dtype == bf16 and bias.dtype == f32 and out.dtype == f32 and out.is_contiguous()
        _zfwd_segs[i].W, _zfwd_segs[i].bias, _zfwd_segs[i].out = W.data_ptr(), bias.data_ptr(), out.data_ptr()
    check(lib.svae_zproj_fwd_multi(ctypes.addressof(_zfwd_segs), len(segs), z.data_ptr(), B, d, Z, stream()),
          'svae_zproj_fwd_multi')


def layernorm_fwd_z(x, zrows, zmod, w, b, y, mean, rstd, rows, D):
    """svae_layernorm_fwd_z: LayerNorm forward of f32 x whose rows r % zmod == 0 come from zrows (and are written into x)."""
    _dev(x, zrows, w, b, y, mean, rstd)
    assert x.dtype == f32 and zrows.dtype == f32 and x.is_contiguous() and zrows.is_contiguous()
    check(lib.svae_layernorm_fwd_z(x.data_ptr(), zrows.data_ptr(), zmod, w.data_ptr(), b.data_ptr(), y.data_ptr(),
                                   mean.data_ptr(), rstd.data_ptr(), rows, D, stream()), 'svae_layernorm_fwd_z')


_zproj_segs = (N.ZprojSeg * N.ZPROJ_MAX)()


def zproj_bwd_multi(segs, z, dz, B, d, Z):
    """svae_zproj_bwd_multi: segs = [(g f32 [B, d], W bf16 [d, Z], dW f32, db f32)] (<= 32) sharing z and dz; the
    same results as zproj_bwd per segment in list order."""
    assert 0 < len(segs) <= N.ZPROJ_MAX
    _dev(z, dz)
    assert z.dtype == bf16 and dz.dtype == f32
    for i, (g, W, dW, db) in enumerate(segs):
        _dev(g, W, dW, db)
        assert g.dtype == f32 and W.dtype == bf16 and dW.dtype == f32 and db.dtype == f32
        _zproj_segs[i].g, _zproj_segs[i].W = g.data_ptr(), W.data_ptr()
        _zproj_segs[i].dW, _zproj_segs[i].db = dW.data_ptr(), db.data_ptr()
    check(lib.svae_zproj_bwd_multi(ctypes.addressof(_zproj_segs), len(segs), z.data_ptr(), dz.data_ptr(), B, d, Z,
                                   stream()), 'svae_zproj_bwd_multi')


def sumsq(g, n, part):
    check(lib.svae_sumsq(g.data_ptr(), n, part.data_ptr(), part.numel(), stream()), 'svae_sumsq')


def clip_grad(g, n, part, max_norm, norm_out=None):
    check(lib.svae_clip_grad(g.data_ptr(), n, part.data_ptr(), part.numel(), float(max_norm), ptr(norm_out), stream()),
          'svae_clip_grad')


def radam(p, pbf, g, m, v, n, part, scal, norm_out):
    check(lib.svae_radam(p.data_ptr(), ptr(pbf), g.data_ptr(), m.data_ptr(), v.data_ptr(), n, part.data_ptr(),
                         part.numel(), scal.data_ptr(), ptr(norm_out), stream()), 'svae_radam')


# ---- fp32 kernel mode (argmax-reconstruction parity)
def gemm_f32(A, W, C, M, N_, K_, *, lda=None, ldw=None, ldc=None, epi=N.EPI_F32, bias=None, resid=None, ldr=0,
             rot=None, rot_cols=0, rot_d=0, rot_seq=0):
    _dev(A, W, C)
    check(lib.svae_gemm_f32(A.data_ptr(), W.data_ptr(), C.data_ptr(), M, N_, K_, lda or K_, ldw or K_, ldc or N_,
                            ptr(bias), ptr(resid), ldr, epi, ptr(rot), rot_cols, rot_d, rot_seq, stream()),
          'svae_gemm_f32')


def attention_f32(q, k, v, o, *, B, H, Lq, Lk, hd, sq, sk, sv, so, bq, bk, bv, bo, key_pad=None, causal=False,
                  window=0):
    check(lib.svae_attn_fwd_f32(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), sq, sk, sv, so, bq, bk, bv, bo,
                                ptr(key_pad), B, H, Lq, Lk, hd, int(causal), int(window), hd ** -0.5, stream()),
          'svae_attn_fwd_f32')


def layernorm_fwd_f32(x, w, b, y, rows, D):
    check(lib.svae_layernorm_fwd_f32(x.data_ptr(), w.data_ptr(), b.data_ptr(), y.data_ptr(), rows, D, stream()),
          'svae_layernorm_fwd_f32')


# ---- autoregressive decoding (f32; positions from the device scalar `cur`)
def dec_linear(X, W, Y, M, N_, K_, *, bias=None, resid=None, epi=N.EPI_F32, rot=None, rot_cols=0, rot_d=0, cur=None,
               ldx=None, ldw=None, ldy=None, ldr=None, part=None):
    """part: optional f32 workspace for split-K partials (the library splits narrow outputs when it fits)."""
    _dev(X, W, Y)
    assert X.dtype == f32 and W.dtype == f32 and Y.dtype == f32
    check(lib.svae_dec_linear(X.data_ptr(), ldx or K_, W.data_ptr(), ldw or K_, ptr(bias), Y.data_ptr(), ldy or N_,
                              ptr(resid), ldr or N_, M, N_, K_, epi, ptr(rot), rot_cols, rot_d, ptr(cur), ptr(part),
                              part.numel() if part is not None else 0, stream()), 'svae_dec_linear')


def dec_attn(qkv, kc, vc, O, B, H, hd, T, cur, window, scale=None, ldq=None, ldo=None):
    _dev(qkv, kc, vc, O, cur)
    check(lib.svae_dec_attn(qkv.data_ptr(), ldq or 3 * H * hd, kc.data_ptr(), vc.data_ptr(), B, H, hd, T,
                            cur.data_ptr(), window, hd ** -0.5 if scale is None else scale, O.data_ptr(),
                            ldo or H * hd, stream()), 'svae_dec_attn')


def dec_embed(out_ids, T, cur, table, x, B, D):
    assert out_ids.dtype == torch.int64
    check(lib.svae_dec_embed(out_ids.data_ptr(), T, cur.data_ptr(), table.data_ptr(), x.data_ptr(), B, D, stream()),
          'svae_dec_embed')


def dec_penalty(logits, rows, row_map, out_ids, T, cur, live, penalty):
    check(lib.svae_dec_penalty(logits.data_ptr(), logits.stride(0), rows, ptr(row_map), out_ids.data_ptr(), T,
                               cur.data_ptr(), ptr(live), penalty, stream()), 'svae_dec_penalty')


def dec_sample(logits, V, rows, row_map, out_ids, T, cur, live, end_token, temperature, top_k, top_p, seed,
               live_count=None):
    check(lib.svae_dec_sample(logits.data_ptr(), logits.stride(0), V, rows, ptr(row_map), out_ids.data_ptr(), T,
                              cur.data_ptr(), ptr(live), end_token, temperature, top_k, top_p,
                              seed & 0xFFFFFFFFFFFFFFFF, ptr(live_count), stream()), 'svae_dec_sample')


def dec_advance(cur):
    check(lib.svae_dec_advance(cur.data_ptr(), stream()), 'svae_dec_advance')


# ---- streaming bulk sampling (f32; one position per slot: pos int32 [S], 0 = idle, < 0 = finished)
def _slot_state(S, *ts):
    _dev(*ts)
    for t in ts:
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= S


def slot_linear(X, W, Y, S, N_, K_, *, rot, rot_cols, rot_d, pos, bias=None, resid=None, ldx=None, ldw=None,
                ldy=None, ldr=None, part=None):
    """svae_slot_linear: dec_linear with the rotary epilogue at position pos[m]-1 of each row."""
    _dev(X, W, Y, rot)
    _slot_state(S, pos)
    assert X.dtype == f32 and W.dtype == f32 and Y.dtype == f32
    check(lib.svae_slot_linear(X.data_ptr(), ldx or K_, W.data_ptr(), ldw or K_, ptr(bias), Y.data_ptr(), ldy or N_,
                               ptr(resid), ldr or N_, S, N_, K_, rot.data_ptr(), rot_cols, rot_d, pos.data_ptr(),
                               ptr(part), part.numel() if part is not None else 0, stream()), 'svae_slot_linear')


def slot_attn(qkv, kc, vc, O, S, H, hd, T, pos, window, scale=None, ldq=None, ldo=None):
    _dev(qkv, kc, vc, O)
    _slot_state(S, pos)
    assert kc.numel() >= S * H * T * hd and vc.numel() >= S * H * T * hd
    check(lib.svae_slot_attn(qkv.data_ptr(), ldq or 3 * H * hd, kc.data_ptr(), vc.data_ptr(), S, H, hd, T,
                             pos.data_ptr(), window, hd ** -0.5 if scale is None else scale, O.data_ptr(),
                             ldo or H * hd, stream()), 'svae_slot_attn')


def slot_embed(ids, T, pos, table, x, S, D):
    _dev(ids, table, x)
    _slot_state(S, pos)
    assert ids.dtype == torch.int64 and ids.numel() >= S * T
    check(lib.svae_slot_embed(ids.data_ptr(), T, pos.data_ptr(), table.data_ptr(), x.data_ptr(), S, D, stream()),
          'svae_slot_embed')


def slot_splice(x, zp, pos, S, D, ldz=None):
    """x[s] = zp[s][:D] for the slots at position 1; zp may be a column block of a wider [S, ldz] buffer."""
    _dev(x, zp)
    _slot_state(S, pos)
    ldz = ldz or D
    assert x.dtype == f32 and zp.dtype == f32 and x.numel() >= S * D
    assert zp.shape == (S, zp.shape[1]) and zp.shape[1] >= D and zp.stride() == (ldz, 1)
    check(lib.svae_slot_splice(x.data_ptr(), zp.data_ptr(), ldz, pos.data_ptr(), S, D, stream()), 'svae_slot_splice')


def slot_penalty(logits, S, ids, T, pos, penalty):
    _dev(logits, ids)
    _slot_state(S, pos)
    assert ids.dtype == torch.int64 and ids.numel() >= S * T
    check(lib.svae_slot_penalty(logits.data_ptr(), logits.stride(0), S, ids.data_ptr(), T, pos.data_ptr(), penalty,
                                stream()), 'svae_slot_penalty')


def slot_sample(logits, V, S, ids, T, pos, key, out, num_samples, end_token, temperature, top_k, top_p, seed):
    """out: int16 [num_samples, T - 1], zeroed by the caller; the token of slot s lands in out[key[s]][pos[s] - 1]."""
    _dev(logits, ids, out)
    _slot_state(S, pos, key)
    assert ids.dtype == torch.int64 and ids.numel() >= S * T
    assert out.dtype == torch.int16 and out.is_contiguous() and out.numel() >= num_samples * (T - 1)
    check(lib.svae_slot_sample(logits.data_ptr(), logits.stride(0), V, S, ids.data_ptr(), T, pos.data_ptr(),
                               key.data_ptr(), out.data_ptr(), num_samples, end_token, temperature, top_k, top_p,
                               seed & 0xFFFFFFFFFFFFFFFF, stream()), 'svae_slot_sample')


def slot_refill(pos, key, ids, T, S, start_token, z_all, z_slot, num_samples, next_sample, completed):
    """svae_slot_refill: finished slots take the next sample numbers in slot order (or go idle)."""
    _dev(ids, z_all, z_slot)
    _slot_state(S, pos, key)
    _slot_state(1, next_sample, completed)
    Z = z_slot.shape[-1]
    assert ids.dtype == torch.int64 and ids.numel() >= S * T
    assert z_all.dtype == f32 and z_slot.dtype == f32 and z_all.is_contiguous() and z_slot.is_contiguous()
    assert z_all.numel() >= num_samples * Z and z_slot.numel() >= S * Z
    check(lib.svae_slot_refill(pos.data_ptr(), key.data_ptr(), ids.data_ptr(), T, S, start_token, z_all.data_ptr(),
                               z_slot.data_ptr(), Z, num_samples, next_sample.data_ptr(), completed.data_ptr(),
                               stream()), 'svae_slot_refill')


# ---- beam search decoding (R = B * W rows; the state buffers of decoding.BeamState)
def beam_attn(qkv, kc, vc, anc, O, R, W, H, hd, T, cur, window, scale=None, ldq=None, ldo=None):
    """svae_beam_attn: dec_attn reading key j < p of row r from cache row (r // W) * W + anc[r][j]."""
    _dev(qkv, kc, vc, anc, O, cur)
    assert anc.dtype == torch.uint8 and anc.is_contiguous() and anc.numel() >= R * T
    assert kc.numel() >= R * H * T * hd and vc.numel() >= R * H * T * hd
    check(lib.svae_beam_attn(qkv.data_ptr(), ldq or 3 * H * hd, kc.data_ptr(), vc.data_ptr(), anc.data_ptr(), R, W, H,
                             hd, T, cur.data_ptr(), window, hd ** -0.5 if scale is None else scale, O.data_ptr(),
                             ldo or H * hd, stream()), 'svae_beam_attn')


def beam_topk(logits, V, R, W, cum, done, cand_score, cand_tok):
    """svae_beam_topk: cand_score f32 / cand_tok int32 [R, 2W] of the rows with cum > -inf whose document is live."""
    _dev(logits, cum, cand_score, cand_tok)
    assert logits.dtype == f32 and logits.stride(1) == 1 and logits.shape[0] >= R and logits.shape[1] >= V
    assert cum.dtype == f32 and cum.numel() >= R and (done is None or (done.dtype == torch.uint8 and done.numel() * W >= R))
    assert cand_score.dtype == f32 and cand_tok.dtype == torch.int32
    assert cand_score.is_contiguous() and cand_tok.is_contiguous() and min(cand_score.numel(), cand_tok.numel()) >= R * 2 * W
    check(lib.svae_beam_topk(logits.data_ptr(), logits.stride(0), V, R, W, cum.data_ptr(), ptr(done),
                             cand_score.data_ptr(), cand_tok.data_ptr(), stream()), 'svae_beam_topk')


def _beam_state(st):
    B, W, T = st.B, st.W, st.T
    R = B * W
    for t, dt, n in ((st.cum, f32, R), (st.ids, torch.int64, R * T), (st.anc, torch.uint8, R * T),
                     (st.ids_next, torch.int64, R * T), (st.anc_next, torch.uint8, R * T), (st.len_pen, f32, T),
                     (st.pool_score, f32, R), (st.pool_logp, f32, R), (st.pool_len, torch.int32, R),
                     (st.pool_ids, torch.int64, R * T), (st.pool_n, torch.int32, B), (st.done, torch.uint8, B),
                     (st.not_done, torch.int32, 1), (st.stamp, torch.int32, B), (st.cur, torch.int32, 1)):
        assert t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= n
    for t, dt in ((st.hist_parent, torch.int32), (st.hist_token, torch.int32), (st.hist_score, f32)):
        assert t is None or (t.is_cuda and t.dtype == dt and t.is_contiguous() and t.numel() >= T * R)


def beam_select(cand_score, cand_tok, st):
    """svae_beam_select on a decoding.BeamState: one step's selection, pool update and commit."""
    _beam_state(st)
    R = st.B * st.W
    assert cand_score.dtype == f32 and cand_tok.dtype == torch.int32
    assert cand_score.is_contiguous() and cand_tok.is_contiguous()
    assert min(cand_score.numel(), cand_tok.numel()) >= R * 2 * st.W
    check(lib.svae_beam_select(cand_score.data_ptr(), cand_tok.data_ptr(), st.cum.data_ptr(), st.ids.data_ptr(),
                               st.anc.data_ptr(), st.ids_next.data_ptr(), st.anc_next.data_ptr(), st.B, st.W, st.T,
                               st.cur.data_ptr(), st.end_token, st.len_pen.data_ptr(), 1 if st.alpha > 0 else 0,
                               st.pool_score.data_ptr(), st.pool_logp.data_ptr(), st.pool_len.data_ptr(),
                               st.pool_ids.data_ptr(), st.pool_n.data_ptr(), st.done.data_ptr(),
                               st.not_done.data_ptr(), st.stamp.data_ptr(), ptr(st.hist_parent), ptr(st.hist_token),
                               ptr(st.hist_score), stream()), 'svae_beam_select')


def beam_finalize(st, n):
    """svae_beam_finalize -> (ids int64 [B, n, T - 1], scores f32 [B, n], log_probs f32 [B, n], lengths int32 [B, n])."""
    _beam_state(st)
    B, T, dev = st.B, st.T, st.cum.device
    ids = torch.empty(B, n, T - 1, device=dev, dtype=torch.int64)
    scores, logp = torch.empty(B, n, device=dev, dtype=f32), torch.empty(B, n, device=dev, dtype=f32)
    lengths = torch.empty(B, n, device=dev, dtype=torch.int32)
    check(lib.svae_beam_finalize(st.cum.data_ptr(), st.ids.data_ptr(), B, st.W, T, st.len_pen.data_ptr(),
                                 st.pool_score.data_ptr(), st.pool_logp.data_ptr(), st.pool_len.data_ptr(),
                                 st.pool_ids.data_ptr(), st.pool_n.data_ptr(), st.done.data_ptr(), n, ids.data_ptr(),
                                 scores.data_ptr(), logp.data_ptr(), lengths.data_ptr(), stream()), 'svae_beam_finalize')
    return ids, scores, logp, lengths


def _latent_rows(*ts):
    """The [rows, Z] f32 operands of the latent kernels: contiguous device tensors of one shape."""
    _dev(*ts)
    for t in ts:
        assert t.dtype == f32 and t.dim() == 2 and t.is_contiguous() and t.shape == ts[0].shape
    return ts[0].shape


def latent_prepare(mu, scale, inv_var=None, logdet=None, inv_norm=None):
    """svae_latent_prepare: from mu, scale f32 [N, Z] the per-row quantities the searches need, computed once:
    inv_var [N, Z] = 1 / scale^2, logdet [N] = sum log scale, inv_norm [N] = 1 / max(|mu|, 1e-8). Outputs are
    allocated when not given; returns (inv_var, logdet, inv_norm)."""
    n, Z = _latent_rows(mu, scale)
    inv_var = torch.empty_like(mu) if inv_var is None else inv_var
    logdet = torch.empty(n, dtype=f32, device=mu.device) if logdet is None else logdet
    inv_norm = torch.empty(n, dtype=f32, device=mu.device) if inv_norm is None else inv_norm
    _latent_rows(mu, inv_var)
    for t in (logdet, inv_norm):
        _dev(t)
        assert t.dtype == f32 and t.is_contiguous() and t.numel() == n
    if n:
        check(lib.svae_latent_prepare(mu.data_ptr(), scale.data_ptr(), inv_var.data_ptr(), logdet.data_ptr(),
                                      inv_norm.data_ptr(), n, Z, stream()), 'svae_latent_prepare')
    return inv_var, logdet, inv_norm


def _latent_operands(metric, query, corpus):
    """query = (mu, scale, logdet, inv_norm) [Q, Z] / [Q]; corpus = (mu, inv_var, logdet, inv_norm) [N, Z] / [N]
    (the outputs of latent_prepare next to their mu); a metric's unused operands may be None."""
    if isinstance(metric, str):
        metric = N.LATENT_METRICS[metric]
    q_mu, q_scale, q_ld, q_in = query
    c_mu, c_iv, c_ld, c_in = corpus
    need = {N.LATENT_L2: (), N.LATENT_COSINE: (q_in, c_in), N.LATENT_KL: (q_scale, q_ld, c_iv, c_ld)}[metric]
    assert all(t is not None for t in need), 'operand missing for this metric'
    Q, Z = _latent_rows(*[t for t in (q_mu, q_scale) if t is not None])
    n, Zc = _latent_rows(*[t for t in (c_mu, c_iv) if t is not None])
    assert Z == Zc and Q >= 1 and n >= 1
    for t, m in ((q_ld, Q), (q_in, Q), (c_ld, n), (c_in, n)):
        if t is not None:
            _dev(t)
            assert t.dtype == f32 and t.is_contiguous() and t.numel() == m
    args_q = (q_mu.data_ptr(), ptr(q_scale), ptr(q_ld), ptr(q_in), Q)
    args_c = (c_mu.data_ptr(), ptr(c_iv), ptr(c_ld), ptr(c_in), n, Z)
    return metric, args_q, args_c, Q, n


def latent_scores(metric, query, corpus, out=None):
    """svae_latent_scores: the dense f32 [Q, N] score matrix of `metric` ('l2' | 'cosine' | 'kl' or the enum)."""
    metric, args_q, args_c, Q, n = _latent_operands(metric, query, corpus)
    if out is None:
        out = torch.empty(Q, n, dtype=f32, device=query[0].device)
    _dev(out)
    assert out.dtype == f32 and out.is_contiguous() and out.shape == (Q, n)
    check(lib.svae_latent_scores(metric, *args_q, *args_c, out.data_ptr(), stream()), 'svae_latent_scores')
    return out


def latent_topk(metric, query, corpus, k):
    """svae_latent_topk: the best k corpus rows per query, best first: (scores f32 [Q, k], indices int32 [Q, k]).
    The candidate workspace is allocated per call (stream-ordered by the caching allocator: nothing shared between
    calls or streams)."""
    metric, args_q, args_c, Q, n = _latent_operands(metric, query, corpus)
    if not 1 <= k <= min(64, n):
        raise ValueError(f'latent_topk: k = {k} outside 1..min(64, {n} rows)')
    dev = query[0].device
    nbytes = lib.svae_latent_topk_ws_bytes(Q, k)
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    scores = torch.empty(Q, k, dtype=f32, device=dev)
    indices = torch.empty(Q, k, dtype=torch.int32, device=dev)
    check(lib.svae_latent_topk(metric, *args_q, *args_c, k, ws.data_ptr(), nbytes, scores.data_ptr(),
                               indices.data_ptr(), stream()), 'svae_latent_topk')
    return scores, indices


def _tsne_f32(t, *shape):
    _dev(t)
    assert t.dtype == f32 and t.is_contiguous() and tuple(t.shape) == shape, (tuple(t.shape), shape)
    return t


def _tsne_graph_shape(n, k):
    if n * k >= 2 ** 31:
        raise ValueError(f'tsne: N * k = {n * k} does not fit the int32 edge ids')
    if not 1 <= k <= 64:
        raise ValueError(f'tsne: k = {k} outside 1..64')


def tsne_affinities(dist, perplexity):
    """svae_tsne_affinities: dist f32 [N, k] (a row's neighbour dissimilarities) -> (p f32 [N, k], beta f32 [N]): per
    row the Gaussian conditional whose entropy is log(perplexity), and the precision found for it."""
    _dev(dist)
    assert dist.dtype == f32 and dist.dim() == 2 and dist.is_contiguous()
    n, k = dist.shape
    _tsne_graph_shape(n, k)
    if not 1.0 < perplexity < k:
        raise ValueError(f'tsne_affinities: perplexity {perplexity} outside (1, k = {k})')
    p = torch.empty_like(dist)
    beta = torch.empty(n, dtype=f32, device=dist.device)
    if n:
        check(lib.svae_tsne_affinities(dist.data_ptr(), n, k, float(perplexity), p.data_ptr(), beta.data_ptr(),
                                       stream()), 'svae_tsne_affinities')
    return p, beta


def tsne_repulse_geometry(n):
    """(rows per workgroup, column slices, columns per slice) of svae_tsne_repulse at n rows."""
    cols = lib.svae_tsne_repulse_slice_cols(n)
    return N.TSNE_ROWS_PER_BLOCK, -(-n // cols), cols


def tsne_repulse(y, rep=None, zrow=None, zsum=None):
    """svae_tsne_repulse: y f32 [N, 2] -> (rep f32 [N, 2], zrow f32 [N], zsum f32 [1]), the exact all-pairs Student-t
    repulsion and its normaliser. The slice workspace is allocated per call (stream-ordered by the caching
    allocator)."""
    n = y.shape[0]
    _tsne_f32(y, n, 2)
    if n < 2:
        raise ValueError('tsne_repulse: at least two points')
    dev = y.device
    rep = torch.empty_like(y) if rep is None else _tsne_f32(rep, n, 2)
    zrow = torch.empty(n, dtype=f32, device=dev) if zrow is None else _tsne_f32(zrow, n)
    zsum = torch.empty(1, dtype=f32, device=dev) if zsum is None else _tsne_f32(zsum, 1)
    nbytes = lib.svae_tsne_repulse_ws_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    check(lib.svae_tsne_repulse(y.data_ptr(), n, ws.data_ptr(), nbytes, rep.data_ptr(), zrow.data_ptr(),
                                zsum.data_ptr(), stream()), 'svae_tsne_repulse')
    return rep, zrow, zsum


def tsne_attract(y, nbr, p, rev_ptr, rev_edge, attr=None):
    """svae_tsne_attract: the attraction over the k-NN edges in both directions. nbr int32 [N, k], p f32 [N, k] (the
    conditional affinities), rev_ptr int32 [N + 1] / rev_edge int32 [N * k] from sparse_vae.tsne.reverse_edges ->
    attr f32 [N, 2] (without the 1 / 2N of the symmetrisation: tsne_update applies it)."""
    n = y.shape[0]
    _tsne_f32(y, n, 2)
    _dev(nbr, rev_ptr, rev_edge)
    assert nbr.dim() == 2 and nbr.shape[0] == n
    k = nbr.shape[1]
    if n < 2:
        raise ValueError('tsne_attract: at least two points')
    _tsne_graph_shape(n, k)
    _tsne_f32(p, n, k)
    for t, m in ((nbr, n * k), (rev_ptr, n + 1), (rev_edge, n * k)):
        assert t.dtype == torch.int32 and t.is_contiguous() and t.numel() == m
    attr = torch.empty_like(y) if attr is None else _tsne_f32(attr, n, 2)
    check(lib.svae_tsne_attract(y.data_ptr(), nbr.data_ptr(), p.data_ptr(), rev_ptr.data_ptr(), rev_edge.data_ptr(),
                                n, k, attr.data_ptr(), stream()), 'svae_tsne_attract')
    return attr


def tsne_update(y, vel, gains, attr, rep, zsum, exaggeration, learning_rate, momentum):
    """svae_tsne_update, in place on y, vel, gains (f32 [N, 2]): one step of van der Maaten's optimiser from the
    attraction, the repulsion and its normaliser zsum (f32 [1], read on the device)."""
    n = y.shape[0]
    if n < 2:
        raise ValueError('tsne_update: at least two points')
    for t in (y, vel, gains, attr, rep):
        _tsne_f32(t, n, 2)
    _tsne_f32(zsum, 1)
    check(lib.svae_tsne_update(y.data_ptr(), vel.data_ptr(), gains.data_ptr(), attr.data_ptr(), rep.data_ptr(),
                               zsum.data_ptr(), n, float(exaggeration), float(learning_rate), float(momentum),
                               stream()), 'svae_tsne_update')


def _mmd_rows(t, name):
    """An [rows, Z] f32 operand of the MMD kernels: contiguous, on the device, Z a multiple of 4 in 4..256."""
    _dev(t)
    assert t.dtype == f32 and t.dim() == 2 and t.is_contiguous(), name
    n, Z = t.shape
    if Z % 4 or not 4 <= Z <= 256:
        raise ValueError(f'{name}: the row length must be a multiple of 4 in 4..256, got {Z}')
    if not 1 <= n <= 2 ** 24:
        raise ValueError(f'{name}: 1..2^24 rows, got {n}')
    return n, Z


def pairsum_geometry(n, m, Z, triangular):
    """(rows per workgroup, row blocks, column slices, columns per slice, tile columns) of svae_pairsum."""
    geom = (ctypes.c_int32 * 5)()
    check(lib.svae_pairsum_geometry(n, m, Z, int(bool(triangular)), ctypes.addressof(geom)), 'svae_pairsum_geometry')
    return tuple(geom)


def pairsum(x, y=None, *, kind, params, col_off=None, out=None):
    """svae_pairsum: out f64 [P] = sum over pairs of k_p(|x_i - y_j|^2 + col_off_j). y None: the pairs i < j of x
    (pdist's); else all pairs of x [N, Z] with y [M, Z]. kind 'rbf': k_p = exp(-params[p] d2); 'imq': k_p =
    params[p] / (params[p] + d2). params: up to 8 Python floats (rounded to f32). col_off: f32 [M], rectangular only.
    The per-workgroup workspace is allocated per call (stream-ordered by the caching allocator)."""
    n, Z = _mmd_rows(x, 'pairsum x')
    tri = y is None
    if tri:
        m = n
        if n < 2:
            raise ValueError('pairsum: the triangular set needs at least two rows')
        if col_off is not None:
            raise ValueError('pairsum: a column offset only goes with a second set of rows')
    else:
        m, Zy = _mmd_rows(y, 'pairsum y')
        assert Zy == Z, 'x and y differ in row length'
    params = [float(p) for p in params]
    P = len(params)
    if not 1 <= P <= N.PAIRSUM_MAX_P:
        raise ValueError(f'pairsum: 1..{N.PAIRSUM_MAX_P} kernel parameters, got {P}')
    if col_off is not None:
        _dev(col_off)
        assert col_off.dtype == f32 and col_off.is_contiguous() and col_off.numel() == m
    dev = x.device
    out = torch.empty(P, dtype=torch.float64, device=dev) if out is None else out
    _dev(out)
    assert out.dtype == torch.float64 and out.is_contiguous() and out.numel() == P
    nbytes = lib.svae_pairsum_ws_bytes(n, m, Z, int(tri))
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    prm = (ctypes.c_float * P)(*params)
    check(lib.svae_pairsum(x.data_ptr(), n, None if tri else y.data_ptr(), m, Z, int(tri), N.PAIR_KINDS[kind],
                           ctypes.addressof(prm), P, ptr(col_off), ws.data_ptr(), nbytes, out.data_ptr(), stream()),
          'svae_pairsum')
    return out


def mmd_rowterm(x, w, m=None, out=None):
    """svae_mmd_rowterm: out f64 [1] = sum_i exp(-0.5 sum_j (x_ij - m_j)^2 w_j); w f32 [Z], m f32 [Z] or None (0)."""
    n, Z = _mmd_rows(x, 'mmd_rowterm x')
    for t in (w,) if m is None else (w, m):
        _dev(t)
        assert t.dtype == f32 and t.is_contiguous() and t.numel() == Z
    out = torch.empty(1, dtype=torch.float64, device=x.device) if out is None else out
    _dev(out)
    assert out.dtype == torch.float64 and out.numel() == 1
    nbytes = lib.svae_mmd_rowterm_ws_bytes(n)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=x.device)
    check(lib.svae_mmd_rowterm(x.data_ptr(), ptr(m), w.data_ptr(), n, Z, ws.data_ptr(), nbytes, out.data_ptr(),
                               stream()), 'svae_mmd_rowterm')
    return out


def latent_colstats(loc, scale):
    """svae_latent_colstats: (mean_loc, var_loc, mean_kl), f64 [Z] each, over the rows of loc, scale f32 [N, Z]:
    the mean and unbiased variance of loc and the mean KL to N(0, 1) per latent dimension."""
    n, Z = _mmd_rows(loc, 'latent_colstats loc')
    _latent_rows(loc, scale)
    out = torch.empty(3, Z, dtype=torch.float64, device=loc.device)
    nbytes = lib.svae_latent_colstats_ws_bytes(n, Z)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=loc.device)
    check(lib.svae_latent_colstats(loc.data_ptr(), scale.data_ptr(), n, Z, ws.data_ptr(), nbytes, out[0].data_ptr(),
                                   out[1].data_ptr(), out[2].data_ptr(), stream()), 'svae_latent_colstats')
    return out[0], out[1], out[2]


def latent_draw(loc, scale, seed=0, eps=None, out=None):
    """svae_latent_draw: z = loc + scale * eps, f32 [N, Z]; eps f32 [N, Z] or None (the counter RNG keyed by seed,
    row and column)."""
    n, Z = _mmd_rows(loc, 'latent_draw loc')
    ts = (loc, scale) if eps is None else (loc, scale, eps)
    _latent_rows(*ts)
    out = torch.empty_like(loc) if out is None else out
    _latent_rows(loc, out)
    check(lib.svae_latent_draw(loc.data_ptr(), scale.data_ptr(), ptr(eps), int(seed) & (2 ** 64 - 1), n, Z,
                               out.data_ptr(), stream()), 'svae_latent_draw')
    return out


def _kmeans_shape(x, K, name):
    n, Z = _mmd_rows(x, f'{name} x')
    if not 1 <= K <= min(N.KMEANS_MAX_K, n):
        raise ValueError(f'{name}: 1 <= K <= min({N.KMEANS_MAX_K}, {n} rows), got {K}')
    return n, Z


def _kmeans_vec(t, dtype, numel, name):
    _dev(t)
    assert t.dtype == dtype and t.is_contiguous() and t.numel() == numel, name
    return t


def _kmeans_ws(nbytes, dev):
    return torch.empty(nbytes // 8, dtype=torch.int64, device=dev)


def kmeans_geometry(n, K, Z):
    """svae_kmeans_geometry: (assign rows per workgroup, assign row blocks, centroid tile, sort blocks, rows per sort
    block, row groups of the segment sums, seed block rows, seed blocks)."""
    geom = (ctypes.c_int32 * 8)()
    check(lib.svae_kmeans_geometry(n, K, Z, ctypes.addressof(geom)), 'svae_kmeans_geometry')
    return tuple(geom)


def kmeans_assign(x, cent, label=None, d2=None, changed=None, inertia=None, want_d2=True):
    """svae_kmeans_assign: x f32 [N, Z] against cent f32 [K, Z] -> (label int32 [N], d2 f32 [N] or None, changed int32
    [1], inertia f64 [1]). label is in/out: the previous labels (default: all -1, none). Ties go to the lower centroid
    index; a NaN distance loses to every number. The workspace is allocated per call (stream-ordered by the caching
    allocator)."""
    K = cent.shape[0]
    n, Z = _kmeans_shape(x, K, 'kmeans_assign')
    dev = x.device
    _dev(cent)
    assert cent.dtype == f32 and cent.is_contiguous() and tuple(cent.shape) == (K, Z)
    label = torch.full((n,), -1, dtype=torch.int32, device=dev) if label is None else label
    _kmeans_vec(label, torch.int32, n, 'label')
    if d2 is None and want_d2:
        d2 = torch.empty(n, dtype=f32, device=dev)
    if d2 is not None:
        _kmeans_vec(d2, f32, n, 'd2')
    changed = torch.empty(1, dtype=torch.int32, device=dev) if changed is None else changed
    inertia = torch.empty(1, dtype=torch.float64, device=dev) if inertia is None else inertia
    _kmeans_vec(changed, torch.int32, 1, 'changed')
    _kmeans_vec(inertia, torch.float64, 1, 'inertia')
    nbytes = lib.svae_kmeans_assign_ws_bytes(n, K, Z)
    ws = _kmeans_ws(nbytes, dev)
    check(lib.svae_kmeans_assign(x.data_ptr(), n, cent.data_ptr(), K, Z, label.data_ptr(), ptr(d2), changed.data_ptr(),
                                 inertia.data_ptr(), ws.data_ptr(), nbytes, stream()), 'svae_kmeans_assign')
    return label, d2, changed, inertia


def kmeans_update(x, label, cent, count=None):
    """svae_kmeans_update, in place on cent f32 [K, Z]: cent[c] = the f64 mean of the rows of x labelled c, rounded to
    f32 (a fixed summation tree, no atomics); an empty cluster keeps its centroid; labels outside 0..K-1 are ignored.
    Returns (cent, count int32 [K])."""
    K = cent.shape[0]
    n, Z = _kmeans_shape(x, K, 'kmeans_update')
    dev = x.device
    _dev(cent)
    assert cent.dtype == f32 and cent.is_contiguous() and tuple(cent.shape) == (K, Z)
    _kmeans_vec(label, torch.int32, n, 'label')
    count = torch.empty(K, dtype=torch.int32, device=dev) if count is None else count
    _kmeans_vec(count, torch.int32, K, 'count')
    nbytes = lib.svae_kmeans_update_ws_bytes(n, K, Z)
    ws = _kmeans_ws(nbytes, dev)
    check(lib.svae_kmeans_update(x.data_ptr(), n, label.data_ptr(), K, Z, cent.data_ptr(), count.data_ptr(),
                                 ws.data_ptr(), nbytes, stream()), 'svae_kmeans_update')
    return cent, count


def kmeans_seed(x, K, seed=0, u=None, rows=None, cent=None):
    """svae_kmeans_seed: k-means++ (D^2 sampling) of K rows of x f32 [N, Z] -> (rows int32 [K], cent f32 [K, Z]). u:
    f32 [K] uniforms in [0, 1), or None (the counter RNG keyed by (seed, step)). Nothing is read back: the K steps
    queue on the stream."""
    K = int(K)
    n, Z = _kmeans_shape(x, K, 'kmeans_seed')
    dev = x.device
    if u is not None:
        _kmeans_vec(u, f32, K, 'u')
    rows = torch.empty(K, dtype=torch.int32, device=dev) if rows is None else rows
    cent = torch.empty(K, Z, dtype=f32, device=dev) if cent is None else cent
    _kmeans_vec(rows, torch.int32, K, 'rows')
    _kmeans_vec(cent, f32, K * Z, 'cent')
    nbytes = lib.svae_kmeans_seed_ws_bytes(n, K, Z)
    ws = _kmeans_ws(nbytes, dev)
    check(lib.svae_kmeans_seed(x.data_ptr(), n, K, Z, ptr(u), int(seed) & (2 ** 64 - 1), rows.data_ptr(),
                               cent.data_ptr(), ws.data_ptr(), nbytes, stream()), 'svae_kmeans_seed')
    return rows, cent


def _text_pairs(cand, ref, cand_len, ref_len, name):
    _dev(cand, ref, cand_len, ref_len)
    for t, what in ((cand, 'candidates'), (ref, 'references')):
        if t.dim() != 2 or t.dtype != torch.int16 or not t.is_contiguous():
            raise ValueError(f'{name}: {what} must be contiguous int16 [P, W], got {t.dtype} {tuple(t.shape)}')
        if not 1 <= t.shape[1] <= N.TEXT_MAX_LEN:
            raise ValueError(f'{name}: {what} are {t.shape[1]} wide; the kernels take 1..{N.TEXT_MAX_LEN} '
                             f'(SVAE_TEXT_MAX_LEN)')
    P = cand.shape[0]
    if P < 1 or ref.shape[0] != P:
        raise ValueError(f'{name}: {P} candidates against {ref.shape[0]} references')
    for t in (cand_len, ref_len):
        if t.dtype != torch.int32 or not t.is_contiguous() or tuple(t.shape) != (P,):
            raise ValueError(f'{name}: lengths must be contiguous int32 [{P}], got {t.dtype} {tuple(t.shape)}')
    return P


def ngram_overlap(cand, ref, cand_len, ref_len, out=None):
    """svae_ngram_overlap: cand int16 [P, wc], ref int16 [P, wr], lengths int32 [P] (clamped into [0, width] by the
    kernel) -> int32 [P, 5] = (m1, m2, m3, m4, exact): the clipped n-gram match counts of orders 1..4 and the number of
    equal positions. Ids must be 0..32767 (not checked here: that would synchronise)."""
    P = _text_pairs(cand, ref, cand_len, ref_len, 'ngram_overlap')
    out = torch.empty(P, 5, dtype=torch.int32, device=cand.device) if out is None else out
    _dev(out)
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (P, 5)
    check(lib.svae_ngram_overlap(cand.data_ptr(), cand.shape[1], ref.data_ptr(), ref.shape[1], cand_len.data_ptr(),
                                 ref_len.data_ptr(), P, out.data_ptr(), stream()), 'svae_ngram_overlap')
    return out


def edit_distance(cand, ref, cand_len, ref_len, out=None):
    """svae_edit_distance: the token Levenshtein distance (unit costs) of every pair -> int32 [P]. Operands as
    ngram_overlap."""
    P = _text_pairs(cand, ref, cand_len, ref_len, 'edit_distance')
    out = torch.empty(P, dtype=torch.int32, device=cand.device) if out is None else out
    _dev(out)
    assert out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (P,)
    check(lib.svae_edit_distance(cand.data_ptr(), cand.shape[1], ref.data_ptr(), ref.shape[1], cand_len.data_ptr(),
                                 ref_len.data_ptr(), P, out.data_ptr(), stream()), 'svae_edit_distance')
    return out


def gmm_param_offsets(K, Z):
    """The float offsets of a svae_gmm parameter block (include/svae.h's SVAE_GMM_OFF_*): dict name -> (offset, shape),
    plus 'floats', the block's length."""
    kp, kz = (K + 3) // 4 * 4, K * Z
    out = {'weight': (0, (K,)), 'logc': (kp, (K,))}
    for j, name in enumerate(('mean', 'var', 'inv_var', 'sd')):
        out[name] = (2 * kp + j * kz, (K, Z))
    out['floats'] = 2 * kp + 4 * kz
    assert out['floats'] == lib.svae_gmm_params_floats(K, Z)
    return out


def gmm_view(params, K, Z, name):
    """The view of row `name` ('weight', 'logc', 'mean', 'var', 'inv_var', 'sd') inside a parameter block."""
    off, shape = gmm_param_offsets(K, Z)[name]
    n = 1
    for d in shape:
        n *= d
    return params[off:off + n].view(shape)


def _gmm_shape(x, s2, params, K, name):
    n, Z = _mmd_rows(x, f'{name} x')
    if s2 is not None:
        _latent_rows(x, s2)
    if not 1 <= K <= N.GMM_MAX_K:
        raise ValueError(f'{name}: 1 <= K <= {N.GMM_MAX_K}, got {K}')
    _kmeans_vec(params, f32, lib.svae_gmm_params_floats(K, Z), 'params')
    return n, Z


def gmm_geometry(n, K, Z, has_s2=False):
    """svae_gmm_geometry: (E-step rows per workgroup, row blocks, component tile, M-step row groups, rows per group,
    E-step row segments)."""
    geom = (ctypes.c_int32 * 6)()
    check(lib.svae_gmm_geometry(n, K, Z, int(bool(has_s2)), ctypes.addressof(geom)), 'svae_gmm_geometry')
    return tuple(geom)


def gmm_pack(weight, mean, var):
    """A parameter block from weight [K], mean [K, Z], var [K, Z] device tensors, derived rows included
    (svae_gmm_prepare)."""
    _dev(weight, mean, var)
    K, Z = mean.shape
    if Z % 4 or not 4 <= Z <= 256 or not 1 <= K <= N.GMM_MAX_K:
        raise ValueError(f'gmm_pack: Z a multiple of 4 in 4..256 and 1 <= K <= {N.GMM_MAX_K}, got K = {K}, Z = {Z}')
    assert weight.shape == (K,) and var.shape == (K, Z)
    params = torch.zeros(gmm_param_offsets(K, Z)['floats'], dtype=f32, device=mean.device)
    gmm_view(params, K, Z, 'weight').copy_(weight)
    gmm_view(params, K, Z, 'mean').copy_(mean)
    gmm_view(params, K, Z, 'var').copy_(var)
    return gmm_prepare(params, K, Z)


def gmm_prepare(params, K, Z):
    """svae_gmm_prepare, in place: the derived rows (inv_var, sd, logc) of a block from its (weight, mean, var)."""
    _kmeans_vec(params, f32, lib.svae_gmm_params_floats(K, Z), 'params')
    check(lib.svae_gmm_prepare(params.data_ptr(), K, Z, stream()), 'svae_gmm_prepare')
    return params


def gmm_estep(x, s2, params, K, lse=None, label=None, resp=None, bound=None, want_label=True, want_resp=False):
    """svae_gmm_estep: rows x (and their variances s2, or None for points) f32 [N, Z] against a K-component block ->
    (lse f32 [N], label int32 [N] or None, resp f32 [N, K] or None, bound f64 [1] = sum lse). The workspace is
    allocated per call (stream-ordered by the caching allocator)."""
    n, Z = _gmm_shape(x, s2, params, K, 'gmm_estep')
    dev = x.device
    lse = torch.empty(n, dtype=f32, device=dev) if lse is None else lse
    _kmeans_vec(lse, f32, n, 'lse')
    if label is None and want_label:
        label = torch.empty(n, dtype=torch.int32, device=dev)
    if label is not None:
        _kmeans_vec(label, torch.int32, n, 'label')
    if resp is None and want_resp:
        resp = torch.empty(n, K, dtype=f32, device=dev)
    if resp is not None:
        _kmeans_vec(resp, f32, n * K, 'resp')
    bound = torch.empty(1, dtype=torch.float64, device=dev) if bound is None else bound
    _kmeans_vec(bound, torch.float64, 1, 'bound')
    nbytes = lib.svae_gmm_estep_ws_bytes(n, K, Z)
    ws = _kmeans_ws(nbytes, dev)
    check(lib.svae_gmm_estep(x.data_ptr(), ptr(s2), n, params.data_ptr(), K, Z, lse.data_ptr(), ptr(label), ptr(resp),
                             bound.data_ptr(), ws.data_ptr(), nbytes, stream()), 'svae_gmm_estep')
    return lse, label, resp, bound


def gmm_mstep(x, s2, params, K, lse=None, label=None, reg_covar=1e-6, nk=None):
    """svae_gmm_mstep, in place on params: one M-step from the soft responsibilities expf(a - lse) (lse f32 [N]) or
    from hard labels (int32 [N]); exactly one of the two. -> nk f64 [K]."""
    n, Z = _gmm_shape(x, s2, params, K, 'gmm_mstep')
    if (lse is None) == (label is None):
        raise ValueError('gmm_mstep: exactly one of lse (soft) and label (hard)')
    if lse is not None:
        _kmeans_vec(lse, f32, n, 'lse')
    else:
        _kmeans_vec(label, torch.int32, n, 'label')
    dev = x.device
    nk = torch.empty(K, dtype=torch.float64, device=dev) if nk is None else nk
    _kmeans_vec(nk, torch.float64, K, 'nk')
    nbytes = lib.svae_gmm_mstep_ws_bytes(n, K, Z)
    ws = _kmeans_ws(nbytes, dev)
    check(lib.svae_gmm_mstep(x.data_ptr(), ptr(s2), n, ptr(lse), ptr(label), params.data_ptr(), K, Z, float(reg_covar),
                             nk.data_ptr(), ws.data_ptr(), nbytes, stream()), 'svae_gmm_mstep')
    return nk


def gmm_sample(params, K, Z, n, seed=0, u=None, eps=None):
    """svae_gmm_sample: n draws -> (z f32 [n, Z], comp int32 [n]). u f32 [n] and eps f32 [n, Z] are injected, or drawn
    from the counter RNG keyed by seed (eps exactly as latent_draw draws it)."""
    _kmeans_vec(params, f32, lib.svae_gmm_params_floats(K, Z), 'params')
    if not 1 <= n <= 2 ** 24:
        raise ValueError(f'gmm_sample: 1..2^24 rows, got {n}')
    dev = params.device
    if u is not None:
        _kmeans_vec(u, f32, n, 'u')
    if eps is not None:
        _kmeans_vec(eps, f32, n * Z, 'eps')
    z = torch.empty(n, Z, dtype=f32, device=dev)
    comp = torch.empty(n, dtype=torch.int32, device=dev)
    check(lib.svae_gmm_sample(params.data_ptr(), K, Z, n, ptr(u), ptr(eps), int(seed) & (2 ** 64 - 1), z.data_ptr(),
                              comp.data_ptr(), stream()), 'svae_gmm_sample')
    return z, comp


def aggpost_geometry(m, n, Z, per_dim=False):
    """svae_aggpost_geometry: (points per workgroup, point blocks, row slices, rows per slice, tile rows, dimensions
    held per pass)."""
    geom = (ctypes.c_int32 * 6)()
    check(lib.svae_aggpost_geometry(m, n, Z, int(bool(per_dim)), ctypes.addressof(geom)), 'svae_aggpost_geometry')
    return tuple(geom)


def _aggpost_shape(z, loc, scale, name):
    m, Z = _mmd_rows(z, f'{name} z')
    n, Zr = _mmd_rows(loc, f'{name} loc')
    _latent_rows(loc, scale)
    if Zr != Z:
        raise ValueError(f'{name}: the points have {Z} dimensions and the rows {Zr}')
    return m, n, Z


def aggpost_logq(z, loc, scale, skip=None, per_dim=False, logq=None, logq_dim=None):
    """svae_aggpost_logq: the log-density of the aggregate posterior (1 / N) sum_j N(loc_j, scale_j^2) at the points
    z f32 [M, Z] against the rows loc, scale f32 [N, Z] -> logq f32 [M], or with per_dim (logq, logq_dim f32 [M, Z],
    the same per latent dimension). skip int32 [M] or None: the row each point leaves out (-1: none; needs N >= 2).
    The workspace is allocated per call (stream-ordered by the caching allocator)."""
    m, n, Z = _aggpost_shape(z, loc, scale, 'aggpost_logq')
    dev = z.device
    if skip is not None:
        _kmeans_vec(skip, torch.int32, m, 'skip')
        if n < 2:
            raise ValueError('aggpost_logq: leaving a row out needs at least two rows')
    logq = torch.empty(m, dtype=f32, device=dev) if logq is None else logq
    _kmeans_vec(logq, f32, m, 'logq')
    if logq_dim is None and per_dim:
        logq_dim = torch.empty(m, Z, dtype=f32, device=dev)
    if logq_dim is not None:
        _kmeans_vec(logq_dim, f32, m * Z, 'logq_dim')
    nbytes = lib.svae_aggpost_ws_bytes(m, n, Z, int(logq_dim is not None))
    ws = torch.empty(nbytes // 16, 2, dtype=torch.float64, device=dev)
    check(lib.svae_aggpost_logq(z.data_ptr(), m, loc.data_ptr(), scale.data_ptr(), n, Z, ptr(skip), logq.data_ptr(),
                                ptr(logq_dim), ws.data_ptr(), nbytes, stream()), 'svae_aggpost_logq')
    return (logq, logq_dim) if logq_dim is not None else logq


def aggpost_decompose(z, src, loc, scale, logq, logq_dim, out=None):
    """svae_aggpost_decompose: out f64 [4 + Z] = (mi, marginal_kl, tc, kl_mc, dim_kl[Z]) of the points z f32 [M, Z]
    drawn from the rows src int [M] of loc, scale f32 [N, Z], from their logq f32 [M] and logq_dim f32 [M, Z]. A CPU
    src outside 0..N-1 raises IndexError; a device src is not read back, its rows are clamped into that range."""
    m, n, Z = _aggpost_shape(z, loc, scale, 'aggpost_decompose')
    dev = z.device
    if not torch.is_tensor(src) or src.is_floating_point() or src.numel() != m:
        raise ValueError(f'aggpost_decompose: src must hold {m} integer rows')
    if src.is_cuda:
        src = src.reshape(-1).clamp(0, n - 1).to(torch.int32).contiguous()
    else:
        if not (0 <= int(src.min()) and int(src.max()) < n):
            raise IndexError(f'aggpost_decompose: src outside the rows (0..{n - 1})')
        src = src.reshape(-1).to(dev, torch.int32).contiguous()
    _kmeans_vec(logq, f32, m, 'logq')
    _kmeans_vec(logq_dim, f32, m * Z, 'logq_dim')
    out = torch.empty(4 + Z, dtype=torch.float64, device=dev) if out is None else out
    _kmeans_vec(out, torch.float64, 4 + Z, 'out')
    nbytes = lib.svae_aggpost_decompose_ws_bytes(m, Z)
    ws = torch.empty(nbytes // 8, dtype=torch.float64, device=dev)
    check(lib.svae_aggpost_decompose(z.data_ptr(), src.data_ptr(), loc.data_ptr(), scale.data_ptr(), logq.data_ptr(),
                                     logq_dim.data_ptr(), m, Z, ws.data_ptr(), nbytes, out.data_ptr(), stream()),
          'svae_aggpost_decompose')
    return out
