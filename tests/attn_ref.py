"""Plain torch restatements of the flash attention kernels of csrc/attention.hip (svae.h "Flash attention":
svae_attn_fwd, svae_attn_bwd), the cases the GPU test feeds them, the error measure and the bounds that test holds them
to, and a restatement of the library's kernel choice. Nothing in this file runs product code.

  attention()   the closed forms in float64 over [B, H, L, hd] views: O, lse, delta, dQ, dK, dV from P = exp(s - lse),
                dS = P o (dO V^T - delta), ...; test_attn_ref.py pins them with float64 autograd of
                softmax(s - 1e7 mask) v.
  emulate()     the same formulas in float64 with a bf16 rounding at exactly the places the kernels round: P before
                P V and P^T dO, dS before dS^T Q and dS K, and O, dK, dV and the bf16 dQ on output; delta from the O
                the call form provides. This is the rounding budget of the kernels' design; it runs no kernel.
  row_error()   per (batch, head, position) row of hd elements: max |got - ref| / rms(magnitude row), the magnitude
                being the same contraction with every factor replaced by its absolute value. One wrong row is one
                large term of the max. deviation(rows=True) does not serve here: causal query 0 and padded keys have
                an exactly zero reference, and the first few causal rows cancel (the emulation alone reaches 0.19 of
                the reference's own rms on dQ there).
  dispatch()    the set of kernel paths the library takes for a call: launch_fwd, fwd_split, bwd_layout and
                svae_attn_bwd restated for the default environment switches. test_attn_ref.py requires the union over
                CASES to be every path name; the GPU test cross-checks it against the library's workspace queries.

Layouts: token-major rows of d = H hd columns, heads interleaved (the nn.Linear output layout). The three call forms
are engine.py's: 'self' (one packed qkv matrix, row stride 3 d), 'cross' (q with stride d, packed kv with stride 2 d)
and 'learned' (one [Lq, d] query matrix shared by the batch, bq = 0, packed kv)."""
import collections
import functools
import math
import zlib

import torch

import oracle
from optim_ref import LOG2E, TOL_FACTOR, deviation  # noqa: F401  (one tolerance factor for every kernel test)

f64, f32, bf16 = torch.float64, torch.float32, torch.bfloat16


def heads(t, H):
    """[B, L, H hd] -> [B, H, L, hd]"""
    B, L, d = t.shape
    return t.view(B, L, H, d // H).transpose(1, 2)


def unheads(t):
    """[B, H, L, hd] -> [B, L, H hd]"""
    B, H, L, hd = t.shape
    return t.transpose(1, 2).reshape(B, L, H * hd)


def hidden(B, Lq, Lk, pad, causal, window):
    """[B, 1, Lq, Lk] bool, True where the key is NOT visible to the query: key_pad, above the diagonal, outside
    SparseAttention's window (oracle.sparse_mask)."""
    m = torch.zeros(B, 1, Lq, Lk, dtype=torch.bool)
    if pad is not None:
        m = m | pad.bool()[:, None, None, :]
    if window:
        m = m | oracle.sparse_mask(Lq, window)[None, None]
    elif causal:
        m = m | torch.ones(Lq, Lk, dtype=torch.bool).triu(1)[None, None]
    return m


def rotate(x, rot, inverse=False):
    """The rotary map of oracle.rotary with the table's factors: x [B, L, d], rot [>= L][d / 2] (cos, sin), pairs
    (2 i, 2 i + 1): (a, b) -> (a c - b s, b c + a s); inverse: its transpose (a c + b s, b c - a s), which is what the
    backward kernels apply to dQ (at the query row) and dK (at the key row)."""
    L = x.shape[1]
    c, s = rot[:L, :, 0].to(x.dtype), rot[:L, :, 1].to(x.dtype)
    if inverse:
        s = -s
    a, b = x[..., 0::2], x[..., 1::2]
    return torch.stack([a * c - b * s, b * c + a * s], dim=-1).flatten(-2)


def _rot_heads(t, rot):
    return heads(rotate(unheads(t), rot, inverse=True), t.shape[1])


def _softmax(q, k, hid, scale):
    """-> (P = exp(s - lse), zero where hidden and on rows with no visible key; lse, -inf on such rows)"""
    s = (q @ k.transpose(-1, -2)) * scale
    s = s.masked_fill(hid, -math.inf)
    lse = torch.logsumexp(s, -1)
    dead = torch.isinf(lse)
    P = (s - lse.masked_fill(dead, 0.0)[..., None]).exp()
    return P, lse


def attention(q, k, v, do, *, pad=None, causal=False, window=0, scale=None, rot=None, rot_q=True, dtype=f64):
    """q, do [B, H, Lq, hd]; k, v [B, H, Lk, hd]; pad [B, Lk] (non-zero = masked) or None. -> dict O, lse, delta, dQ,
    dK, dV (and P, dP), all [B, H, L, hd] / [B, H, Lq] in `dtype`. rot: dK, and with rot_q dQ, after the inverse
    rotation (the library rotates the bf16 dQ; the f32 dQ of the learned queries is left as it is)."""
    q, k, v, do = (t.to(dtype) for t in (q, k, v, do))
    B, H, Lq, hd = q.shape
    scale = hd ** -0.5 if scale is None else scale
    hid = hidden(B, Lq, k.shape[2], pad, causal, window)
    P, lse = _softmax(q, k, hid, scale)
    O = P @ v
    delta = (do * O).sum(-1)
    dP = do @ v.transpose(-1, -2)
    dS = P * (dP - delta[..., None])
    dQ, dK, dV = (dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale, P.transpose(-1, -2) @ do
    if rot is not None:
        dQ, dK = _rot_heads(dQ, rot) if rot_q else dQ, _rot_heads(dK, rot)
    return dict(O=O, lse=lse, delta=delta, dQ=dQ, dK=dK, dV=dV, P=P, dP=dP)


def _bf(t):
    return t.to(bf16).to(f64)


def o_forms(O_acc, o_extra):
    """The O the backward's delta is formed from, per call form: 'o_lo' bf16(O) + bf16(O - bf16(O)), 'o32' the f32 O,
    None bf16(O) alone. -> float64"""
    hi = _bf(O_acc)
    if o_extra == 'o_lo':
        return hi + _bf(O_acc - hi)
    if o_extra == 'o32':
        return O_acc.to(f32).to(f64)
    return hi


def emulate(q, k, v, do, *, pad=None, causal=False, window=0, scale=None, rot=None, o_extra=None, dq_bf=True,
            delta=None):
    """attention() in float64 with the kernels' bf16 roundings (the module docstring lists them). o_extra: the O the
    delta is formed from (o_forms); delta: given (the delta_ready form) instead. dq_bf: dQ is rotated and stored as
    bf16 (otherwise f32, unrotated).
    -> dict O, dQ, dK, dV, delta."""
    q, k, v, do = (t.to(f64) for t in (q, k, v, do))
    B, H, Lq, hd = q.shape
    scale = hd ** -0.5 if scale is None else scale
    hid = hidden(B, Lq, k.shape[2], pad, causal, window)
    P, _ = _softmax(q, k, hid, scale)
    Pb = _bf(P)
    O_acc = Pb @ v
    if delta is None:
        delta = (do * o_forms(O_acc, o_extra)).sum(-1)
    dS = _bf(P * (do @ v.transpose(-1, -2) - delta.to(f64)[..., None]))
    dQ, dK, dV = (dS @ k) * scale, (dS.transpose(-1, -2) @ q) * scale, Pb.transpose(-1, -2) @ do
    if rot is not None:
        dQ, dK = _rot_heads(dQ, rot) if dq_bf else dQ, _rot_heads(dK, rot)
    return dict(O=_bf(O_acc), dQ=_bf(dQ) if dq_bf else dQ, dK=_bf(dK), dV=_bf(dV), delta=delta)


def magnitudes(q, k, v, do, ref, scale=None):
    """The size each output row is held to: the output's contraction with every factor replaced by its absolute value
    (P, |dP| and |delta| from the reference `ref` of attention()). O: P |V|; dV: P^T |dO|; dQ: (P o (|dP| + |delta|))
    |K| scale; dK: (P o (|dP| + |delta|))^T |Q| scale. Unrotated: the rotation turns pairs inside a row and leaves
    the row's rms where it was to within the pair's imbalance."""
    q, k, v, do = (t.to(f64).abs() for t in (q, k, v, do))
    scale = q.shape[-1] ** -0.5 if scale is None else scale
    P = ref['P']
    A = P * (ref['dP'].abs() + ref['delta'].abs()[..., None])
    return dict(O=P @ v, dV=P.transpose(-1, -2) @ do, dQ=(A @ k) * scale, dK=(A.transpose(-1, -2) @ q) * scale)


def row_error(got, ref, mag):
    """max over elements of |got - ref| / rms(mag row), rows of hd elements ([..., hd] tensors). A row whose magnitude
    is zero (a padded key's dK / dV, every output of a batch entry with no visible key) has to be exactly zero in
    `got`: inf otherwise. A non-finite element of `got` gives inf."""
    got, ref, mag = got.to(f64), ref.to(f64), mag.to(f64)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    rms = mag.pow(2).mean(-1, keepdim=True).sqrt()
    zero = (rms == 0).expand_as(got)
    if bool((got[zero] != 0).any()):
        return math.inf
    live = ~zero
    if not bool(live.any()):
        return 0.0
    return ((got - ref).abs() / rms.clamp_min(1e-300))[live].max().item()


# ---------------------------------------------------------------------------------------------- f32 row constants
def lse_f32(q, k, hid, scale):
    """lse as the forward kernels form it, in float32: raw scores, the row maximum m, l = sum exp2((s - m) c) with
    c = scale log2 e, lse = m scale + log2(l) ln 2 (__logf is the hardware's log2 times ln 2); -inf on a row with no
    visible key."""
    s = (q.to(f32) @ k.to(f32).transpose(-1, -2)).masked_fill(hid, -math.inf)
    m = s.max(-1).values
    dead = torch.isinf(m)
    c = torch.tensor(scale * LOG2E, dtype=f32)
    l = torch.exp2((s - m.masked_fill(dead, 0.0)[..., None]) * c).sum(-1)
    ln2 = torch.tensor(math.log(2.0), dtype=f32)
    return (m * torch.tensor(scale, dtype=f32) + l.log2() * ln2).masked_fill(dead, -math.inf)


def delta_of(do, o_form, dtype=f64):
    """delta = rowsum(dO o O) over hd. float32: one chain of f32 additions over the hd products, the longest any
    summation order has."""
    prod = do.to(dtype) * o_form.to(dtype)
    if dtype == f64:
        return prod.sum(-1)
    acc = torch.zeros(prod.shape[:-1], dtype=dtype)       # (torch's CPU sum and cumsum of f32 accumulate in f64)
    for i in range(prod.shape[-1]):
        acc = acc + prod[..., i]
    return acc


def scalar_error(got, ref):
    """lse and delta ([B, H, Lq]): deviation() over the rows whose reference is finite (the whole tensor one scale);
    where the reference is -inf (lse of a row with no visible key) `got` has to be -inf too: inf otherwise."""
    got, ref = got.to(f64), ref.to(f64)
    fin = torch.isfinite(ref)
    if not torch.equal(got[~fin], ref[~fin]) or not bool(torch.isfinite(got[fin]).all()):
        return math.inf
    return deviation(got[fin], ref[fin]) if bool(fin.any()) else 0.0


# ---------------------------------------------------------------------------------------------- kernel choice
PATHS = frozenset((
    'fwd32', 'fwd16<64>', 'fwd16<128,96>', 'fwd16<128>', 'split_kv', 'split_kv_empty_slice',
    'bwd8<64,1>', 'bwd8<64,2>', 'bwd8<96,1>', 'bwd8<96,2>', 'bwd4<64>', 'bwd4<128>',
    'dq_direct', 'dq_reduce_f32', 'dq_reduce_bf16', 'dq_reduce_bf16_rot', 'dq_direct_rot',
    'cls_split', 'window_compact',
    'delta_inkernel', 'delta_pass<8>', 'delta_pass<16>', 'delta_ready',
    'dk_rot'))
FWD32_MAXPAD = 4096
BWD_KEYS, BWD8_KEYS, SBLK = 128, 256, 32


def _cdiv(a, b):
    return -(-a // b)


def fwd_split(B, H, Lq, Lk, causal, window):
    """fwd_split: -> (nsplit, kc); nsplit 1 = one pass."""
    nwg = _cdiv(Lq, 128) * H * B
    if causal or window > 0 or Lq > 128 or nwg >= 128 or Lk < 2048:
        return 1, Lk
    sp = min(_cdiv(512, nwg), _cdiv(Lk, 256))
    if sp < 2:
        return 1, Lk
    kc = _cdiv(_cdiv(Lk, sp), 64) * 64
    return _cdiv(Lk, kc), kc


def bwd_layout(B, H, Lq, Lk, hd, causal, window):
    """bwd_layout: -> (use8, nsub, kblk, wrows)"""
    use8 = hd <= 96 and not (Lq <= 64 and hd <= 64)
    nsub = 2 if use8 and Lq >= 512 else 1
    kblk = BWD8_KEYS * nsub if use8 else BWD_KEYS
    wrows = 0
    if use8 and window > 0 and causal:
        R = _cdiv(min(Lq, kblk - SBLK + SBLK * window), 64) * 64
        if _cdiv(Lk, kblk) > 1 and R < Lq:
            wrows = R
    return use8, nsub, kblk, wrows


def dispatch(B, H, Lq, Lk, hd, causal, window, padded, o_extra, delta_ready, dq_kind, rot):
    """The kernel paths svae_attn_fwd and svae_attn_bwd take for this call with the default environment switches
    (PATHS lists the names). padded: None / False, True, or the key_pad mask [B, Lk] itself (needed to tell whether a
    split-KV slice holds padding only); o_extra: 'o_lo', 'o32' or None; dq_kind: 'bf16' (dq_bf) or 'f32' (dq); rot:
    a rotary table is passed. The 32-bit offset limits of launch_fwd and svae_attn_bwd (sequences of 2^31 bytes) are
    not restated: no test shape comes near them."""
    mask = padded if isinstance(padded, torch.Tensor) else None
    padded = mask is not None or bool(padded)
    out = set()
    nsplit, kc = fwd_split(B, H, Lq, Lk, causal, window)
    if nsplit > 1:
        out.add('split_kv')
        if mask is not None and any(bool(mask[b, s * kc:(s + 1) * kc].bool().all()) for b in range(B)
                                    for s in range(nsplit)):
            out.add('split_kv_empty_slice')
    keys = kc if nsplit > 1 else Lk
    if hd <= 64:
        out.add('fwd32' if not padded or keys <= FWD32_MAXPAD else 'fwd16<64>')
    else:
        out.add('fwd16<128,96>' if hd <= 96 else 'fwd16<128>')
    use8, nsub, kblk, wrows = bwd_layout(B, H, Lq, Lk, hd, causal, window)
    if use8:
        out.add(f'bwd8<{64 if hd <= 64 else 96},{nsub}>')
    else:
        out.add('bwd4<64>' if hd <= 64 else 'bwd4<128>')
    dq_direct = ((2 if nsub == 2 and hd <= 64 else 1) * BWD8_KEYS) if use8 and causal else 0
    rot_q = rot and dq_kind == 'bf16'
    if dq_direct:
        out.add('dq_direct_rot' if rot_q else 'dq_direct')
    if Lq > dq_direct:
        out.add('dq_reduce_f32' if dq_kind == 'f32' else 'dq_reduce_bf16_rot' if rot_q else 'dq_reduce_bf16')
    if wrows:
        out.add('window_compact')
    if use8 and window > 0 and causal and _cdiv(min(Lq, kblk - SBLK + SBLK * window), 64) * 64 < Lq:
        out.add('cls_split')
    if delta_ready:
        out.add('delta_ready')
    elif use8 and hd <= 64 and o_extra == 'o_lo':
        out.add('delta_inkernel')
    else:
        out.add('delta_pass<8>' if hd <= 64 else 'delta_pass<16>')
    if rot:
        out.add('dk_rot')
    return out


# ---------------------------------------------------------------------------------------------- cases
Case = collections.namedtuple('Case', 'name form B H Lq Lk hd causal window pad o_extra delta_ready dq_kind rot')


def _case(name, form, B, H, Lq, Lk, hd, *, pad=None, window=0, o_extra='o_lo', delta_ready=False, dq_kind=None,
          rot=True):
    causal = form == 'self'
    dq_kind = dq_kind or ('f32' if form == 'learned' else 'bf16')
    return Case(name, form, B, H, Lq, Lk, hd, causal, window, pad, o_extra, delta_ready, dq_kind, rot)


def _cases():
    c = []
    for hd in (64, 96):
        # engine.py's three backward call forms, a different padded suffix per batch entry
        c.append(_case(f'self_L200_hd{hd}', 'self', 2, 2, 200, 200, hd, pad='suffix'))      # bwd8<.,1>: dQ all direct
        c.append(_case(f'self_L600_hd{hd}', 'self', 2, 2, 600, 600, hd, pad='suffix'))      # bwd8<.,2>: direct + reduce
        c.append(_case(f'cross_200x330_hd{hd}', 'cross', 2, 2, 200, 330, hd, pad='suffix'))
        c.append(_case(f'learned_64x330_hd{hd}', 'learned', 2, 2, 64, 330, hd, pad='suffix'))
        # few queries over many keys: split-KV; padded from key 1500 on: whole slices are padding
        c.append(_case(f'split_64x2100_hd{hd}', 'cross', 1, 2, 64, 2100, hd))
        c.append(_case(f'split_64x2100_hd{hd}_pad1500', 'cross', 1, 2, 64, 2100, hd, pad='from1500'))
    for hd, dq_kind in ((128, 'bf16'), (16, 'f32')):
        for o_extra in ('o32', None):
            c.append(_case(f'self_L130_hd{hd}_{o_extra or "o"}', 'self', 2, 2, 130, 130, hd, o_extra=o_extra,
                           dq_kind=dq_kind, rot=False))
    c.append(_case('self_L4160_hd64', 'self', 1, 1, 4160, 4160, 64, pad='suffix'))          # past FWD32_MAXPAD
    c.append(_case('delta_ready_hd64', 'self', 2, 2, 200, 200, 64, pad='suffix', delta_ready=True))
    c.append(_case('window1_L320_hd64', 'self', 2, 2, 320, 320, 64, window=1, pad='suffix'))
    c.append(_case('window1_L576_hd64', 'self', 2, 2, 576, 576, 64, window=1, pad='suffix'))
    c.append(_case('window2_L320_hd96', 'self', 2, 2, 320, 320, 96, window=2, pad='suffix'))
    # masks: a 70-token sequence in L = 600; isolated padded keys; ragged lengths
    c.append(_case('short70_self_L600', 'self', 2, 2, 600, 600, 64, pad='short70'))
    c.append(_case('short70_cross_200x600', 'cross', 2, 2, 200, 600, 64, pad='short70'))
    c.append(_case('isolated_self_L330', 'self', 2, 2, 330, 330, 64, pad='isolated'))
    c.append(_case('isolated_cross_200x330', 'cross', 2, 2, 200, 330, 64, pad='isolated'))
    c.append(_case('ragged_self_L77', 'self', 2, 2, 77, 77, 64, pad='suffix'))
    c.append(_case('ragged_cross_1x77', 'cross', 2, 2, 1, 77, 64, pad='suffix'))
    # the two edge cases: a fully padded leading key tile pair in a non-causal call; a batch entry with no key at all
    c.append(_case('lead128_cross_200x330', 'cross', 2, 2, 200, 330, 64, pad='lead128'))
    c.append(_case('entry1_padded_self_L200', 'self', 2, 2, 200, 200, 64, pad='entry1'))
    c.append(_case('entry1_padded_cross_200x330', 'cross', 2, 2, 200, 330, 64, pad='entry1'))
    # head sizes off the templates' own (the p.hd != HDC paths)
    for hd in (8, 48, 80, 112):
        c.append(_case(f'self_L200_hd{hd}', 'self', 2, 2, 200, 200, hd, pad='suffix'))
    return tuple(c)


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
ALL_PADDED = {'entry1_padded_self_L200': 1, 'entry1_padded_cross_200x330': 1}    # case -> the batch entry without a key


def pad_of(c):
    """key_pad uint8 [B, Lk] of a case, or None."""
    if c.pad is None:
        return None
    pad = torch.zeros(c.B, c.Lk, dtype=torch.uint8)
    for b in range(c.B):
        if c.pad in ('suffix', 'entry1'):
            pad[b, c.Lk - 1 - 17 * b - 5:] = 1            # 6 and 23 trailing keys
        elif c.pad == 'from1500':
            pad[b, 1500:] = 1
        elif c.pad == 'short70':
            pad[b, 70 - 7 * b:] = 1
        elif c.pad == 'isolated':
            pad[b, [3, 64, 65, 255, 256, c.Lk - 1]] = 1
        elif c.pad == 'lead128':
            pad[b, :128] = 1
            pad[b, c.Lk - 3 * b:] = 1
    if c.pad == 'entry1':
        pad[1] = 1
    return pad


def rot_of(c):
    """The rotary table engine.rotary_table builds ([pos][d / 2] (cos, sin), float32; SparseAttention's base in window
    mode), or None."""
    if not c.rot:
        return None
    d, max_pos = c.H * c.hd, (2 * c.window * 32 if c.window else 10000)
    half = d // 2
    theta = max_pos ** (-torch.arange(half, dtype=f32) / half)
    ang = torch.arange(0, max(c.Lq, c.Lk), dtype=f32)[:, None] * theta
    return torch.stack([ang.cos(), ang.sin()], dim=-1).contiguous()


@functools.lru_cache(maxsize=None)
def inputs(name):
    """q [B or 1, Lq, d], k, v [B, Lk, d], do [B, Lq, d]: bf16 values ~ N(0, 1) drawn on the CPU from the case's seed
    (scores of unit variance); pad; rot. The learned form has one query matrix for the whole batch."""
    c = BY_NAME[name]
    d = c.H * c.hd
    gen = torch.Generator().manual_seed(zlib.crc32(name.encode()))
    q = torch.randn(1 if c.form == 'learned' else c.B, c.Lq, d, generator=gen).to(bf16)
    k, v = (torch.randn(c.B, c.Lk, d, generator=gen).to(bf16) for _ in range(2))
    do = torch.randn(c.B, c.Lq, d, generator=gen).to(bf16)
    return dict(q=q, k=k, v=v, do=do, pad=pad_of(c), rot=rot_of(c))


def _hv(c, x):
    q = x['q'].expand(c.B, -1, -1) if c.form == 'learned' else x['q']
    return heads(q, c.H), heads(x['k'], c.H), heads(x['v'], c.H), heads(x['do'], c.H)


@functools.lru_cache(maxsize=None)
def reference(name):
    """attention() of the case's inputs and the row magnitudes. Shared by the tests; do not modify."""
    c, x = BY_NAME[name], inputs(name)
    hv = _hv(c, x)
    ref = attention(*hv, pad=x['pad'], causal=c.causal, window=c.window, rot=x['rot'], rot_q=c.dq_kind == 'bf16')
    ref['mag'] = magnitudes(*hv, ref)
    return ref


def emulation(name):
    c, x = BY_NAME[name], inputs(name)
    delta = reference(name)['delta'].to(f32) if c.delta_ready else None
    return emulate(*_hv(c, x), pad=x['pad'], causal=c.causal, window=c.window, rot=x['rot'], o_extra=c.o_extra,
                   dq_bf=c.dq_kind == 'bf16', delta=delta)


def dispatch_of(c):
    return dispatch(c.B, c.H, c.Lq, c.Lk, c.hd, c.causal, c.window, pad_of(c), c.o_extra, c.delta_ready, c.dq_kind,
                    c.rot)


def measure(name):
    """The case's share of the constants below: row_error of emulate() against attention() for O, dQ, dK and dV,
    scalar_error of the float32 lse and delta formulas against float64."""
    c, x = BY_NAME[name], inputs(name)
    ref, emu = reference(name), emulation(name)
    out = {k: row_error(emu[k], ref[k], ref['mag'][k]) for k in ('O', 'dQ', 'dK', 'dV')}
    q, k, v, do = _hv(c, x)
    hid = hidden(c.B, c.Lq, c.Lk, x['pad'], c.causal, c.window)
    out['lse'] = scalar_error(lse_f32(q, k, hid, c.hd ** -0.5), ref['lse'])
    form = o_forms(ref['O'], c.o_extra)
    out['delta'] = scalar_error(delta_of(do, form, f32), delta_of(do, form))
    return out


# ---------------------------------------------------------------------------------------------- recorded bounds
# Largest row_error() of emulate() against the float64 reference over CASES (O, dQ, dK, dV), and largest
# scalar_error() of the float32 lse / delta formulas against float64, measured on the CPU by test_attn_ref.py (which
# re-measures them and fails if one has moved by more than a quarter). The GPU bound is TOL_FACTOR times the constant:
# the kernels round at the same places but sum in another order and in f32. delta is compared with the float64 row
# sums over the O the kernels themselves wrote (its own formula), lse with the float64 logsumexp.
# Beside each: the largest value seen from the kernels on an MI355X.
EMU_O = 1.0e-2        # kernels on an MI355X: 9.6e-3 (self_L200_hd112; bound 4.00e-02)
EMU_DQ = 8.9e-3       # kernels on an MI355X: 8.9e-3 (entry1_padded_self_L200; bound 3.56e-02)
EMU_DK = 3.9e-2       # kernels on an MI355X: 1.9e-2 (self_L130_hd128_o32; bound 1.56e-01) (constant: ragged_cross_1x77)
EMU_DV = 1.8e-2       # kernels on an MI355X: 1.8e-2 (ragged_cross_1x77; bound 7.20e-02)
F32_LSE = 6.8e-8      # kernels on an MI355X: 9.6e-8 (self_L4160_hd64; bound 2.72e-07)
F32_DELTA = 8.5e-7    # kernels on an MI355X: 5.7e-7 (self_L4160_hd64, the in-kernel delta; bound 3.40e-06)
RECORDED = {'O': EMU_O, 'dQ': EMU_DQ, 'dK': EMU_DK, 'dV': EMU_DV, 'lse': F32_LSE, 'delta': F32_DELTA}


def bound(key):
    return TOL_FACTOR * RECORDED[key]
