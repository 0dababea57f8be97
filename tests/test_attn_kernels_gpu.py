"""The flash attention kernels (svae.h "Flash attention": svae_attn_fwd, svae_attn_bwd) per row, on every path of
their dispatch, in the call forms engine.py uses, against the float64 restatement of tests/attn_ref.py.

One test over attn_ref.CASES (test_attn_ref.py requires the cases to reach every path name of attn_ref.dispatch):
  operands   packed as engine.py packs them: qkv rows of stride 3 d (self-attention), q of stride d with kv of stride
             2 d (cross attention), one [Lq, d] query matrix for the batch with bq = 0 (learned queries); bf16 dQ with
             the inverse rotary into the packed gradient matrix (ldq_bf = 3 d or d) or f32 dQ; the rotary on dK; o_lo,
             o32 or neither; delta_ready
  outputs    every one a view into a sentinel-filled buffer (sentinels.py); O, o_lo and o32 have 8 sentinel columns
             after their d (so = d + 8), the packed gradient matrices sentinel rows after them, and dq_part and the
             split-KV workspace are exactly as long as the library's size queries say, plus a guard
  measure    attn_ref.row_error per (batch, head, position) row against the magnitude of the row's own contraction:
             O, dQ, dK, dV within TOL_FACTOR x the bf16 rounding budget (attn_ref.emulate, measured on the CPU); rows
             without magnitude (padded keys, a batch entry with no visible key) exactly zero; lse against the float64
             logsumexp and delta against the float64 row sums over the O the kernels wrote, within TOL_FACTOR x the
             f32-vs-f64 distance of their formulas
  also       the backward run twice is bit-identical (no float atomics); with delta_ready the supplied delta comes back
             unchanged; the library's workspace queries agree with attn_ref.dispatch (split_kv, window_compact)"""
import pytest
import torch

import attn_ref as R
from sentinels import SENTINEL, dev, flat, g, intact, matrix, report

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae._native import lib

f32, bf16 = torch.float32, torch.bfloat16
OPAD = 8                          # sentinel columns after O, o_lo and o32


def _operands(c, x):
    """The device operands in the case's call form -> (q, k, v, stride arguments)."""
    d = c.H * c.hd
    if c.form == 'self':
        qkv = g(torch.cat([x['q'], x['k'], x['v']], -1).view(c.B * c.Lq, 3 * d).contiguous())
        return qkv, qkv[:, d:], qkv[:, 2 * d:], dict(sq=3 * d, bq=c.Lq * 3 * d, sk=3 * d, sv=3 * d, bk=c.Lk * 3 * d,
                                                     bv=c.Lk * 3 * d)
    kv = g(torch.cat([x['k'], x['v']], -1).view(c.B * c.Lk, 2 * d).contiguous())
    q = g(x['q'].reshape(-1, d).contiguous())
    return q, kv, kv[:, d:], dict(sq=d, bq=0 if c.form == 'learned' else c.Lq * d, sk=2 * d, sv=2 * d,
                                  bk=c.Lk * 2 * d, bv=c.Lk * 2 * d)


class _Grads:
    """The backward's outputs in the call form's layout, each in a sentinel buffer."""

    def __init__(self, c):
        d, rq, rk = c.H * c.hd, c.B * c.Lq, c.B * c.Lk
        self.c, self.d = c, d
        self.delta_full, self.delta = flat(c.B * c.H * c.Lq)
        self.dq32_full = self.dqbf_full = None
        if c.form == 'self':
            self.kv_full, kv = matrix(rk, 3 * d, 3 * d, bf16)
            self.dk, self.dv, self.ldkv = kv[:, d:2 * d], kv[:, 2 * d:], 3 * d
            if c.dq_kind == 'bf16':
                self.dq_bf, self.ldq_bf = kv[:, :d], 3 * d
        else:
            self.kv_full, kv = matrix(rk, 2 * d, 2 * d, bf16)
            self.dk, self.dv, self.ldkv = kv[:, :d], kv[:, d:], 2 * d
            if c.dq_kind == 'bf16':
                self.dqbf_full, self.dq_bf = matrix(rq, d, d, bf16)
                self.ldq_bf = d
        if c.dq_kind == 'f32':
            self.dq32_full, self.dq32 = flat(rq * d)
        n = K.attn_dq_part_elems(c.B, c.H, c.Lq, c.Lk, c.hd, c.window)
        self.part_full, self.part = flat(n)

    def args(self):
        c, d = self.c, self.d
        a = dict(delta=self.delta, dk=self.dk, dv=self.dv, sdk=self.ldkv, sdv=self.ldkv, bdk=c.Lk * self.ldkv,
                 bdv=c.Lk * self.ldkv, dq_part=self.part)
        if c.dq_kind == 'bf16':
            a.update(dq_bf=self.dq_bf, ldq_bf=self.ldq_bf)
        else:
            a.update(dq=self.dq32, bdq=c.Lq * d)
        return a

    def check_sentinels(self):
        c, d = self.c, self.d
        assert intact(self.delta_full) and intact(self.part_full)
        assert intact(self.kv_full, c.B * c.Lk, self.kv_full.shape[1])
        if c.form == 'self' and c.dq_kind == 'f32':          # the packed matrix's q columns are nobody's output here
            assert bool((self.kv_full[:, :d] == torch.tensor(SENTINEL, dtype=bf16)).all())
        if self.dqbf_full is not None:
            assert intact(self.dqbf_full, c.B * c.Lq, d)
        if self.dq32_full is not None:
            assert intact(self.dq32_full)

    def buffers(self):
        return [t for t in (self.delta_full, self.kv_full, self.dqbf_full, self.dq32_full) if t is not None]

    def dq(self):
        t = self.dq_bf if self.c.dq_kind == 'bf16' else self.dq32.view(self.c.B * self.c.Lq, self.d)
        return t.float().cpu()


def _heads(c, t, L):
    return R.heads(t.reshape(c.B, L, c.H * c.hd), c.H)


@pytest.mark.parametrize('name', [c.name for c in R.CASES])
def test_attention_case(name):
    c, x, ref = R.BY_NAME[name], R.inputs(name), R.reference(name)
    paths = R.dispatch_of(c)
    print(f'{name}: {sorted(paths)}')
    B, H, Lq, Lk, hd, d = c.B, c.H, c.Lq, c.Lk, c.hd, c.H * c.hd
    rq = B * Lq

    # the restatement of the dispatch against the library's own workspace queries
    n_ws = lib.svae_attn_fwd_ws_elems(B, H, Lq, Lk, hd, int(c.causal), c.window)
    assert (n_ws > 0) == ('split_kv' in paths)
    n_dense = lib.svae_attn_dq_part_elems(B, H, Lq, Lk, hd)
    n_part = lib.svae_attn_dq_part_elems_w(B, H, Lq, Lk, hd, c.window)
    assert (n_part < n_dense) == ('window_compact' in paths) and n_part <= n_dense

    q, k, v, strides = _operands(c, x)
    pad = None if x['pad'] is None else g(x['pad'])
    rot = None if x['rot'] is None else g(x['rot'])
    ld = d + OPAD
    o_full, o = matrix(rq, d, ld, bf16)
    lse_full, lse = flat(B * H * Lq)
    common = dict(B=B, H=H, Lq=Lq, Lk=Lk, hd=hd, so=ld, bo=Lq * ld, key_pad=pad, causal=c.causal, window=c.window,
                  **strides)
    extra, x_full, xo = {}, None, None
    if c.o_extra == 'o_lo':
        x_full, xo = matrix(rq, d, ld, bf16)
        extra = dict(o_lo=xo, so_lo=ld, bo_lo=Lq * ld)
    elif c.o_extra == 'o32':
        x_full, xo = matrix(rq, d, ld, f32)
        extra = dict(o32=xo, so32=ld, bo32=Lq * ld)

    # ---- forward (the split-KV workspace: exactly the library's size, in the slot kernels.attention takes it from)
    ws_full = None
    if n_ws > 0:
        ws_full, ws = flat(n_ws)
        K._fwd_ws[q.device] = ws
    try:
        K.attention(q, k, v, o, lse.view(B, H, Lq), **extra, **common)
        torch.cuda.synchronize()
    finally:
        K._fwd_ws.pop(q.device, None)
    assert intact(o_full, rq, d) and intact(lse_full)
    assert x_full is None or intact(x_full, rq, d)
    assert ws_full is None or intact(ws_full)
    o_cpu, lse_cpu = o.float().cpu(), lse.cpu().view(B, H, Lq)
    report('O', R.row_error(_heads(c, o_cpu, Lq), ref['O'], ref['mag']['O']), R.bound('O'))
    report('lse', R.scalar_error(lse_cpu, ref['lse']), R.bound('lse'))
    if xo is not None:
        assert bool(torch.isfinite(xo).all())

    # ---- backward, twice
    do = g(x['do'].view(rq, d))
    runs = []
    for _ in range(2):
        gr = _Grads(c)
        if c.delta_ready:
            gr.delta.copy_(g(ref['delta'].to(f32).reshape(-1)))
        K.attention(q, k, v, o, lse.view(B, H, Lq), backward=True, dout=do, sdo=d, bdo=Lq * d, rot=rot,
                    rot_d=d if rot is not None else 0, delta_ready=c.delta_ready, **gr.args(), **extra, **common)
        torch.cuda.synchronize()
        gr.check_sentinels()
        runs.append(gr)
    assert intact(o_full, rq, d) and intact(lse_full) and (x_full is None or intact(x_full, rq, d))
    for a, b in zip(runs[0].buffers(), runs[1].buffers()):
        assert torch.equal(a, b)                              # bit-identical: no float atomics, no stale slot
    gr = runs[0]

    delta = gr.delta.cpu().view(B, H, Lq)
    if c.delta_ready:
        assert torch.equal(delta, ref['delta'].to(f32))       # read, not written
    else:
        form = o_cpu.double()
        if c.o_extra is not None:
            form = xo.cpu().double() + (form if c.o_extra == 'o_lo' else 0.0)
        want = R.delta_of(_heads(c, x['do'], Lq), _heads(c, form, Lq))
        report('delta', R.scalar_error(delta, want), R.bound('delta'))
    got = dict(dQ=_heads(c, gr.dq(), Lq), dK=_heads(c, gr.dk.float().cpu(), Lk), dV=_heads(c, gr.dv.float().cpu(), Lk))
    for key in ('dQ', 'dK', 'dV'):
        report(key, R.row_error(got[key], ref[key], ref['mag'][key]), R.bound(key))

    if name in R.ALL_PADDED:                                  # the entry without a key: zeros, lse = -inf, nothing else
        b = R.ALL_PADDED[name]
        assert bool((o_cpu.view(B, Lq, d)[b] == 0).all()) and bool((lse_cpu[b] == -float('inf')).all())
        assert all(bool((t[b] == 0).all()) for t in got.values())
        assert all(bool(torch.isfinite(t).all()) for t in (o_cpu, delta, *got.values()))
