"""KV-cache decoding of TransformerVAE.sample (transformer_vae.py:95-128) on libsvae, in f32.

One decode step = for every decoder layer: LayerNorm -> fused q|k|v linear with rotary at position cur-1 ->
cache append + attention over the visible keys -> output linear (+ residual) -> LayerNorm -> FFN (GELU) (+
residual); then the output head (Linear, GELU, LayerNorm, tied vocabulary Linear), the repetition penalty
and the sampler, which writes the next id and the live mask, and `cur += 1`. Every kernel reads the position
from the device scalar `cur`, so the step for positions >= 2 is captured once as a HIP graph
(torch.cuda.CUDAGraph) and replayed. Step 1 differs (each layer's input is z_projections[i](z),
transformer_vae.py:119-121) and runs eagerly.

Finished rows are not compacted as the reference does (Attention.update_kv_cache, attention.py:162-168): their
ids stop changing (the sampler skips rows whose live flag is clear), which keeps the step's shapes fixed for
the graph. Rows are independent, so the surviving rows' outputs are the same.

The KV cache holds every position ([layers][B][H][T][hd] f32); with sparse_self_attention the attention kernel
reads exactly the keys the reference's sliding-window cache keeps (attention.py:115-140).

StreamDecoder (below) is the bulk generator: the same step with one position per row, finished rows refilled on
the device with the next sample, for `TransformerVAE.sample_stream`.
"""
import math
from types import SimpleNamespace
from typing import NamedTuple, Optional

import torch

from . import kernels as K
from ._native import BEAM_MAX_W, EPI_F32, EPI_GELU, EPI_ROTARY_BF16

f32 = torch.float32


class KVDecoder:
    def __init__(self, engine, state, z, use_graph=True):
        self.eng, self.st = engine, state
        P, hp = engine.P, engine.hp
        self.P = P
        B, T = state.output_ids.shape
        d, H, NL, V = engine.d, engine.H, hp.num_layers, hp.vocab_size
        self.B, self.T, self.d, self.H, self.hd, self.NL, self.V = B, T, d, H, engine.hd, NL, V
        self.window = engine.window
        dev = P.device
        self.z = z.reshape(B, -1).to(dev, f32).contiguous()
        self.kc = torch.empty(NL, B, H, T, self.hd, device=dev, dtype=f32)
        self.vc = torch.empty_like(self.kc)
        self.rot = engine.rot(T, self.window)
        e = lambda *s: torch.empty(*s, device=dev, dtype=f32)   # noqa: E731
        self.x, self.xin, self.h, self.x1 = e(B, d), e(B, d), e(B, d), e(B, d)
        self.qkv, self.O, self.f = e(B, 3 * d), e(B, d), e(B, 4 * d)
        self.h0, self.hh, self.logits = e(B, d), e(B, d), e(B, V)
        self.part = e(16 * B * 4 * d)          # split-K partials of the narrow linears (<= 16 splits)
        self.use_graph = use_graph
        self.graph = None

    # ------------------------------------------------------------------ one layer (transformer_layer.py:44-61)
    def _layer(self, i, x_in, x_out):
        P, B, d, st = self.P, self.B, self.d, self.st
        pre = f'decoder_layers.{i}.'
        a = pre + 'attention.'
        K.layernorm_fwd_f32(x_in, P.f(pre + 'attn_layer_norm.weight'), P.f(pre + 'attn_layer_norm.bias'), self.h, B, d)
        # q | k | v weights and biases are adjacent in the arena: one [3d, d] operand; rotary on q and k
        K.dec_linear(self.h, P.f(a + 'q_linear.weight'), self.qkv, B, 3 * d, d, bias=P.f(a + 'q_linear.bias'),
                     epi=EPI_ROTARY_BF16, rot=self.rot, rot_cols=2 * d, rot_d=d, cur=st.cur, part=self.part)
        self._attn(i)
        K.dec_linear(self.O, P.f(a + 'output_linear.weight'), self.x1, B, d, d, bias=P.f(a + 'output_linear.bias'),
                     resid=x_in, part=self.part)
        K.layernorm_fwd_f32(self.x1, P.f(pre + 'ffn_layer_norm.weight'), P.f(pre + 'ffn_layer_norm.bias'), self.h, B, d)
        K.dec_linear(self.h, P.f(pre + 'ffn.0.weight'), self.f, B, 4 * d, d, bias=P.f(pre + 'ffn.0.bias'), epi=EPI_GELU,
                     part=self.part)
        K.dec_linear(self.f, P.f(pre + 'ffn.2.weight'), x_out, B, d, 4 * d, resid=self.x1, part=self.part)

    def _attn(self, i):
        K.dec_attn(self.qkv, self.kc[i], self.vc[i], self.O, self.B, self.H, self.hd, self.T, self.st.cur, self.window)

    def _choose(self):
        """GenerationState.process_logits (generation.py:30-77) on all rows; dead rows are skipped in-kernel."""
        B, st = self.B, self.st
        if st.repetition_penalty > 1.0:
            K.dec_penalty(self.logits, B, None, st.output_ids, self.T, st.cur, st.live_sample_mask,
                          float(st.repetition_penalty))
        K.dec_sample(self.logits, self.V, B, None, st.output_ids, self.T, st.cur, st.live_sample_mask,
                     int(st.end_token), float(st.temperature), int(st.top_k), float(st.top_p), st.seed, st.live_count)
        K.dec_advance(st.cur)

    def _step(self, first):
        P, B, d, st = self.P, self.B, self.d, self.st
        Z = self.z.shape[1]
        if not first:
            K.dec_embed(st.output_ids, self.T, st.cur, P.f('input_layer.0.weight'), self.x, B, d)
        for i in range(self.NL):
            if first:    # transformer_vae.py:119-120: the layer input is z_projections[i](z) at current_index 1
                K.dec_linear(self.z, P.f(f'z_projections.{i}.weight'), self.xin, B, d, Z,
                             bias=P.f(f'z_projections.{i}.bias'))
                self._layer(i, self.xin, self.x)
            else:
                self._layer(i, self.x, self.x)
        # output_layer (transformer_language_model.py:55-63)
        K.dec_linear(self.x, P.f('output_layer.0.weight'), self.h0, B, d, d, bias=P.f('output_layer.0.bias'),
                     epi=EPI_GELU, part=self.part)
        K.layernorm_fwd_f32(self.h0, P.f('output_layer.2.weight'), P.f('output_layer.2.bias'), self.hh, B, d)
        K.dec_linear(self.hh, P.f('input_layer.0.weight'), self.logits, B, self.V, d, bias=P.f('output_layer.3.bias'))
        self._choose()

    def run(self, check_every=8):
        """The reference's `while not state.should_stop()` loop (transformer_vae.py:114-126)."""
        st = self.st
        if st.should_stop():
            return st.final_output()
        self._step(first=True)
        st.step_done()
        n = 0
        while st.current_index < self.T - 1:
            if n % check_every == 0 and int(st.live_count.item()) == 0:
                break
            if self.use_graph:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
            else:
                self._step(first=False)
            st.step_done()
            n += 1
        return st.final_output()

    def _capture(self):
        """Capture one generic step. The warm-up/capture launches would advance the device state, so it is
        saved and restored around the capture."""
        st = self.st
        saved = (st.output_ids.clone(), st.live_sample_mask.clone(), st.cur.clone(), st.live_count.clone(),
                 self.kc.clone(), self.vc.clone())
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step(first=False)          # warm-up outside the graph
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step(first=False)
        st.output_ids.copy_(saved[0])
        st.live_sample_mask.copy_(saved[1])
        st.cur.copy_(saved[2])
        st.live_count.copy_(saved[3])
        self.kc.copy_(saved[4])
        self.vc.copy_(saved[5])
        self.graph = g


class StreamDecoder:
    """Bulk unconditional sampling (the reference's sample.py + batch_generation.py workload) as a stream: S slots,
    each decoding one sample at its own position; a slot whose sample ends is refilled on the device with the next
    sample number in the same step, so all S rows stay busy until the last samples drain. The step has static
    shapes and reads every position from the device (`pos[s]`), so it is captured once and replayed.

    One step: slot_embed -> per layer (slot_splice of z_projections[i](z) into the rows at position 1, LayerNorm,
    q|k|v slot_linear with rotary at pos-1, slot_attn, output linear, LayerNorm, FFN) -> output head ->
    slot_penalty -> slot_sample (token into ids and into the result buffer, advance or finish) -> slot_refill ->
    the z projections of the slots' latents for the next step. The arithmetic per row is KVDecoder's, kernel for
    kernel (the same bodies, the same split rule through a `part` workspace of the same 16 * S * 4d floats), so
    sample j equals row j of `sample()` on the same z and seed while the slot count stays within the same number
    of 64-row blocks (the split rule reads the block count).

    A refilled slot reuses its cache rows as they are: at position p only keys <= p are read, and each is written
    by the sample's own earlier steps.
    """

    def __init__(self, engine, num_samples, max_length, slots, z, start_token, end_token, *, top_k=0, top_p=0.9,
                 temperature=1.0, repetition_penalty=1.2, seed=0, use_graph=True):
        P, hp = engine.P, engine.hp
        self.eng, self.P = engine, P
        dev = P.device
        if dev.type != 'cuda':
            raise RuntimeError('StreamDecoder runs on the MI355X kernels: pass a GPU engine (no CPU fallback)')
        N, T, S = int(num_samples), int(max_length), int(slots)
        if N < 1 or S < 1 or not 3 <= T <= 32768:
            raise ValueError(f'StreamDecoder: num_samples {N}, slots {S}, max_length {T} (3..32768)')
        d, H, NL, V = engine.d, engine.H, hp.num_layers, hp.vocab_size
        self.N, self.T, self.S, self.d, self.H, self.hd, self.NL, self.V = N, T, S, d, H, engine.hd, NL, V
        self.window = engine.window
        self.start, self.end = int(start_token), int(end_token)
        self.top_k, self.top_p, self.temperature = int(top_k), float(top_p), float(temperature)
        self.repetition_penalty, self.seed = float(repetition_penalty), int(seed)
        self.z_all = z.reshape(N, -1).to(dev, f32).contiguous()
        Z = self.z_all.shape[1]
        i32 = lambda v: torch.full((S,), v, device=dev, dtype=torch.int32)   # noqa: E731
        self.pos, self.key = i32(-1), i32(-1)            # every slot "finished" without a sample: the first refill
        self.next = torch.zeros(1, device=dev, dtype=torch.int32)
        self.completed = torch.zeros(1, device=dev, dtype=torch.int32)
        self.ids = torch.zeros(S, T, device=dev, dtype=torch.long)
        self.out = torch.zeros(N, T - 1, device=dev, dtype=torch.int16)
        z_ = lambda *s: torch.zeros(*s, device=dev, dtype=f32)   # noqa: E731  (idle rows stay finite)
        # every layer's z projection as one [NL * d, Z] operand (a packed copy: the arena interleaves them with
        # the layers), so the slots' latents are projected by one launch into zp [S, NL * d]; a row's dot products
        # do not depend on how many output columns the launch has
        self.z_slot, self.zp = z_(S, Z), z_(S, NL * d)
        self.wz = torch.cat([P.f(f'z_projections.{i}.weight').reshape(d, Z) for i in range(NL)]).contiguous()
        self.bz = torch.cat([P.f(f'z_projections.{i}.bias').reshape(d) for i in range(NL)]).contiguous()
        self.kc = torch.empty(NL, S, H, T, self.hd, device=dev, dtype=f32)
        self.vc = torch.empty_like(self.kc)
        self.rot = engine.rot(T, self.window)
        self.x, self.h, self.x1 = z_(S, d), z_(S, d), z_(S, d)
        self.qkv, self.O, self.f = z_(S, 3 * d), z_(S, d), z_(S, 4 * d)
        self.h0, self.hh, self.logits = z_(S, d), z_(S, d), z_(S, V)
        self.part = z_(16 * S * 4 * d)
        self.use_graph = use_graph
        self.graph = None
        self.steps = 0

    def _layer(self, i):
        P, S, d = self.P, self.S, self.d
        pre = f'decoder_layers.{i}.'
        a = pre + 'attention.'
        x = self.x
        K.slot_splice(x, self.zp[:, i * d:], self.pos, S, d, ldz=self.NL * d)
        K.layernorm_fwd_f32(x, P.f(pre + 'attn_layer_norm.weight'), P.f(pre + 'attn_layer_norm.bias'), self.h, S, d)
        K.slot_linear(self.h, P.f(a + 'q_linear.weight'), self.qkv, S, 3 * d, d, bias=P.f(a + 'q_linear.bias'),
                      rot=self.rot, rot_cols=2 * d, rot_d=d, pos=self.pos, part=self.part)
        K.slot_attn(self.qkv, self.kc[i], self.vc[i], self.O, S, self.H, self.hd, self.T, self.pos, self.window)
        K.dec_linear(self.O, P.f(a + 'output_linear.weight'), self.x1, S, d, d, bias=P.f(a + 'output_linear.bias'),
                     resid=x, part=self.part)
        K.layernorm_fwd_f32(self.x1, P.f(pre + 'ffn_layer_norm.weight'), P.f(pre + 'ffn_layer_norm.bias'), self.h, S, d)
        K.dec_linear(self.h, P.f(pre + 'ffn.0.weight'), self.f, S, 4 * d, d, bias=P.f(pre + 'ffn.0.bias'), epi=EPI_GELU,
                     part=self.part)
        K.dec_linear(self.f, P.f(pre + 'ffn.2.weight'), x, S, d, 4 * d, resid=self.x1, part=self.part)

    def _refill(self):
        """Hand finished slots their next samples, then project the slots' latents for the step that follows
        (KVDecoder's first-step arithmetic: an un-split dec_linear, here over all layers' columns at once)."""
        S = self.S
        K.slot_refill(self.pos, self.key, self.ids, self.T, S, self.start, self.z_all, self.z_slot, self.N, self.next,
                      self.completed)
        K.dec_linear(self.z_slot, self.wz, self.zp, S, self.NL * self.d, self.z_slot.shape[1], bias=self.bz)

    def _step(self):
        P, S, d = self.P, self.S, self.d
        K.slot_embed(self.ids, self.T, self.pos, P.f('input_layer.0.weight'), self.x, S, d)
        for i in range(self.NL):
            self._layer(i)
        K.dec_linear(self.x, P.f('output_layer.0.weight'), self.h0, S, d, d, bias=P.f('output_layer.0.bias'),
                     epi=EPI_GELU, part=self.part)
        K.layernorm_fwd_f32(self.h0, P.f('output_layer.2.weight'), P.f('output_layer.2.bias'), self.hh, S, d)
        K.dec_linear(self.hh, P.f('input_layer.0.weight'), self.logits, S, self.V, d, bias=P.f('output_layer.3.bias'))
        if self.repetition_penalty > 1.0:
            K.slot_penalty(self.logits, S, self.ids, self.T, self.pos, self.repetition_penalty)
        K.slot_sample(self.logits, self.V, S, self.ids, self.T, self.pos, self.key, self.out, self.N, self.end,
                      self.temperature, self.top_k, self.top_p, self.seed)
        self._refill()

    def max_steps(self):
        """Every sample takes at most T - 2 steps and a slot is never idle while samples remain."""
        return (-(-self.N // self.S) + 1) * (self.T - 1)

    def run(self, check_every=8):
        """Fill the slots, then step until the device has counted num_samples completed samples. The host reads
        that counter every `check_every` steps and at no other time."""
        self._refill()
        bound = self.max_steps()
        while True:
            if self.steps % check_every == 0 or self.steps >= bound:
                done = int(self.completed.item())
                if done >= self.N:
                    break
                if self.steps >= bound:
                    raise RuntimeError(f'StreamDecoder: {done} of {self.N} samples after {self.steps} steps '
                                       f'(bound {bound})')
            if self.use_graph:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
            else:
                self._step()
            self.steps += 1
        return self.out

    def _capture(self):
        """Capture one step. The warm-up launch advances the device state, so it is saved and restored around the
        capture, as KVDecoder._capture does. The KV cache is not part of it: the warm-up wrote, at each slot's
        position, the rows the first replay writes again from the same restored state."""
        state = (self.pos, self.key, self.next, self.completed, self.ids, self.out, self.z_slot, self.zp)
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step()                     # warm-up outside the graph
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step()
        for t, v in zip(state, saved):
            t.copy_(v)
        self.graph = g


class BeamResult(NamedTuple):
    """TransformerVAE.beam_search's result: the best `num_return` hypotheses of each document, best first."""
    ids: torch.Tensor            # int64 [B, n, T - 1]: start token excluded, zero after the end token
    scores: torch.Tensor         # f32 [B, n]: log_probs / length ** length_penalty
    log_probs: torch.Tensor      # f32 [B, n]: the un-normalised sums
    lengths: torch.Tensor        # int32 [B, n]: generated tokens, the end token included
    history: Optional[dict] = None   # parent, token int32 and score f32 [T, R] of every step's new rows


class BeamState:
    """The device state of a beam search (include/svae.h "beam search decoding"): per row the cumulative
    log-probability, the id row and the ancestry row; per document the pool of finished hypotheses and the done
    flag; the step index `cur`. Every buffer keeps its address over a decode."""

    def __init__(self, B, W, T, start_token, end_token, alpha, device, history=False):
        B, W, T = int(B), int(W), int(T)
        if not 1 <= W <= BEAM_MAX_W:
            raise ValueError(f'num_beams {W}: 1..{BEAM_MAX_W}')
        if B < 1 or not 3 <= T <= 32768 or B * W > 65535:
            raise ValueError(f'beam search: {B} documents x {W} beams (at most 65535 rows), max_length {T} (3..32768)')
        self.B, self.W, self.T, self.alpha = B, W, T, float(alpha)
        self.start_token, self.end_token = int(start_token), int(end_token)
        R, dev = B * W, torch.device(device)
        z = lambda dt, *s: torch.zeros(*s, device=dev, dtype=dt)   # noqa: E731
        self.cum = torch.full((B, W), -math.inf, device=dev, dtype=f32)
        self.cum[:, 0] = 0.0                                       # step 1 expands one hypothesis per document
        self.ids, self.ids_next = z(torch.int64, R, T), z(torch.int64, R, T)
        self.ids[:, 0] = self.start_token
        self.anc, self.anc_next = z(torch.uint8, R, T), z(torch.uint8, R, T)
        self.cur = torch.ones(1, device=dev, dtype=torch.int32)
        # l ** alpha in float64, rounded once: the kernels and the float64 reference divide by the same numbers
        self.len_pen = torch.arange(T, dtype=torch.float64).clamp_(min=1).pow_(self.alpha).to(f32).to(dev)
        self.pool_score, self.pool_logp = z(f32, B, W), z(f32, B, W)
        self.pool_len, self.pool_ids, self.pool_n = z(torch.int32, B, W), z(torch.int64, B, W, T), z(torch.int32, B)
        self.done, self.stamp = z(torch.uint8, B), z(torch.int32, B)
        self.not_done = torch.full((1,), B, device=dev, dtype=torch.int32)
        self.cand_score, self.cand_tok = z(f32, R, 2 * W), z(torch.int32, R, 2 * W)
        self.hist_parent = self.hist_token = self.hist_score = None
        if history:
            self.hist_parent = torch.full((T, R), -1, device=dev, dtype=torch.int32)
            self.hist_token = torch.full((T, R), -1, device=dev, dtype=torch.int32)
            self.hist_score = torch.full((T, R), -math.inf, device=dev, dtype=f32)

    def tensors(self):
        """Everything a step changes (what a graph capture saves and restores)."""
        ts = [self.cum, self.ids, self.anc, self.cur, self.pool_score, self.pool_logp, self.pool_len, self.pool_ids,
              self.pool_n, self.done, self.stamp, self.not_done]
        return ts + [t for t in (self.hist_parent, self.hist_token, self.hist_score) if t is not None]

    def history(self):
        if self.hist_parent is None:
            return None
        return dict(parent=self.hist_parent, token=self.hist_token, score=self.hist_score)


class BeamDecoder(KVDecoder):
    """Beam search over p(x|z): KVDecoder's step on R = B * W rows (row b * W + w is hypothesis w of document b; z
    repeated per beam), with beam_attn for dec_attn and beam_topk -> beam_select -> dec_advance for dec_sample. The
    hypotheses are reordered every step, the KV caches never: attention finds a hypothesis's key j in the cache row
    its ancestry row names. Step 1 runs eagerly, the generic step is captured once and replayed on one stream; the
    host reads the count of documents not done every `check_every` steps."""

    def __init__(self, engine, z, max_length, num_beams, start_token, end_token, *, length_penalty=1.0,
                 repetition_penalty=1.0, use_graph=True, history=False):
        dev = engine.P.device
        if dev.type != 'cuda':
            raise RuntimeError('BeamDecoder runs on the MI355X kernels: pass a GPU engine (no CPU fallback)')
        B = z.shape[0]
        self.beam = BeamState(B, num_beams, max_length, start_token, end_token, length_penalty, dev, history=history)
        self.W, self.docs = self.beam.W, B
        self.repetition_penalty = float(repetition_penalty)
        # KVDecoder reads the id rows and the position through its state
        state = SimpleNamespace(output_ids=self.beam.ids, cur=self.beam.cur)
        zr = z.reshape(B, -1).to(dev, f32).repeat_interleave(self.W, dim=0)
        super().__init__(engine, state, zr, use_graph=use_graph)
        if self.V < 2 * self.W:
            raise ValueError(f'num_beams {self.W}: the vocabulary has {self.V} entries (2 * num_beams at least)')

    def _attn(self, i):
        K.beam_attn(self.qkv, self.kc[i], self.vc[i], self.beam.anc, self.O, self.B, self.W, self.H, self.hd, self.T,
                    self.beam.cur, self.window)

    def _choose(self):
        bs, R = self.beam, self.B
        if self.repetition_penalty > 1.0:
            K.dec_penalty(self.logits, R, None, bs.ids, self.T, bs.cur, None, self.repetition_penalty)
        K.beam_topk(self.logits, self.V, R, self.W, bs.cum, bs.done, bs.cand_score, bs.cand_tok)
        K.beam_select(bs.cand_score, bs.cand_tok, bs)
        K.dec_advance(bs.cur)

    def run(self, num_return=1, check_every=8):
        bs, T = self.beam, self.T
        if not 1 <= num_return <= self.W:
            raise ValueError(f'num_return {num_return}: 1..num_beams ({self.W})')
        self._step(first=True)
        c, n = 2, 0                                  # c mirrors *cur: the index of the token the next step generates
        while c <= T - 2:
            if n % check_every == 0 and int(bs.not_done.item()) == 0:
                break
            if self.use_graph:
                if self.graph is None:
                    self._capture()
                self.graph.replay()
            else:
                self._step(first=False)
            c += 1
            n += 1
        self.steps = c - 1
        return BeamResult(*K.beam_finalize(bs, int(num_return)), bs.history())

    def _capture(self):
        """Capture one generic step on one stream. The warm-up launch advances the device state, so it is saved and
        restored around the capture; the KV caches are not part of it: the warm-up wrote, in every row at the
        current position, what the first replay writes again from the same restored state."""
        state = self.beam.tensors()
        saved = [t.clone() for t in state]
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            self._step(first=False)          # warm-up outside the graph
        torch.cuda.current_stream().wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            self._step(first=False)
        for t, v in zip(state, saved):
            t.copy_(v)
        self.graph = g
