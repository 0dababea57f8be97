"""Beam search step time on one MI355X: the C2 decoder (6 layers, d 512, 8 heads, random weights) at 64 documents x
4 beams, max_length 512, no end token (every decode runs all 510 steps, so the attention cost at every position is in
the figure).

    python scripts/bench_beam.py [--docs 64] [--beams 4] [--max-length 512] [--repeats 3] [--out profiles/beam_bench.log]

Three figures, each the wall time of whole decodes (host clock around work that ends in a device synchronise) over
their step count, after a warm-up decode of the same shape:
* table: TransformerVAE.beam_search as shipped -- the captured step with svae_beam_attn reading the caches through the
  ancestry table; the caches never move.
* copy:  the same captured step with svae_dec_attn, and after the selection both caches of all layers reordered by
  torch index_select with each row's parent (the form the table replaces: [layers][R][H][T][hd] f32 read and written
  once per step).
* greedy: KVDecoder (`sample` at temperature 0) on docs * beams rows, the floor: the same rows without any search.
The decodes of `table` and `copy` must give the same ids; the log says whether they did.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--docs', type=int, default=64)
    ap.add_argument('--beams', type=int, default=4)
    ap.add_argument('--max-length', type=int, default=512)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'beam_bench.log'))
    a = ap.parse_args()
    from sparse_vae import TransformerVAE, TransformerVAEHparams
    from sparse_vae import kernels as K
    from sparse_vae.decoding import BeamDecoder
    assert torch.cuda.is_available(), 'bench_beam.py measures on the GPU'
    dev = torch.device('cuda', 0)
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    hp = TransformerVAEHparams(d_model=512, num_layers=6, num_heads=8, latent_depth=64, sparse_self_attention=False,
                               kl_weight=1.0)
    model = TransformerVAE(hp, device=dev)
    model.initialize_weights()
    model.eval()
    model.start_token, model.end_token = 1, -1
    B, W, T = a.docs, a.beams, a.max_length
    R = B * W
    z = torch.randn(B, 1, 64, device=dev)
    eng = model._require_engine()

    class CopyDecoder(BeamDecoder):
        """The step with physically reordered caches: dec_attn on the row's own cache row, then every row takes its
        parent's cache rows (the parent is the ancestry entry the selection just wrote at position cur - 2)."""

        def _attn(self, i):
            K.dec_attn(self.qkv, self.kc[i], self.vc[i], self.O, self.B, self.H, self.hd, self.T, self.beam.cur,
                       self.window)

        def _capture(self):
            kc, vc = self.kc.clone(), self.vc.clone()    # the warm-up step moves the caches: put them back
            super()._capture()
            self.kc.copy_(kc)
            self.vc.copy_(vc)

        def _choose(self):
            super()._choose()
            bs = self.beam
            pos = (bs.cur.long() - 2).clamp_(min=0).expand(self.B, 1)
            doc0 = torch.arange(self.B, device=bs.cur.device) // self.W * self.W
            rows = doc0 + bs.anc.gather(1, pos).squeeze(1).long()
            self.kc.copy_(self.kc.index_select(1, rows))
            self.vc.copy_(self.vc.index_select(1, rows))

    def table(t):
        out = model.beam_search(t, z, num_beams=W, length_penalty=1.0)
        return out.ids, model.last_beam_steps

    def copy(t):
        dec = CopyDecoder(eng, z, t, W, 1, -1, length_penalty=1.0)
        out = dec.run()
        return out.ids, dec.steps

    def greedy(t):
        zr = z.repeat_interleave(W, dim=0)
        return model.sample(t, R, z=zr, temperature=0.0, repetition_penalty=1.0), t - 2

    lines, ids = [], {}
    for name, fn in (('table', table), ('copy', copy), ('greedy', greedy)):
        fn(T)                                            # warm-up at the timed shape (code objects, allocator pools)
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            out, steps = fn(T)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) / steps * 1e3)
        ids[name] = out
        lines.append(json.dumps({'form': name, 'docs': B, 'beams': W, 'rows': R, 'max_length': T, 'steps': steps,
                                 'ms_per_step': [round(m, 4) for m in ms],
                                 'median_ms_per_step': round(statistics.median(ms), 4)}))
        print(lines[-1], flush=True)
    NL, H, hd = hp.num_layers, hp.num_heads, hp.d_model // hp.num_heads
    lines.append(json.dumps({'table_equals_copy_ids': bool(torch.equal(ids['table'], ids['copy'])),
                             'cache_bytes_moved_per_step_copy_form': 2 * 2 * NL * R * H * T * hd * 4,
                             'ancestry_bytes_per_step_table_form': 2 * R * T,
                             'device': torch.cuda.get_device_name(0)}))
    print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
