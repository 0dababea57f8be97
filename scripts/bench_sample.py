"""Bulk sampling throughput on one MI355X: the batch-synchronous loop over TransformerVAE.sample against the
streaming sampler TransformerVAE.sample_stream, on the C2 model (6 layers, d 512, 8 heads) with random weights.

    python scripts/bench_sample.py --mode loop|stream [--slots 64,256,1000] [--regimes never,quarter,sixteenth]
                                   [--max-length 512] [--samples-per-slot 8]

For every (slots S, regime) it generates N = samples-per-slot * S samples and prints one JSON line.
* --mode loop: repeated model.sample(T, S) until N samples (what batch_generate_samples does). It uses only API
  older than sample_stream, so the same file measures an older checkout.
* --mode stream: model.sample_stream(T, N, slots=S).
Regimes set the end token's output bias to ln(q V / (1 - q)) so that, on the near-uniform logits of a random-init
model, a sample ends with probability about q per step: never (no end token), quarter (q = 4 / T: mean length
near T / 4), sixteenth (q = 16 / T). The measured mean length is reported.
steps: the stream's own step count; for the loop, (T - 2) per batch when nothing ends, else the longest row of
each batch (the loop polls its live count every 8 steps, so it runs up to 7 more).
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402

END = 2
GEN = dict(temperature=1.0, top_p=0.9, repetition_penalty=1.2)


def lengths(ids):
    """Tokens up to and including the first end token; rows without one count their non-zero width."""
    hit = ids == END
    first = hit.to(torch.uint8).argmax(dim=1) + 1
    return torch.where(hit.any(dim=1), first, (ids != 0).sum(dim=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mode', choices=('loop', 'stream'), required=True)
    ap.add_argument('--slots', default='64,256,1000')
    ap.add_argument('--regimes', default='never,quarter,sixteenth')
    ap.add_argument('--max-length', type=int, default=512)
    ap.add_argument('--samples-per-slot', type=int, default=8)
    ap.add_argument('--tag', default='')
    a = ap.parse_args()
    from sparse_vae import TransformerVAE, TransformerVAEHparams
    dev = torch.device('cuda', 0)
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    hp = TransformerVAEHparams(d_model=512, num_layers=6, num_heads=8, latent_depth=64, sparse_self_attention=False,
                               kl_weight=1.0)
    model = TransformerVAE(hp, device=dev)
    model.initialize_weights()
    model.eval()
    model.start_token = 1
    T = a.max_length
    bias = model._flat.f('output_layer.3.bias')
    bias0 = bias[END].clone()
    for S in (int(s) for s in a.slots.split(',')):
        N = a.samples_per_slot * S
        for regime in a.regimes.split(','):
            q = {'never': 0.0, 'quarter': 4.0 / T, 'sixteenth': 16.0 / T}[regime]
            bias[END] = bias0 + (math.log(q * bias.numel() / (1 - q)) if q else 0.0)
            model.end_token = END if q else -1
            z = torch.randn(N, 1, 64, device=dev)

            def run(n, t):
                if a.mode == 'stream':
                    out = model.sample_stream(t, n, slots=min(S, n), z=z[:n], **GEN)
                    return out, model.last_stream_steps
                outs, steps = [], 0
                for i in range(0, n, S):
                    o = model.sample(t, min(S, n - i), z=z[i:i + S], **GEN)
                    outs.append(o)
                    steps += (t - 2) if not q else int(lengths(o).max().item())
                return torch.cat(outs), steps

            torch.manual_seed(1)
            run(min(N, S), 8)                                   # warm-up (allocations, code objects)
            torch.cuda.synchronize()
            torch.manual_seed(2)
            t0 = time.perf_counter()
            out, steps = run(N, T)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            ln = lengths(out)
            tokens = int(ln.sum().item())
            print(json.dumps({'mode': a.mode, 'tag': a.tag, 'slots': S, 'regime': regime, 'num_samples': N,
                              'max_length': T, 'seconds': round(dt, 3), 'samples_per_s': round(N / dt, 1),
                              'emitted_tokens_per_s': round(tokens / dt, 1), 'steps': steps,
                              'ms_per_step': round(dt / steps * 1e3, 4),
                              'mean_length': round(tokens / N, 2)}), flush=True)
    bias[END] = bias0


if __name__ == '__main__':
    main()
