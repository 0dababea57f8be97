"""t-SNE iterations on one MI355X: the svae_tsne_* kernels (exact all-pairs repulsion, attraction over the k-NN edges,
optimiser step) against the same iteration written in torch in the same process -- a row-chunked broadcast expression
for the repulsion, index_add_ for the attraction, elementwise torch for the update.

    python scripts/bench_tsne.py [--rows 4096 65536 524288] [--reps 20] [--json PATH]

Seeded Gaussian blobs, Z = 64, perplexity 20 (60 neighbours). Each call is timed on its own between two HIP events
after 3 warm-up calls; the figure is the median of --reps (>= 20), on both sides at every size (the torch side takes
about 11 s per call at 524,288 rows, so that size runs for some eight minutes; lines starting with '#' mark its
progress). Per case: ms and pairs/s (N^2 pair evaluations) of tsne_repulse, ms and edges/s (2 N k directed edge
visits) of tsne_attract, ms of a full iteration (repulse + attract + update), the torch figures and the ratios. The
k-NN self-join (LatentIndex.knn_graph, N / 8 corpus passes of svae_latent_topk) is timed once per size by the host
clock. Nothing is asserted about the ratios: the table reports what was measured, including any case where torch
wins."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402

Z, PERPLEXITY, K_NBR, BLOBS = 64, 20.0, 60, 10


def blobs(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    centres = torch.randn(BLOBS, Z, generator=g, device=dev) * 18.0 ** 0.5
    return centres[torch.arange(n, device=dev) % BLOBS] + torch.randn(n, Z, generator=g, device=dev)


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


class TorchIteration:
    """The same iteration as torch expressions. The repulsion goes in chunks of rows sized so that a [chunk, N]
    temporary holds 2^25 elements (128 MiB of f32)."""

    def __init__(self, nbr, p):
        n, k = nbr.shape
        self.n, self.chunk = n, max(1, 2 ** 25 // n)
        self.src = torch.arange(n, device=nbr.device).repeat_interleave(k)
        self.dst = nbr.reshape(-1).to(torch.int64)
        self.w = p.reshape(-1)

    def repulse(self, y):
        n = self.n
        rep, zrow = torch.empty_like(y), torch.empty(n, device=y.device)
        for c0 in range(0, n, self.chunk):
            c1 = min(n, c0 + self.chunk)
            d = y[c0:c1, None, :] - y[None, :, :]
            q = 1.0 / (1.0 + (d * d).sum(-1))
            r = torch.arange(c1 - c0, device=y.device)
            q[r, r + c0] = 0.0
            zrow[c0:c1] = q.sum(1)
            rep[c0:c1] = ((q * q)[:, :, None] * d).sum(1)
        return rep, zrow.sum()

    def attract(self, y):
        d = y[self.src] - y[self.dst]
        f = (self.w / (1.0 + (d * d).sum(-1)))[:, None] * d
        return torch.zeros_like(y).index_add_(0, self.src, f).index_add_(0, self.dst, -f)

    def step(self, y, vel, gains, ex, lr, mom):
        rep, zsum = self.repulse(y)
        g = 4.0 * (ex / (2.0 * self.n) * self.attract(y) - rep / zsum)
        gains.copy_(torch.where(vel * g < 0, gains + 0.2, gains * 0.8).clamp_min_(0.01))
        vel.mul_(mom).sub_(lr * gains * g)
        y.add_(vel)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[4096, 65536, 524288])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert a.reps >= 20, 'median of at least 20'
    assert torch.cuda.is_available(), 'bench_tsne needs a GPU (no CPU fallback)'
    from sparse_vae import LatentIndex, kernels as K
    from sparse_vae.tsne import reverse_edges
    dev = torch.device('cuda', 0)
    results = []
    print(f'{"rows":>7s} {"knn s":>7s} {"repulse ms":>10s} {"Tpairs/s":>8s} {"attract ms":>10s} {"Gedges/s":>8s} '
          f'{"iter ms":>9s} | {"torch rep":>10s} {"torch att":>10s} {"torch iter":>10s} {"reps":>4s} | '
          f'{"rep x":>7s} {"att x":>7s} {"iter x":>7s}', flush=True)
    for n in a.rows:
        x = blobs(n, 1, dev)
        index = LatentIndex(Z).add(x, torch.ones_like(x))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        dist, nbr = index.knn_graph(K_NBR)
        torch.cuda.synchronize()
        knn_s = time.perf_counter() - t0
        del index, x
        p, _ = K.tsne_affinities(dist, PERPLEXITY)
        rev_ptr, rev_edge = reverse_edges(nbr)
        g = torch.Generator(device=dev).manual_seed(2)
        y0 = torch.randn(n, 2, generator=g, device=dev) * 10.0      # the spread of a mid-run embedding
        y, vel, gains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        rep, attr = torch.empty_like(y), torch.empty_like(y)
        zrow, zsum = torch.empty(n, device=dev), torch.empty(1, device=dev)
        lr = max(n / 12.0 / 4.0, 50.0)

        def ours_step():
            K.tsne_repulse(y, rep, zrow, zsum)
            K.tsne_attract(y, nbr, p, rev_ptr, rev_edge, attr)
            K.tsne_update(y, vel, gains, attr, rep, zsum, 1.0, lr, 0.8)

        rep_ms = timed(lambda: K.tsne_repulse(y, rep, zrow, zsum), a.reps)
        att_ms = timed(lambda: K.tsne_attract(y, nbr, p, rev_ptr, rev_edge, attr), a.reps)
        it_ms = timed(ours_step, a.reps)
        base = TorchIteration(nbr, p)
        ty, tvel, tgains = y0.clone(), torch.zeros_like(y0), torch.ones_like(y0)
        t_reps = a.reps
        print(f'# {n} rows: kernels timed, torch repulsion next', flush=True)
        trep_ms = timed(lambda: base.repulse(ty), t_reps)
        tatt_ms = timed(lambda: base.attract(ty), t_reps)
        print(f'# {n} rows: torch repulsion {trep_ms:.3f} ms, torch iteration next', flush=True)
        tit_ms = timed(lambda: base.step(ty, tvel, tgains, 1.0, lr, 0.8), t_reps)
        agree = (None, None)
        if n <= 65536:   # the two sides agree on one iteration's forces (a sanity check of the baseline, not a test)
            r_t, z_t = base.repulse(y0)
            r_o, _, z_o = K.tsne_repulse(y0)
            agree = (float(((r_o - r_t).abs().max() / r_t.abs().max()).item()),
                     float(((z_o - z_t).abs() / z_t).item()))
        r = {'rows': n, 'k': K_NBR, 'knn_graph_s': round(knn_s, 3), 'repulse_ms': round(rep_ms, 4),
             'pairs_per_s': round(n * n / (rep_ms * 1e-3), 0), 'attract_ms': round(att_ms, 4),
             'edges_per_s': round(2 * n * K_NBR / (att_ms * 1e-3), 0), 'iteration_ms': round(it_ms, 4),
             'torch_repulse_ms': round(trep_ms, 4), 'torch_attract_ms': round(tatt_ms, 4),
             'torch_iteration_ms': round(tit_ms, 4), 'torch_reps': t_reps,
             'repulse_vs_torch': round(trep_ms / rep_ms, 2), 'attract_vs_torch': round(tatt_ms / att_ms, 2),
             'iteration_vs_torch': round(tit_ms / it_ms, 2), 'repulse_rel_diff_vs_torch': agree[0],
             'zsum_rel_diff_vs_torch': agree[1]}
        results.append(r)
        print(f'{n:7d} {knn_s:7.2f} {rep_ms:10.4f} {n * n / (rep_ms * 1e-3) / 1e12:8.3f} {att_ms:10.4f} '
              f'{2 * n * K_NBR / (att_ms * 1e-3) / 1e9:8.2f} {it_ms:9.4f} | {trep_ms:10.3f} {tatt_ms:10.3f} '
              f'{tit_ms:10.3f} {t_reps:4d} | {trep_ms / rep_ms:6.1f}x {tatt_ms / att_ms:6.2f}x {tit_ms / it_ms:6.1f}x',
              flush=True)
        del base, dist, nbr, p, rev_ptr, rev_edge
        torch.cuda.empty_cache()
    print(json.dumps({'bench': 'tsne_iteration', 'results': results}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
