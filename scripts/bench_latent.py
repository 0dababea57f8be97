"""Latent-index search on one MI355X: LatentIndex.search (svae_latent_topk, fused score + select) against what a user
would write without it -- the reference's three torch expressions (knn.py:28-50) on the GPU followed by torch.topk, one
query at a time as knn.py does.

    python scripts/bench_latent.py [--rows 65536 4194304] [--queries 1 8 64] [--reps 20] [--json PATH]

Seeded random posteriors, Z = 64, k = 10. Each search is timed on its own between two HIP events after 3 warm-up
searches; the figure is the median of --reps (>= 20). Both sides run in this one process on the same tensors.
Per case: ms per search; the bytes one pass over the corpus must stream (L2: mu; cosine: mu + inv_norm; KL: mu +
inv_var + logdet) over that time, in TB/s and as a fraction of the 6.29 TB/s measured HBM copy rate; and the ratio
to the torch baseline. A second baseline column ("batched": every query at once as GEMMs over the corpus and one topk
over the [Q, N] matrix, see BatchedTorch) shows what a user who rewrites the expressions gets; it is reported, the
assertion at the end is against the first. Caveats: the searches repeat on a warm cache, so the 65,536-row corpus (16-32 MiB) is served by the
256 MiB Infinity Cache and its figure is launch-bound, not a bandwidth; the 4,194,304-row corpus (1-2 GiB) exceeds that
cache, so every pass comes from HBM. The kernel makes ceil(Q / 8) passes (8 queries per pass), the rate column counts
one."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch.distributions import Normal, kl_divergence  # noqa: E402

HBM_COPY_TBS = 6.29
Z, K = 64, 10
METRICS = ('l2', 'cosine', 'kl')


def posteriors(n, seed, dev):
    g = torch.Generator(device=dev).manual_seed(seed)
    mu = torch.randn(n, Z, generator=g, device=dev)
    lo, hi = torch.log(torch.tensor(0.05)).item(), torch.log(torch.tensor(2.0)).item()
    scale = torch.exp(torch.rand(n, Z, generator=g, device=dev) * (hi - lo) + lo)
    return mu, scale


def stream_bytes(metric, n):
    return {'l2': n * Z * 4, 'cosine': n * (Z * 4 + 4), 'kl': n * (2 * Z * 4 + 4)}[metric]


def torch_search(metric, q_mu, q_scale, mu, scale, corpus):
    """One query at a time: [N, Z] temporaries, then topk."""
    out = []
    for i in range(q_mu.shape[0]):
        if metric == 'l2':
            out.append(((q_mu[i] - mu) ** 2).sum(-1).topk(K, largest=False))
        elif metric == 'cosine':
            out.append(F.cosine_similarity(q_mu[i][None], mu).topk(K, largest=True))
        else:
            q = Normal(q_mu[i], q_scale[i], validate_args=False)
            out.append(kl_divergence(q, corpus).sum(-1).topk(K, largest=False))
    return out


class BatchedTorch:
    """A second, stronger torch baseline: all Q queries at once as GEMMs over the corpus, then one topk over the
    [Q, N] matrix. The corpus-side operands (unit means; 1/var, mu/var, sum mu^2/var, sum log scale) are prepared once,
    outside the timed region, as LatentIndex prepares its rows. The expanded quadratic forms cancel where the
    per-query expressions subtract first, so this column is a speed comparison only."""

    def __init__(self, mu, scale):
        self.mu = mu
        self.unit = F.normalize(mu, dim=-1)
        self.iv = scale.pow(-2)
        self.mu_iv = mu * self.iv
        self.const = (mu * self.mu_iv).sum(-1) + 2.0 * scale.log().sum(-1) - Z

    def search(self, metric, q_mu, q_scale):
        if metric == 'l2':
            return torch.cdist(q_mu, self.mu).pow(2).topk(K, largest=False)
        if metric == 'cosine':
            return (F.normalize(q_mu, dim=-1) @ self.unit.T).topk(K, largest=True)
        quad = (q_scale.pow(2) + q_mu.pow(2)) @ self.iv.T - 2.0 * (q_mu @ self.mu_iv.T) + self.const
        return (0.5 * quad - q_scale.log().sum(-1, keepdim=True)).topk(K, largest=False)


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


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[65536, 4194304])
    ap.add_argument('--queries', type=int, nargs='+', default=[1, 8, 64])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert a.reps >= 20, 'median of at least 20'
    assert torch.cuda.is_available(), 'bench_latent needs a GPU (no CPU fallback)'
    from sparse_vae import LatentIndex
    dev = torch.device('cuda', 0)
    results = []
    print(f'{"metric":7s} {"rows":>8s} {"Q":>3s} {"search ms":>10s} {"TB/s":>7s} {"of copy":>8s} {"torch ms":>10s} '
          f'{"speed-up":>9s} {"same hits":>9s} {"batched ms":>10s} {"vs batched":>10s} {"same hits":>9s}', flush=True)
    for n in a.rows:
        mu, scale = posteriors(n, 1, dev)
        index = LatentIndex(Z).add(mu, scale)
        corpus = Normal(mu, scale, validate_args=False)
        batched = BatchedTorch(mu, scale)
        for nq in a.queries:
            q_mu, q_scale = posteriors(nq, 2, dev)
            for metric in METRICS:
                ours = timed(lambda: index.search((q_mu, q_scale), k=K, metric=metric), a.reps)
                base = timed(lambda: torch_search(metric, q_mu, q_scale, mu, scale, corpus), a.reps)
                _, hits = index.search((q_mu, q_scale), k=K, metric=metric)
                ref = torch.stack([i for _, i in torch_search(metric, q_mu, q_scale, mu, scale, corpus)])
                same = sum(len(set(h.tolist()) & set(r.tolist())) for h, r in zip(hits, ref)) / (nq * K)
                bat = timed(lambda: batched.search(metric, q_mu, q_scale), a.reps)
                bref = batched.search(metric, q_mu, q_scale)[1]
                bsame = sum(len(set(h.tolist()) & set(r.tolist())) for h, r in zip(hits, bref)) / (nq * K)
                tbs = stream_bytes(metric, n) / (ours * 1e-3) / 1e12
                r = {'metric': metric, 'rows': n, 'queries': nq, 'k': K, 'Z': Z, 'search_ms': round(ours, 4),
                     'stream_tb_s': round(tbs, 3), 'fraction_of_copy_rate': round(tbs / HBM_COPY_TBS, 3),
                     'torch_ms': round(base, 4), 'speedup_vs_torch': round(base / ours, 2),
                     'passes': -(-nq // 8), 'hits_shared_with_torch': round(same, 4),
                     'batched_torch_ms': round(bat, 4), 'speedup_vs_batched_torch': round(bat / ours, 2),
                     'hits_shared_with_batched_torch': round(bsame, 4)}
                results.append(r)
                print(f'{metric:7s} {n:8d} {nq:3d} {ours:10.4f} {tbs:7.3f} {tbs / HBM_COPY_TBS:8.3f} {base:10.4f} '
                      f'{base / ours:8.2f}x {same:9.4f} {bat:10.4f} {bat / ours:9.2f}x {bsame:9.4f}', flush=True)
        del index, corpus, batched, mu, scale
        torch.cuda.empty_cache()
    print(json.dumps({'bench': 'latent_search', 'results': results}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
    assert all(r['speedup_vs_torch'] > 1.0 for r in results), 'a fused search at or below the torch baseline is wrong'


if __name__ == '__main__':
    main()
