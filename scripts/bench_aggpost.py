"""ELBO surgery on one MI355X: LatentIndex.log_density (joint, and with the per-dimension marginals) and
LatentIndex.elbo_surgery against what a user would write in torch on the same device, in the same process on the same
tensors.

    python scripts/bench_aggpost.py [--sizes 16384x16384 131072x131072 16384x1048576] [--reps 20] [--torch-reps 3]
                                    [--torch-points 16384] [--budget-mib 1024] [--json PATH]

A size is MxN: M points against N rows, Z = 64. The rows are seeded posteriors, half of the dimensions informative
(scale 0.05..0.5) and half collapsed (scale ~ 1); the points are one draw from each of the first M rows.

The torch baseline is the chunked form of marginal_kl's cross_probs (math_utils.py:51-58 of the reference):
Normal(loc, scale).log_prob(z[c0:c1, None]) is a [chunk, N, Z] tensor, .sum(-1).logsumexp(1) the joint density and
.logsumexp(1) the per-dimension one, with the chunk sized so that one such f32 intermediate fills --budget-mib. Its
cost is linear in the number of points (the chunk loop runs over them), so beyond --torch-points points it is timed on
the first --torch-points and the figure is scaled by M / points; the table says which rows are scaled. Each library
figure is the median of --reps (>= 20) runs between two HIP events after 3 warm-ups, each torch figure the median of
--torch-reps after one. The two results are compared on the points both computed and the largest difference is
printed; no speed is asserted: the table says where torch wins."""
import argparse
import json
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402

Z = 64


def index_of(n, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    loc = torch.randn(n, Z, generator=g, device=dev)
    loc[:, 1::2] *= 0.05
    scale = torch.where(torch.arange(Z, device=dev)[None] % 2 == 0,
                        0.05 + 0.45 * torch.rand(n, Z, generator=g, device=dev),
                        0.9 + 0.2 * torch.rand(n, Z, generator=g, device=dev))
    return loc.contiguous(), scale.contiguous()


def torch_logq(z, loc, scale, per_dim, budget_bytes):
    q = torch.distributions.Normal(loc, scale)
    n = loc.shape[0]
    chunk = max(1, budget_bytes // (n * Z * 4))
    outs, outd = [], []
    for c0 in range(0, z.shape[0], chunk):
        lp = q.log_prob(z[c0:c0 + chunk, None])
        outs.append(lp.sum(-1).logsumexp(1) - math.log(n))
        if per_dim:
            outd.append(lp.logsumexp(1) - math.log(n))
    return torch.cat(outs), (torch.cat(outd) if per_dim else None)


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
    ap.add_argument('--sizes', nargs='+', default=['16384x16384', '131072x131072', '16384x1048576'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--torch-reps', type=int, default=3)
    ap.add_argument('--torch-points', type=int, default=16384)
    ap.add_argument('--budget-mib', type=int, default=1024)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert a.reps >= 20, 'median of at least 20'
    assert torch.cuda.is_available(), 'bench_aggpost needs a GPU (no CPU fallback)'
    from sparse_vae import LatentIndex, kernels as K
    dev = torch.device('cuda', 0)
    budget = a.budget_mib << 20
    results = []
    print(f'{"points":>8s} {"rows":>8s} {"joint ms":>9s} {"Gterm/s":>8s} {"torch ms":>10s} {"speed-up":>9s} '
          f'{"per-dim ms":>10s} {"Gterm/s":>8s} {"torch ms":>10s} {"speed-up":>9s} {"surgery ms":>10s} {"torch pts":>9s} '
          f'{"logq diff":>10s} {"dim diff":>10s}', flush=True)
    for size in a.sizes:
        m, n = (int(v) for v in size.lower().split('x'))
        loc, scale = index_of(n, dev)
        index = LatentIndex(Z, device=dev).add(loc, scale)
        z = K.latent_draw(loc[:m].contiguous(), scale[:m].contiguous(), seed=2)
        t_j = timed(lambda: index.log_density(z), a.reps)
        t_d = timed(lambda: index.log_density(z, per_dim=True), a.reps)
        rows = torch.arange(m)
        t_s = timed(lambda: index.elbo_surgery(rows=rows, seed=2), a.reps)
        mt = min(m, a.torch_points)
        zt = z[:mt].contiguous()
        t_tj = timed(lambda: torch_logq(zt, loc, scale, False, budget), a.torch_reps, warmup=1) * (m / mt)
        t_td = timed(lambda: torch_logq(zt, loc, scale, True, budget), a.torch_reps, warmup=1) * (m / mt)
        lq, lqd = index.log_density(zt, per_dim=True)
        tq, tqd = torch_logq(zt, loc, scale, True, budget)
        d_q, d_d = (lq - tq).abs().max().item(), (lqd - tqd).abs().max().item()
        terms = float(m) * n * Z
        r = {'points': m, 'rows': n, 'Z': Z, 'joint_ms': round(t_j, 3), 'joint_gterms_per_s': round(terms / t_j / 1e6, 1),
             'torch_joint_ms': round(t_tj, 3), 'joint_speedup_vs_torch': round(t_tj / t_j, 2),
             'per_dim_ms': round(t_d, 3), 'per_dim_gterms_per_s': round(terms / t_d / 1e6, 1),
             'torch_per_dim_ms': round(t_td, 3), 'per_dim_speedup_vs_torch': round(t_td / t_d, 2),
             'surgery_ms': round(t_s, 3), 'torch_points': mt, 'torch_scaled': mt < m, 'logq_diff': d_q,
             'logq_dim_diff': d_d}
        results.append(r)
        print(f'{m:8d} {n:8d} {t_j:9.3f} {terms / t_j / 1e6:8.1f} {t_tj:10.3f} {t_tj / t_j:8.2f}x {t_d:10.3f} '
              f'{terms / t_d / 1e6:8.1f} {t_td:10.3f} {t_td / t_d:8.2f}x {t_s:10.3f} {mt:9d} {d_q:10.3e} {d_d:10.3e}',
              flush=True)
        del index, loc, scale, z, zt, lq, lqd, tq, tqd
        torch.cuda.empty_cache()
    print(json.dumps({'bench': 'aggpost', 'results': results}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
