"""k-means on one MI355X: one Lloyd iteration (svae_kmeans_assign + svae_kmeans_update) and one k-means++ seeding
(svae_kmeans_seed) against what a user would write in torch on the same device, in the same process on the same
tensors.

    python scripts/bench_kmeans.py [--rows 65536 1048576] [--k 10 100 1000] [--reps 20] [--json PATH]

Z = 64. The rows are seeded unit Gaussians around K centres; the centroids of the timed iteration are a k-means++
seeding of them. The torch iteration is chunked torch.cdist + argmin, then index_add_ and bincount for the means (the
cdist of more than 25 rows runs as a GEMM on the matrix cores; index_add_ adds with atomics, so its sums are not
reproducible run to run). The torch seeding is the same D^2 sampling with the same uniforms: per step a broadcast
difference, a running minimum, an f64 cumsum and a searchsorted, nothing read back. Each figure is the median of
--reps (>= 20) runs between two HIP events after 3 warm-ups. Labels are compared with torch's on every row whose two
smallest torch distances differ by more than 1e-3 relative (closer than that the expanded f32 form of cdist cannot tell
them apart); they must all agree. No speed is asserted: the table says where torch wins."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402

Z = 64
TIE = 1e-3


def rows_of(n, k, dev):
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 3.0 * torch.randn(k, Z, generator=g, device=dev)
    which = torch.randint(0, k, (n,), generator=g, device=dev)
    return (centres[which] + torch.randn(n, Z, generator=g, device=dev)).contiguous()


def chunk_rows(n, k):
    return max(1024, min(n, (1 << 26) // k))


def torch_assign(x, cent):
    n = x.shape[0]
    labels = torch.empty(n, dtype=torch.int64, device=x.device)
    step = chunk_rows(n, cent.shape[0])
    for i in range(0, n, step):
        labels[i:i + step] = torch.cdist(x[i:i + step], cent).argmin(1)
    return labels


def torch_iteration(x, cent):
    labels = torch_assign(x, cent)
    sums = torch.zeros_like(cent).index_add_(0, labels, x)
    count = torch.bincount(labels, minlength=cent.shape[0])
    return torch.where(count[:, None] > 0, sums / count[:, None].clamp(min=1), cent), labels


def torch_seed(x, k, u):
    n = x.shape[0]
    rows = torch.empty(k, dtype=torch.int64, device=x.device)
    rows[0] = (u[0].double() * n).floor().long().clamp(max=n - 1)
    mind = None
    for s in range(1, k):
        d = (x - x[rows[s - 1]]).pow(2).sum(-1)
        mind = d if mind is None else torch.minimum(mind, d)
        cum = torch.cumsum(mind.double(), 0)
        rows[s] = torch.searchsorted(cum, u[s].double() * cum[-1], right=True).clamp(max=n - 1)
    return rows


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


def label_agreement(x, cent, ours):
    """(share of the rows compared, share of those on which the labels agree)."""
    n, k = x.shape[0], cent.shape[0]
    if k == 1:
        return 1.0, float((ours == 0).double().mean())
    step = chunk_rows(n, k)
    compared = agree = 0
    for i in range(0, n, step):
        two, idx = torch.cdist(x[i:i + step], cent).topk(2, dim=1, largest=False)
        clear = (two[:, 1] - two[:, 0]) > TIE * two[:, 1]
        compared += int(clear.sum())
        agree += int((clear & (idx[:, 0] == ours[i:i + step])).sum())
    return compared / n, agree / max(compared, 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[65536, 1048576])
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100, 1000])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert a.reps >= 20, 'median of at least 20'
    assert torch.cuda.is_available(), 'bench_kmeans needs a GPU (no CPU fallback)'
    from sparse_vae import kernels as K
    dev = torch.device('cuda', 0)
    results = []
    print(f'{"rows":>8s} {"K":>5s} {"assign ms":>10s} {"TFLOP/s":>8s} {"update ms":>10s} {"iter ms":>9s} {"torch ms":>9s} '
          f'{"speed-up":>9s} {"compared":>9s} {"agree":>7s} {"seed ms":>9s} {"torch ms":>9s} {"speed-up":>9s} '
          f'{"same rows":>9s}', flush=True)
    for n in a.rows:
        for k in a.k:
            x = rows_of(n, k, dev)
            u = torch.rand(k, generator=torch.Generator(device=dev).manual_seed(2), device=dev)
            seed_rows, cent = K.kmeans_seed(x, k, u=u)
            label = torch.full((n,), -1, dtype=torch.int32, device=dev)
            changed = torch.empty(1, dtype=torch.int32, device=dev)
            inertia = torch.empty(1, dtype=torch.float64, device=dev)
            count = torch.empty(k, dtype=torch.int32, device=dev)
            work = cent.clone()

            def assign():
                K.kmeans_assign(x, cent, label, None, changed, inertia, want_d2=False)

            def update():
                work.copy_(cent)
                K.kmeans_update(x, label, work, count)

            def iteration():
                assign()
                update()

            t_assign, t_update, t_iter = timed(assign, a.reps), timed(update, a.reps), timed(iteration, a.reps)
            t_torch = timed(lambda: torch_iteration(x, cent), a.reps)
            compared, agree = label_agreement(x, cent, label.long())
            t_seed = timed(lambda: K.kmeans_seed(x, k, u=u), a.reps)
            t_tseed = timed(lambda: torch_seed(x, k, u), a.reps)
            same_rows = float((torch_seed(x, k, u) == seed_rows.long()).double().mean())
            tflops = 3.0 * n * k * Z / (t_assign * 1e-3) / 1e12
            r = {'rows': n, 'K': k, 'Z': Z, 'assign_ms': round(t_assign, 4), 'assign_tflops': round(tflops, 2),
                 'update_ms': round(t_update, 4), 'iteration_ms': round(t_iter, 4), 'torch_iteration_ms': round(t_torch, 4),
                 'speedup_vs_torch': round(t_torch / t_iter, 2), 'rows_compared': round(compared, 4),
                 'labels_agree': agree, 'seed_ms': round(t_seed, 4),
                 'torch_seed_ms': round(t_tseed, 4), 'seed_speedup_vs_torch': round(t_tseed / t_seed, 2),
                 'seed_rows_shared_with_torch': round(same_rows, 4)}
            results.append(r)
            print(f'{n:8d} {k:5d} {t_assign:10.4f} {tflops:8.2f} {t_update:10.4f} {t_iter:9.4f} {t_torch:9.4f} '
                  f'{t_torch / t_iter:8.2f}x {compared:9.4f} {agree:7.4f} {t_seed:9.3f} {t_tseed:9.3f} '
                  f'{t_tseed / t_seed:8.2f}x {same_rows:9.4f}', flush=True)
            del x, label, work
            torch.cuda.empty_cache()
    print(json.dumps({'bench': 'kmeans', 'results': results}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
    assert all(r['labels_agree'] == 1.0 for r in results), 'a label differs from torch where torch sees no tie'


if __name__ == '__main__':
    main()
