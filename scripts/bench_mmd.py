"""The MMD pair sum on one MI355X: svae_pairsum (triangular, the i < j pairs of one set) against the same sum written in
torch in the same process -- row-chunked torch.cdist against the columns from the chunk's first row on, the kernel
function elementwise, the diagonal block masked with triu, every chunk's sum accumulated in f64.

    python scripts/bench_mmd.py [--rows 4096 65536 524288] [--reps 20] [--json PATH]

Seeded N(0, I) rows, Z = 64. RBF: one kernel exp(-d2 / (2 * Z / 8)) (the analytic estimator's third term); IMQ: the
seven scales of gaussian_imq_mmd_sq. Each call is timed on its own between two HIP events after warm-up calls; the
figure is the median of --reps (>= 20) calls, except for the torch side at more than 100,000 rows, which takes seconds
per call and gets 5 calls after one warm-up (lines starting with '#' mark progress). Per case: ms, pairs/s (N (N - 1) / 2
pair evaluations) and the time as lane-operations per pair at one wave64 VALU instruction per 4 clocks per SIMD (what
one wave sustains; the unit of DESIGN section 13's estimate), the torch figure, the ratio,
and the relative difference of the two sums. Nothing is asserted about the ratios: the table reports what was measured,
including any case where torch wins."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402

Z = 64
IMQ_BASE = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)
CHUNK_ELEMS = 2 ** 27          # a [chunk, N] f32 temporary of 512 MiB
PEAK_LANE_OPS = 256 * 4 * 16 * 2.4e9   # CUs x SIMDs x lanes per clock x Hz at one wave64 VALU instruction per 4 clocks


def timed(fn, reps, warmup):
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


def torch_pairsum(x, kind, params):
    n = x.shape[0]
    chunk = max(1, CHUNK_ELEMS // n)
    out = torch.zeros(len(params), dtype=torch.float64, device=x.device)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk)
        d2 = torch.cdist(x[c0:c1], x[c0:]).square_()
        keep = torch.ones(c1 - c0, c1 - c0, dtype=torch.bool, device=x.device).triu_(1)
        for p, a in enumerate(params):
            t = torch.exp(d2 * -a) if kind == 'rbf' else a / (d2 + a)
            t[:, :c1 - c0].mul_(keep)
            out[p] += t.sum(dtype=torch.float64)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, nargs='+', default=[4096, 65536, 524288])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert a.reps >= 20, 'median of at least 20'
    assert torch.cuda.is_available(), 'bench_mmd needs a GPU (no CPU fallback)'
    from sparse_vae import kernels as K
    dev = torch.device('cuda', 0)
    cases = (('rbf', [0.5 / (0.125 * Z)]), ('imq', [b * 2 * Z for b in IMQ_BASE]))
    results = []
    print(f'{"rows":>7s} {"kind":>4s} {"P":>2s} {"pairsum ms":>11s} {"Tpairs/s":>9s} {"ops/pair":>8s} | {"torch ms":>10s} '
          f'{"reps":>4s} | {"x":>7s} {"rel diff":>9s}', flush=True)
    for n in a.rows:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn(n, Z, generator=g, device=dev)
        pairs = n * (n - 1) / 2
        for kind, params in cases:
            out = torch.empty(len(params), dtype=torch.float64, device=dev)
            ms = timed(lambda: K.pairsum(x, kind=kind, params=params, out=out), a.reps, 3)
            t_reps, t_warm = (a.reps, 3) if n <= 100000 else (5, 1)
            print(f'# {n} rows {kind}: kernel {ms:.3f} ms, torch next', flush=True)
            t_ms = timed(lambda: torch_pairsum(x, kind, params), t_reps, t_warm)
            ours, theirs = K.pairsum(x, kind=kind, params=params), torch_pairsum(x, kind, params)
            diff = float(((ours - theirs).abs() / ours.abs()).max().item())
            r = {'rows': n, 'Z': Z, 'kind': kind, 'P': len(params), 'pairsum_ms': round(ms, 4),
                 'pairs_per_s': round(pairs / (ms * 1e-3), 0),
                 'lane_ops_per_pair_at_4clk': round(PEAK_LANE_OPS * ms * 1e-3 / pairs, 1),
                 'torch_ms': round(t_ms, 4), 'torch_reps': t_reps, 'vs_torch': round(t_ms / ms, 2),
                 'rel_diff_vs_torch': diff}
            results.append(r)
            print(f'{n:7d} {kind:>4s} {len(params):2d} {ms:11.4f} {pairs / (ms * 1e-3) / 1e12:9.3f} '
                  f'{r["lane_ops_per_pair_at_4clk"]:8.1f} | {t_ms:10.3f} {t_reps:4d} | {t_ms / ms:6.1f}x {diff:9.2e}',
                  flush=True)
        del x
        torch.cuda.empty_cache()
    print(json.dumps({'bench': 'mmd_pairsum', 'results': results}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
