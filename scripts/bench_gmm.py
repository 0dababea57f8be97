"""The Gaussian-mixture prior on one MI355X: one EM iteration (svae_gmm_estep + svae_gmm_mstep) and a 1M-row draw
(svae_gmm_sample) against what a user would write in torch on the same device, in the same process on the same tensors.

    python scripts/bench_gmm.py [--rows 65536 1048576] [--k 10 100] [--reps 20] [--sample-rows 1048576] [--json PATH]

Z = 64. The rows are seeded posteriors (means around K centres, variances in 0.1 .. 0.4); the model of the timed
iteration is a hard M-step from the true blob labels. The torch iteration is the same EM step in the expanded quadratic
form: a_ik = logc_k - 1/2 [(x^2 + s2) @ (1/v)^T - 2 x @ (m/v)^T + sum m^2/v] by matmul (on the matrix cores),
torch.logsumexp, r = exp(a - lse), then r.T @ x and r.T @ (x^2 + s2) for the means and variances, all in f32 (its sums
are not about the component mean, so its variances cancel where ours do not). The torch draw is torch.multinomial of
the weights plus randn. Each figure is the median of --reps (>= 20) runs between two HIP events after 3 warm-ups. The
two iterations' bound per row and parameters are compared and printed; no speed is asserted: the table says where torch
wins.

A second table times the E-step alone at the wider latent depths (--corner-rows rows, K = 10), with and without
variances: with variances above Z = 128 a lane cannot hold both of its rows in registers, the kernel loads them in
four segments per component tile and that instance spills; the table says what the corner costs."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import torch  # noqa: E402

Z = 64
REG = 1e-6


def rows_of(n, k, dev, Z=Z):
    g = torch.Generator(device=dev).manual_seed(1)
    centres = 0.8 * torch.randn(k, Z, generator=g, device=dev)
    which = torch.randint(0, k, (n,), generator=g, device=dev)
    s2 = 0.1 + 0.3 * torch.rand(n, Z, generator=g, device=dev)
    x = centres[which] + (1 - s2).sqrt() * torch.randn(n, Z, generator=g, device=dev)
    return x.contiguous(), s2.contiguous(), which.to(torch.int32)


def torch_iteration(x, s2, w, m, v):
    iv = 1.0 / v
    logc = w.log() - 0.5 * (6.283185307179586 * v).log().sum(1)
    e = x * x + s2
    a = logc[None] - 0.5 * (e @ iv.T - 2.0 * (x @ (m * iv).T) + (m * m * iv).sum(1)[None])
    lse = torch.logsumexp(a, dim=1)
    r = (a - lse[:, None]).exp()
    nk = r.sum(0)
    mean = (r.T @ x) / nk[:, None]
    var = (r.T @ e) / nk[:, None] - mean * mean + REG
    return nk / nk.sum(), mean, var, lse.double().mean()


def torch_sample(w, m, v, n):
    comp = torch.multinomial(w, n, replacement=True)
    return m[comp] + v[comp].sqrt() * torch.randn(n, m.shape[1], device=m.device), comp


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
    ap.add_argument('--rows', type=int, nargs='+', default=[65536, 1048576])
    ap.add_argument('--k', type=int, nargs='+', default=[10, 100])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--sample-rows', type=int, default=1 << 20)
    ap.add_argument('--corner-rows', type=int, default=262144)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert a.reps >= 20, 'median of at least 20'
    assert torch.cuda.is_available(), 'bench_gmm needs a GPU (no CPU fallback)'
    from sparse_vae import kernels as K
    dev = torch.device('cuda', 0)
    results = []
    print(f'{"rows":>8s} {"K":>4s} {"estep ms":>9s} {"TFLOP/s":>8s} {"mstep ms":>9s} {"iter ms":>9s} {"torch ms":>9s} '
          f'{"speed-up":>9s} {"bound diff":>11s} {"mean diff":>10s} {"var diff":>10s} {"sample ms":>10s} '
          f'{"torch ms":>9s} {"speed-up":>9s}', flush=True)
    for n in a.rows:
        for k in a.k:
            x, s2, which = rows_of(n, k, dev)
            start = K.gmm_pack(torch.full((k,), 1.0 / k, device=dev), torch.zeros(k, Z, device=dev),
                               torch.ones(k, Z, device=dev))
            K.gmm_mstep(x, s2, start, k, label=which, reg_covar=REG)
            w, m, v = (K.gmm_view(start, k, Z, s).clone() for s in ('weight', 'mean', 'var'))
            work = start.clone()
            lse = torch.empty(n, dtype=torch.float32, device=dev)
            bound = torch.empty(1, dtype=torch.float64, device=dev)
            nk = torch.empty(k, dtype=torch.float64, device=dev)

            def estep():
                K.gmm_estep(x, s2, start, k, lse=lse, bound=bound, want_label=False)

            def mstep():
                work.copy_(start)
                K.gmm_mstep(x, s2, work, k, lse=lse, reg_covar=REG, nk=nk)

            def iteration():
                estep()
                mstep()

            t_e, t_m, t_iter = timed(estep, a.reps), timed(mstep, a.reps), timed(iteration, a.reps)
            t_torch = timed(lambda: torch_iteration(x, s2, w, m, v), a.reps)
            tw, tm, tv, tb = torch_iteration(x, s2, w, m, v)
            d_bound = abs(bound.item() / n - tb.item())
            d_mean = (K.gmm_view(work, k, Z, 'mean') - tm).abs().max().item()
            d_var = (K.gmm_view(work, k, Z, 'var') - tv).abs().max().item()
            ns = a.sample_rows
            t_s = timed(lambda: K.gmm_sample(work, k, Z, ns, seed=3), a.reps)
            t_ts = timed(lambda: torch_sample(tw, tm, tv, ns), a.reps)
            tflops = 5.0 * n * k * Z / (t_e * 1e-3) / 1e12            # sub, fma, fma per element
            r = {'rows': n, 'K': k, 'Z': Z, 'estep_ms': round(t_e, 4), 'estep_tflops': round(tflops, 2),
                 'mstep_ms': round(t_m, 4), 'iteration_ms': round(t_iter, 4), 'torch_iteration_ms': round(t_torch, 4),
                 'speedup_vs_torch': round(t_torch / t_iter, 2), 'bound_diff': d_bound, 'mean_diff': d_mean,
                 'var_diff': d_var, 'sample_rows': ns, 'sample_ms': round(t_s, 4), 'torch_sample_ms': round(t_ts, 4),
                 'sample_speedup_vs_torch': round(t_ts / t_s, 2)}
            results.append(r)
            print(f'{n:8d} {k:4d} {t_e:9.4f} {tflops:8.2f} {t_m:9.4f} {t_iter:9.4f} {t_torch:9.4f} '
                  f'{t_torch / t_iter:8.2f}x {d_bound:11.3e} {d_mean:10.3e} {d_var:10.3e} {t_s:10.4f} {t_ts:9.4f} '
                  f'{t_ts / t_s:8.2f}x', flush=True)
            del x, s2, lse, work
            torch.cuda.empty_cache()
    corner = []
    print(f'{"rows":>8s} {"K":>4s} {"Z":>4s} {"variances":>9s} {"segments":>8s} {"estep ms":>9s} {"TFLOP/s":>8s}', flush=True)
    for z in (64, 128, 256):
        n, k = a.corner_rows, 10
        x, s2, which = rows_of(n, k, dev, z)
        model = K.gmm_pack(torch.full((k,), 1.0 / k, device=dev), torch.zeros(k, z, device=dev),
                           torch.ones(k, z, device=dev))
        K.gmm_mstep(x, s2, model, k, label=which, reg_covar=REG)
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        bound = torch.empty(1, dtype=torch.float64, device=dev)
        for var in (None, s2):
            t = timed(lambda: K.gmm_estep(x, var, model, k, lse=lse, bound=bound, want_label=False), a.reps)
            segs = K.gmm_geometry(n, k, z, var is not None)[5]
            tf = 5.0 * n * k * z / (t * 1e-3) / 1e12
            corner.append({'rows': n, 'K': k, 'Z': z, 'variances': var is not None, 'segments': segs,
                           'estep_ms': round(t, 4), 'estep_tflops': round(tf, 2)})
            print(f'{n:8d} {k:4d} {z:4d} {str(var is not None):>9s} {segs:8d} {t:9.4f} {tf:8.2f}', flush=True)
        del x, s2, lse
        torch.cuda.empty_cache()
    print(json.dumps({'bench': 'gmm', 'results': results, 'estep_by_depth': corner}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)


if __name__ == '__main__':
    main()
