"""python latent_stats.py latents.npz [--seed 0] [--threshold 0.01] [--json out.json]

Does the aggregate posterior q(z) = (1/N) sum_i q(z|x_i) of the latents gathered by gather_latents.py match the
prior N(0, I)? Prints the number of active units (dimensions whose posterior mean varies over the corpus by more than
the threshold, Burda et al. 2016), the mean KL to the prior per dimension, largest first, and the three MMD estimates
of the reference's math_utils.py (analytic Gaussian-RBF against N(0, I), the same against the fitted diagonal Gaussian,
and the seven-scale IMQ), each for one posterior sample per row and for the posterior means. The RBF values are
standardised: MMD^2 over its standard error under the null, of order 1 when the distributions match. Everything runs in
the library's kernels (sparse_vae.LatentIndex.stats / .mmd): a GPU is required.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sparse-vae_amd'))

KINDS = ('rbf', 'rbf_fitted', 'imq')
SOURCES = ('sample', 'mean')


def build_parser():
    ap = argparse.ArgumentParser(description='aggregate-posterior diagnostics of a LatentIndex .npz')
    ap.add_argument('index', help='index .npz written by gather_latents.py')
    ap.add_argument('--seed', type=int, default=0, help='seed of the posterior draws and of the IMQ prior samples')
    ap.add_argument('--threshold', type=float, default=0.01, help='Var[mu_d] above which a dimension is active')
    ap.add_argument('--json', default=None, help='also write the numbers to this file')
    ap.add_argument('--device', default='cuda', help='torch device of the index')
    return ap


def report(index, seed=0, threshold=0.01):
    """All the numbers as plain Python values."""
    st = index.stats(threshold)
    out = {'rows': len(index), 'latent_depth': index.latent_depth, 'seed': seed, 'threshold': threshold,
           'active_units': st['active_units'], 'kl': st['kl'],
           'mean_loc': st['mean_loc'].tolist(), 'var_loc': st['var_loc'].tolist(), 'mean_kl': st['mean_kl'].tolist(),
           'mmd': {}}
    for source in SOURCES:
        for kind in KINDS:
            out['mmd'][f'{kind}/{source}'] = float(index.mmd(kind, source, seed=seed).item())
    return out


def main(argv=None):
    args = build_parser().parse_args(argv)
    from sparse_vae import LatentIndex
    index = LatentIndex.load(args.index, args.device)
    if len(index) < 2:
        raise SystemExit(f'{args.index} holds fewer than two posteriors')
    r = report(index, args.seed, args.threshold)
    print(f"{r['rows']} posteriors of {r['latent_depth']} dimensions")
    print(f"active units (Var[mu_d] > {args.threshold:g}): {r['active_units']} of {r['latent_depth']}")
    print(f"mean KL to the prior: {r['kl']:.6g} nats")
    print('mean KL per dimension, largest first:')
    order = sorted(range(r['latent_depth']), key=lambda d: -r['mean_kl'][d])
    for d in order:
        print(f"  dim {d:3d}  kl {r['mean_kl'][d]:.6g}  var(mu) {r['var_loc'][d]:.6g}  mean(mu) {r['mean_loc'][d]:+.6g}")
    print('MMD^2 to the prior (rbf, rbf_fitted: standardised; imq: raw):')
    for source in SOURCES:
        row = '  '.join(f"{kind} {r['mmd'][f'{kind}/{source}']:.6g}" for kind in KINDS)
        print(f'  posterior {source}s: {row}')
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
