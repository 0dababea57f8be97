"""python fit_prior.py latents.npz --k 10 --out prior.npz [--source posterior|mean] [--holdout 0.1] [--n-init 1]
                     [--max-iter 100] [--seed 0] [--top 5]

Ex-post density estimation (Ghosh et al. 2020): fit a Gaussian mixture to the aggregate posterior gathered by
gather_latents.py and use it as the prior, for when latent_stats.py shows that the aggregate posterior does not match
N(0, I). EM, the density and the sampler run in libsvae's kernels (sparse_vae.GaussianMixture): a GPU is required.
`sample.py --prior prior.npz` then draws z from the mixture.

The rows are split by a seeded permutation into a fitted part and a held-out part (--holdout, a fraction). Printed:
the components by weight, each with the --top titles of highest responsibility among the fitted rows; the bound per
row (nats per document; with --source mean the log-density of the means) on the fitted and on the held-out rows, and
the same two figures under N(0, I); and the --top least likely held-out documents (outliers; of the fitted rows
without a held-out part). --source posterior (the default) fits the posteriors N(mu, sigma^2), not their means: see
sparse_vae/mixture.py for why.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sparse-vae_amd'))


def build_parser():
    ap = argparse.ArgumentParser(description='Fit a Gaussian-mixture prior to a LatentIndex .npz')
    ap.add_argument('index', help='index .npz written by gather_latents.py')
    ap.add_argument('--k', type=int, required=True, help='number of mixture components')
    ap.add_argument('--out', required=True, help='output .npz (weights, means, variances, settings)')
    ap.add_argument('--source', choices=('posterior', 'mean'), default='posterior',
                    help='fit the posteriors N(mu, sigma^2) (default) or the means as points')
    ap.add_argument('--holdout', type=float, default=0.1, help='fraction of the rows held out of the fit')
    ap.add_argument('--n-init', type=int, default=1, help='k-means starts; the one with the highest bound is kept')
    ap.add_argument('--max-iter', type=int, default=100)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--top', type=int, default=5, help='titles printed per component, and outliers printed')
    ap.add_argument('--device', default='cuda', help='torch device of the index')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch
    from sparse_vae import GaussianMixture, LatentIndex
    index = LatentIndex.load(args.index, args.device)
    n = len(index)
    if not 0 <= args.holdout < 1:
        raise SystemExit('--holdout must lie in [0, 1)')
    n_held = int(n * args.holdout)
    n_fit = n - n_held
    if not 1 <= args.k <= n_fit:
        raise SystemExit(f'--k must lie in 1..{n_fit} (the fitted rows of {args.index})')
    perm = torch.from_numpy(np.random.default_rng(args.seed).permutation(n)).to(index.device)
    loc, var = index.loc, index.scale * index.scale

    def part(rows):
        return loc[rows].contiguous(), (var[rows].contiguous() if args.source == 'posterior' else None)

    fit_rows, held_rows = perm[:n_fit], perm[n_fit:]
    gm = GaussianMixture(args.k, n_init=args.n_init, max_iter=args.max_iter, seed=args.seed).fit(*part(fit_rows))
    gm.save(args.out)
    normal = GaussianMixture.standard_normal(index.latent_depth, index.device)
    state = 'converged' if gm.converged_ else 'not converged'
    print(f'{n_fit} rows, {args.k} components, {gm.n_iter_} iterations ({state}) -> {args.out}')
    what = 'bound' if args.source == 'posterior' else 'log-density'
    print(f'{what} per row, nats:        mixture        N(0, I)')
    print(f'  fitted   ({n_fit:8d})  {gm.score(*part(fit_rows)):13.4f}  {normal.score(*part(fit_rows)):13.4f}')
    if n_held:
        print(f'  held out ({n_held:8d})  {gm.score(*part(held_rows)):13.4f}  {normal.score(*part(held_rows)):13.4f}')
    top = max(args.top, 0)
    resp = gm.predict_proba(*part(fit_rows))
    weights = gm.weights_.cpu().numpy()
    for c in np.argsort(-weights, kind='stable'):
        print(f'component {c}: weight {weights[c]:.4f}')
        best = torch.topk(resp[:, c], min(top, n_fit))
        for r, i in zip(best.values.tolist(), fit_rows[best.indices].tolist()):
            print(f'  {r:.4f}  {index.titles[i]}')
    rows = held_rows if n_held else fit_rows
    score = gm.score_samples(*part(rows))
    worst = torch.topk(-score, min(top, len(rows)))
    print(f'least likely {"held-out " if n_held else ""}documents:')
    for s, i in zip(worst.values.tolist(), rows[worst.indices].tolist()):
        print(f'  {-s:.4f}  {index.titles[i]}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
