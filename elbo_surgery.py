"""python elbo_surgery.py latents.npz [--samples M] [--seed 0] [--leave-one-out] [--json out.json] [--device cuda]

How much of the KL term of a trained model is information about the document, and how much is mismatch with the prior?
Over the latents gathered by gather_latents.py the mean KL splits as

    E_x KL(q(z|x) || p(z)) = I_q(x; z) + KL(q(z) || p(z)),        KL(q(z) || p(z)) = TC + sum_d KL(q(z_d) || p(z_d))

(Hoffman & Johnson 2016; Chen et al. 2018) with q(z) = (1/N) sum_i q(z|x_i) the aggregate posterior, taken here as the
exact N-component mixture over the whole index, not inside one batch as the training log's *_mc_mutual_info is (that
one cannot exceed log B). Prints the analytic mean KL against its Monte-Carlo estimate, the three terms with the mutual
information beside its cap log N, and the per-dimension KL of the marginals, largest first, beside the analytic mean KL
per dimension. --samples draws from a seeded subset of the rows (the density is still taken against all of them);
--leave-one-out also prints the estimate with each point's own posterior left out: the inclusive estimate understates
the mutual information and the leave-one-out estimate overstates it, so the two bracket it. Everything runs in the
library's kernels (sparse_vae.LatentIndex.elbo_surgery): a GPU is required.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sparse-vae_amd'))


def build_parser():
    ap = argparse.ArgumentParser(description='ELBO surgery of a LatentIndex .npz')
    ap.add_argument('index', help='index .npz written by gather_latents.py')
    ap.add_argument('--samples', type=int, default=None, help='rows to draw from (default: all of them)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the row subset and of the posterior draws')
    ap.add_argument('--leave-one-out', action='store_true', help="also estimate with each point's own row left out")
    ap.add_argument('--json', default=None, help='also write the numbers to this file')
    ap.add_argument('--device', default='cuda', help='torch device of the index')
    return ap


def report(index, samples=None, seed=0, leave_one_out=False):
    """All the numbers as plain Python values."""
    out = {'rows': len(index), 'latent_depth': index.latent_depth,
           'mean_kl': index.stats()['mean_kl'].tolist(),
           'inclusive': index.elbo_surgery(samples=samples, seed=seed).to_dict()}
    if leave_one_out:
        out['leave_one_out'] = index.elbo_surgery(samples=samples, seed=seed, leave_one_out=True).to_dict()
    return out


def print_terms(name, s):
    print(f'{name} estimate of q(z):')
    print(f"  mutual information I_q(x; z): {s['mutual_info']:.6g} nats (cap {s['mi_cap']:.6g})")
    if s['saturated']:
        print('  the estimate is saturated (within 1 % of its cap): it reports the size of the index, not the model; '
              'more rows are needed')
    print(f"  marginal KL(q(z) || p(z)):    {s['marginal_kl']:.6g} nats")
    print(f"  total correlation:            {s['total_correlation']:.6g} nats")
    print(f"  sum of per-dimension KLs:     {sum(s['dim_kl']):.6g} nats")


def main(argv=None):
    args = build_parser().parse_args(argv)
    from sparse_vae import LatentIndex
    index = LatentIndex.load(args.index, args.device)
    if len(index) < 2:
        raise SystemExit(f'{args.index} holds fewer than two posteriors')
    r = report(index, args.samples, args.seed, args.leave_one_out)
    inc = r['inclusive']
    print(f"{r['rows']} posteriors of {r['latent_depth']} dimensions, {inc['samples']} samples (seed {inc['seed']})")
    print(f"mean KL to the prior: analytic {inc['kl_analytic']:.6g} nats, Monte Carlo {inc['kl_mc']:.6g} nats")
    print_terms('inclusive', inc)
    if args.leave_one_out:
        print_terms('leave-one-out', r['leave_one_out'])
    print('KL(q(z_d) || p(z_d)) per dimension, largest first (beside the mean KL(q(z_d|x) || p(z_d)) of all rows):')
    order = sorted(range(r['latent_depth']), key=lambda d: -inc['dim_kl'][d])
    for d in order:
        print(f"  dim {d:3d}  marginal kl {inc['dim_kl'][d]:.6g}  mean kl {r['mean_kl'][d]:.6g}")
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(r, f, indent=1)


if __name__ == '__main__':
    main()
