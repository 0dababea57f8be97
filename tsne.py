"""python tsne.py latents.npz --out tsne.npz [--perplexity P] [--n-iter T] [--max-points M] [--plot tsne.png] [--seed S]
       [--clusters clusters.npz]

A two-dimensional t-SNE of the posterior means gathered by gather_latents.py, the reference's tsne.py:16-36 without
its LDA colouring; --clusters takes the k-means labels of cluster_latents.py in its place (the output gains `labels`
for the embedded rows and --plot colours by them). The neighbour graph, the affinities and every iteration run in
libsvae's kernels (sparse_vae.TSNE): a GPU is required. The repulsion is the exact all-pairs sum, so an iteration costs N^2 pair
evaluations; --max-points embeds a seeded random subset of a larger index. The output .npz holds `embedding`
[M, 2], the subset's `rows` in the index and their `titles`. --plot scatters a random 1,000 of the points
(matplotlib).
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sparse-vae_amd'))


def build_parser():
    ap = argparse.ArgumentParser(description='t-SNE of a LatentIndex .npz')
    ap.add_argument('index', help='index .npz written by gather_latents.py')
    ap.add_argument('--out', required=True, help='output .npz (embedding, rows, titles)')
    ap.add_argument('--perplexity', type=float, default=20.0)
    ap.add_argument('--n-iter', type=int, default=1000)
    ap.add_argument('--max-points', type=int, default=None, help='embed a seeded random subset of this many rows')
    ap.add_argument('--metric', default='l2', choices=('l2', 'kl'))
    ap.add_argument('--plot', default=None, help='also write a scatter plot of 1,000 random points to this image')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--clusters', default=None, help='clusters .npz written by cluster_latents.py: the output gains '
                                                     '`labels` for the embedded rows and --plot colours by them')
    ap.add_argument('--device', default='cuda', help='torch device of the index')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.plot:
        try:
            import matplotlib
        except ImportError:
            raise SystemExit('--plot needs matplotlib, which is not installed; run without --plot and plot the '
                             '`embedding` array of the output file elsewhere')
        matplotlib.use('Agg')
    import numpy as np
    import torch
    from sparse_vae import LatentIndex, TSNE
    index = LatentIndex.load(args.index, args.device)
    n = len(index)
    if n < 3:
        raise SystemExit(f'{args.index} holds {n} posteriors; t-SNE needs at least three')
    labels = None
    if args.clusters:
        with np.load(args.clusters, allow_pickle=False) as z:
            labels = z['labels']
        if labels.shape != (n,):
            raise SystemExit(f'{args.clusters} holds labels of shape {labels.shape}; {args.index} has {n} rows')
    rng = np.random.default_rng(args.seed)
    if args.max_points is not None and args.max_points < n:
        if args.max_points < 3:
            raise SystemExit('--max-points must be at least 3')
        rows = np.sort(rng.choice(n, size=args.max_points, replace=False))
        pick = torch.from_numpy(rows).to(index.device)
        sub = LatentIndex(index.latent_depth, device=index.device)
        sub.add(index.loc[pick], index.scale[pick], [index.titles[i] for i in rows.tolist()])
        index = sub
    else:
        rows = np.arange(n)
    tsne = TSNE(perplexity=args.perplexity, n_iter=args.n_iter, metric=args.metric, seed=args.seed)
    emb = tsne.fit_transform(index).cpu().numpy()
    extra = {} if labels is None else {'labels': labels[rows].astype(np.int64)}
    with open(args.out, 'wb') as f:
        np.savez(f, embedding=emb, rows=rows.astype(np.int64), titles=np.asarray(index.titles, dtype=np.str_), **extra)
    print(f'{len(rows)} of {n} rows embedded -> {args.out}')
    if args.plot:
        import matplotlib.pyplot as plt
        shown = rng.choice(len(rows), size=min(1000, len(rows)), replace=False)
        plt.figure(figsize=(8, 8))
        if labels is None:
            plt.scatter(emb[shown, 0], emb[shown, 1], s=4)
        else:
            plt.scatter(emb[shown, 0], emb[shown, 1], s=4, c=labels[rows][shown], cmap='tab20')
        plt.savefig(args.plot, dpi=150)
        print(f'{len(shown)} points plotted -> {args.plot}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
