"""python cluster_latents.py latents.npz --k 10 --out clusters.npz [--n-init 4] [--max-iter 100] [--seed 0] [--top 10]

k-means of the posterior means gathered by gather_latents.py: what the latent space groups the documents by, from the
latents alone (it stands in for the LDA topic model of the reference's tsne.py:38-63). The seeding and every iteration
run in libsvae's kernels (sparse_vae.KMeans): a GPU is required. The output .npz holds `labels` [N], `centers` [K, Z],
`counts` [K], `inertia` and the index's `titles`; tsne.py --clusters reads it to colour the map. The clusters are
printed largest first, each with the --top titles nearest its centroid among its own members.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sparse-vae_amd'))


def build_parser():
    ap = argparse.ArgumentParser(description='k-means of a LatentIndex .npz')
    ap.add_argument('index', help='index .npz written by gather_latents.py')
    ap.add_argument('--k', type=int, required=True, help='number of clusters')
    ap.add_argument('--out', required=True, help='output .npz (labels, centers, counts, inertia, titles)')
    ap.add_argument('--n-init', type=int, default=4, help='k-means++ starts; the one with the lowest inertia is kept')
    ap.add_argument('--max-iter', type=int, default=100)
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--top', type=int, default=10, help='titles printed per cluster')
    ap.add_argument('--device', default='cuda', help='torch device of the index')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    from sparse_vae import LatentIndex, kernels as K
    index = LatentIndex.load(args.index, args.device)
    n = len(index)
    if not 1 <= args.k <= n:
        raise SystemExit(f'--k must lie in 1..{n} (the rows of {args.index})')
    km = index.kmeans(args.k, n_init=args.n_init, max_iter=args.max_iter, seed=args.seed)
    # one assignment against the final centroids: the members' distances to their own centroid
    label, d2, _, _ = K.kmeans_assign(index.loc.contiguous(), km.cluster_centers_)
    labels, counts = label.cpu().numpy().astype(np.int64), np.bincount(label.cpu().numpy(), minlength=args.k)
    d2 = d2.cpu().numpy()
    with open(args.out, 'wb') as f:
        np.savez(f, labels=labels, centers=km.cluster_centers_.cpu().numpy(), counts=counts.astype(np.int64),
                 inertia=np.float64(km.inertia_), titles=np.asarray(index.titles, dtype=np.str_))
    print(f'{n} rows in {args.k} clusters after {km.n_iter_} iterations, inertia {km.inertia_:.6g} -> {args.out}')
    order = np.lexsort((d2, labels))                 # by cluster, nearest member first
    starts = np.concatenate([[0], np.cumsum(counts)])
    for c in np.argsort(-counts, kind='stable'):
        print(f'cluster {c}: {counts[c]} rows')
        for i in order[starts[c]:starts[c + 1]][:max(args.top, 0)]:
            print(f'  {d2[i]:.4f}  {index.titles[i]}')
    return 0


if __name__ == '__main__':
    sys.exit(main())
