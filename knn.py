"""python knn.py latents.npz [--query TITLE_OR_ROW ...] [-k 10]

Nearest neighbours of an article among the posterior latents gathered by gather_latents.py, under the three metrics
of the reference's knn.py: squared L2 distance of the means, cosine similarity of the means, and the KL divergence
from the article's posterior to each other one. A query is a title, or a row number when no title matches; without
--query the queries are read from stdin, one per line ('q' quits). The article itself is a legitimate first hit.
Scores and selection run in the latent-index kernels (sparse_vae.LatentIndex.search): a GPU is required.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'sparse-vae_amd'))

TABLES = (('l2', 'Squared L2 distance of the means'), ('cosine', 'Cosine similarity of the means'),
          ('kl', 'KL divergence from the query posterior'))


def build_parser():
    ap = argparse.ArgumentParser(description='k nearest neighbours in a LatentIndex .npz')
    ap.add_argument('index', help='index .npz written by gather_latents.py')
    ap.add_argument('--query', action='append', default=[], help='title or row number (repeatable; default: stdin)')
    ap.add_argument('-k', type=int, default=10, help='hits per table')
    ap.add_argument('--device', default='cuda', help='torch device of the index')
    return ap


def resolve(index, query):
    """Row of a query string: a title first, else a row number; None when neither."""
    row = index.row_of(query)
    if row is None and query.lstrip('-').isdigit() and 0 <= int(query) < len(index):
        row = int(query)
    return row


def tables(index, row, k):
    """The three tables for one row, as lines of text."""
    lines = []
    for metric, heading in TABLES:
        scores, hits = index.search(row, k=k, metric=metric)
        names = [index.titles[i] for i in hits[0].tolist()]
        width = max(len(n) for n in names)
        lines.append('')
        lines.append(heading)
        lines += [f'{n.ljust(width)} - {s}' for n, s in zip(names, scores[0].tolist())]
    lines.append('')
    return lines


def main(argv=None):
    args = build_parser().parse_args(argv)
    from sparse_vae import LatentIndex
    index = LatentIndex.load(args.index, args.device)
    if len(index) == 0:
        raise SystemExit(f'{args.index} holds no posteriors')
    if not 1 <= args.k <= 64:
        raise SystemExit('-k must be in 1..64 (the search kernel keeps at most 64 hits per query)')
    k = min(args.k, len(index))
    if args.query:
        queries = iter(args.query)
    else:
        print('Enter an article title or a row number, one per line; q ends the session.')
        queries = (line.rstrip('\n') for line in sys.stdin)
    for query in queries:
        if not args.query and query == 'q':
            break
        row = resolve(index, query)
        if row is None:
            print(f"'{query}' is neither a title nor a row number of this index.")
            continue
        print('\n'.join(tables(index, row, k)))
    return 0


if __name__ == '__main__':
    sys.exit(main())
