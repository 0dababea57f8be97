"""Exact t-SNE of the posterior latents in two dimensions: what the reference's tsne.py:16-30 gets from tsnecuda (CUDA
only) or, without it, from sklearn.manifold.TSNE on the CPU.

The neighbour graph is LatentIndex.knn_graph (svae_latent_topk); the input affinities, the exact all-pairs repulsion,
the attraction over the graph's edges and the optimiser step are libsvae's svae_tsne_* kernels (csrc/tsne.hip). The
optimiser is van der Maaten's as sklearn implements it: early exaggeration, momentum 0.5 -> 0.8, per-coordinate gains.
There is no CPU fallback."""
import torch

from . import kernels as K
from .latent_index import LatentIndex, _rows

_NO_CPU = ('TSNE runs on the MI355X HIP kernels (svae_tsne_*, svae_latent_topk): give it a LatentIndex or a tensor on '
           'a GPU. There is no CPU fallback.')


def reverse_edges(nbr):
    """The k-NN graph's edges grouped by their target: nbr int [N, k] -> (rev_ptr int32 [N + 1], rev_edge int32
    [N * k]). rev_edge[rev_ptr[i]:rev_ptr[i + 1]] are the flat ids e = j * k + s of the edges with nbr[j][s] == i, in
    ascending order. Index work only (sort, bincount, cumsum), on the tensor's device, CPU included."""
    if nbr.dim() != 2:
        raise ValueError(f'reverse_edges: expected [N, k], got {tuple(nbr.shape)}')
    n = nbr.shape[0]
    target = nbr.reshape(-1).to(torch.int64)
    _, order = torch.sort(target, stable=True)
    counts = torch.bincount(target, minlength=n)
    rev_ptr = torch.zeros(n + 1, dtype=torch.int64, device=nbr.device)
    rev_ptr[1:] = torch.cumsum(counts, 0)
    return rev_ptr.to(torch.int32), order.to(torch.int32)


class TSNE:
    def __init__(self, perplexity=20.0, n_neighbors=None, n_iter=1000, early_exaggeration=12.0, exaggeration_iter=250,
                 learning_rate='auto', metric='l2', seed=0):
        if metric not in ('l2', 'kl'):
            raise ValueError(f"metric must be 'l2' or 'kl', got '{metric}'")
        if n_neighbors is not None and not 1.0 < perplexity < n_neighbors:
            raise ValueError(f'perplexity {perplexity} must lie in (1, n_neighbors = {n_neighbors})')
        if n_neighbors is not None and n_neighbors > 63:
            raise ValueError('n_neighbors is at most 63 (LatentIndex.knn_graph)')
        if not perplexity > 1.0:
            raise ValueError(f'perplexity {perplexity} must exceed 1')
        self.perplexity, self.n_neighbors = float(perplexity), n_neighbors
        self.n_iter, self.exaggeration_iter = int(n_iter), int(exaggeration_iter)
        self.early_exaggeration = float(early_exaggeration)
        self.learning_rate, self.metric, self.seed = learning_rate, metric, int(seed)
        self.embedding_ = self.knn_ = self.beta_ = None

    def _neighbors(self, n):
        k = self.n_neighbors
        if k is None:
            k = int(min(63, 3 * self.perplexity, n - 1))
        if not 1.0 < self.perplexity < k:
            raise ValueError(f'perplexity {self.perplexity} must lie in (1, n_neighbors = {k}) ({n} rows)')
        return k

    def fit_transform(self, x, init=None):
        """x: a LatentIndex, or f32 [N, Z] / [N, 1, Z] device tensor of means -> the embedding f32 [N, 2] (also kept
        as embedding_, with knn_ = (dist, idx) and beta_)."""
        if isinstance(x, LatentIndex):
            index = x
            if index.device is None or index.device.type != 'cuda':
                raise RuntimeError(_NO_CPU)
        else:
            if not torch.is_tensor(x):
                raise TypeError('TSNE.fit_transform takes a LatentIndex or a tensor')
            if not x.is_cuda:
                raise RuntimeError(_NO_CPU)
            if x.dim() == 3 and x.shape[1] == 1:
                x = x[:, 0]
            if x.dim() != 2:
                raise ValueError(f'expected [N, Z] or [N, 1, Z], got {tuple(x.shape)}')
            loc = _rows(x, x.shape[-1], 'x')
            index = LatentIndex(loc.shape[1], device=loc.device).add(loc, torch.ones_like(loc))
        n = len(index)
        if n < 3:
            raise ValueError('TSNE needs at least three rows')
        dist, idx = index.knn_graph(self._neighbors(n), self.metric)
        return self.fit_graph(dist, idx, init)

    def fit_graph(self, dist, idx, init=None, n_iter=None):
        """The embedding of a given k-NN graph: dist f32 [N, k], idx int [N, k] (each row's neighbours) on the device.
        init: f32 [N, 2], used as given (default 1e-4 * randn from the seed)."""
        if not (torch.is_tensor(dist) and torch.is_tensor(idx)) or not (dist.is_cuda and idx.is_cuda):
            raise RuntimeError(_NO_CPU)
        n, k = dist.shape
        if tuple(idx.shape) != (n, k):
            raise ValueError('dist and idx differ in shape')
        if not 1.0 < self.perplexity < k:
            raise ValueError(f'perplexity {self.perplexity} must lie in (1, k = {k})')
        dev = dist.device
        dist = dist.to(torch.float32).contiguous()
        nbr = idx.to(torch.int32).contiguous()
        n_iter = self.n_iter if n_iter is None else int(n_iter)
        p, beta = K.tsne_affinities(dist, self.perplexity)
        rev_ptr, rev_edge = reverse_edges(nbr)
        if init is None:
            gen = torch.Generator(device=dev)
            gen.manual_seed(self.seed)
            y = 1e-4 * torch.randn(n, 2, generator=gen, device=dev, dtype=torch.float32)
        else:
            if tuple(init.shape) != (n, 2):
                raise ValueError(f'init: expected [{n}, 2], got {tuple(init.shape)}')
            y = init.to(dev, torch.float32).clone().contiguous()
        lr = self.learning_rate
        if lr == 'auto':
            lr = max(n / self.early_exaggeration / 4.0, 50.0)
        vel, gains = torch.zeros_like(y), torch.ones_like(y)
        rep, attr = torch.empty_like(y), torch.empty_like(y)
        zrow = torch.empty(n, dtype=torch.float32, device=dev)
        zsum = torch.empty(1, dtype=torch.float32, device=dev)
        for it in range(n_iter):   # plain launches on the current stream; nothing here reads the device back
            early = it < self.exaggeration_iter
            K.tsne_repulse(y, rep, zrow, zsum)
            K.tsne_attract(y, nbr, p, rev_ptr, rev_edge, attr)
            K.tsne_update(y, vel, gains, attr, rep, zsum, self.early_exaggeration if early else 1.0, float(lr),
                          0.5 if early else 0.8)
        self.embedding_, self.knn_, self.beta_ = y, (dist, idx), beta
        return y
