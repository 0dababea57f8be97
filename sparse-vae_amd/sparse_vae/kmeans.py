"""k-means of the posterior means: what the latent space groups documents by, from the latents alone. It stands in for
the topic colouring of the reference's tsne.py:38-63 (an LDA model fitted with gensim on the bag of words), which
needs the tokenised corpus and a third-party package.

k-means++ seeding, the assignment and the centroid update are libsvae's svae_kmeans_* kernels (csrc/kmeans.hip). None
of them uses an atomic, so one seed gives one result bit for bit. There is no CPU fallback."""
import torch

from . import kernels as K
from .latent_index import LatentIndex, _rows

_NO_CPU = ('KMeans runs on the MI355X HIP kernels (svae_kmeans_*): give it a LatentIndex or a tensor on a GPU '
           '(LatentIndex.load(path, device)). There is no CPU fallback.')


class KMeans:
    """Lloyd's iteration from k-means++ starts.

    init: 'k-means++' (n_init starts, start r seeded with seed + r; the start with the lowest final inertia wins,
    ties go to the lower r) or an f32 [K, Z] tensor (one start from these centroids; n_init is ignored).
    Convergence is "no label changed"; there is no tolerance. The counter is read back only every check_every
    iterations: the update is deterministic, so iterations past the fixed point reproduce it bit for bit and the
    result does not depend on check_every. n_iter_ is the first polled iteration with no change, or max_iter.

    After fit: cluster_centers_ f32 [K, Z], labels_ int64 [N] and inertia_ (a float) of the last assignment, counts_
    int64 [K] (an empty cluster keeps its centroid and counts 0), n_iter_, seed_rows_ int64 [K] (the rows the winning
    start drew; None with a tensor init)."""

    def __init__(self, n_clusters, n_init=4, max_iter=100, init='k-means++', seed=0, check_every=4):
        if torch.is_tensor(init):
            if init.dim() != 2 or init.shape[0] != n_clusters:
                raise ValueError(f'init: expected [{n_clusters}, Z], got {tuple(init.shape)}')
        elif init != 'k-means++':
            raise ValueError(f"init must be 'k-means++' or a [K, Z] tensor, got {init!r}")
        if int(n_clusters) < 1 or int(n_init) < 1 or int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError('n_clusters, n_init, max_iter and check_every must be positive')
        self.n_clusters, self.n_init, self.max_iter = int(n_clusters), int(n_init), int(max_iter)
        self.init, self.seed, self.check_every = init, int(seed), int(check_every)
        self.cluster_centers_ = self.labels_ = self.counts_ = self.inertia_ = self.n_iter_ = self.seed_rows_ = None

    @staticmethod
    def _means(x):
        """A LatentIndex (its means) or an f32 [N, Z] / [N, 1, Z] device tensor -> f32 [N, Z], contiguous."""
        if isinstance(x, LatentIndex):
            if len(x) == 0:
                raise ValueError('the index is empty')
            if x.device is None or x.device.type != 'cuda':
                raise RuntimeError(_NO_CPU)
            return x.loc.contiguous()
        if not torch.is_tensor(x):
            raise TypeError('KMeans takes a LatentIndex or a tensor')
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise ValueError(f'expected [N, Z] or [N, 1, Z], got {tuple(x.shape)}')
        return _rows(x, x.shape[-1], 'x').contiguous()

    def _lloyd(self, x, cent):
        """One start, in place on cent -> (label int32 [N], count int32 [K], inertia f64 [1], n_iter)."""
        n, dev = x.shape[0], x.device
        label = torch.full((n,), -1, dtype=torch.int32, device=dev)
        count = torch.empty(self.n_clusters, dtype=torch.int32, device=dev)
        changed = torch.empty(1, dtype=torch.int32, device=dev)
        inertia = torch.empty(1, dtype=torch.float64, device=dev)
        n_iter = self.max_iter
        for it in range(1, self.max_iter + 1):
            K.kmeans_assign(x, cent, label, None, changed, inertia, want_d2=False)
            K.kmeans_update(x, label, cent, count)
            if it % self.check_every == 0 and int(changed.item()) == 0:   # the only read-back of the loop
                n_iter = it
                break
        return label, count, inertia, n_iter

    def fit(self, x):
        x = self._means(x)
        n, Z = x.shape
        k = self.n_clusters
        if k > n:
            raise ValueError(f'n_clusters = {k} exceeds the {n} rows')
        if torch.is_tensor(self.init):
            if self.init.shape[1] != Z:
                raise ValueError(f'init: expected [{k}, {Z}], got {tuple(self.init.shape)}')
            starts = [(None, self.init.to(x.device, torch.float32).clone().contiguous())]
        else:
            starts = [K.kmeans_seed(x, k, seed=self.seed + r) for r in range(self.n_init)]
        best = None
        for rows, cent in starts:
            label, count, inertia, n_iter = self._lloyd(x, cent)
            inertia = float(inertia.item())
            if best is None or inertia < best[0]:
                best = (inertia, cent, label, count, n_iter, rows)
        inertia, cent, label, count, n_iter, rows = best
        self.inertia_, self.cluster_centers_, self.n_iter_ = inertia, cent, n_iter
        self.labels_, self.counts_ = label.to(torch.int64), count.to(torch.int64)
        self.seed_rows_ = None if rows is None else rows.to(torch.int64)
        return self

    def predict(self, x):
        """The nearest of cluster_centers_ per row: int64 [N] on the device."""
        if self.cluster_centers_ is None:
            raise RuntimeError('KMeans.predict before fit')
        x = self._means(x)
        label, _, _, _ = K.kmeans_assign(x, self.cluster_centers_, want_d2=False)
        return label.to(torch.int64)

    def fit_predict(self, x):
        return self.fit(x).labels_
