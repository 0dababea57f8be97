"""The posterior latents of a corpus and nearest-neighbour search over them: what the reference does with a trained
model in gather_latents.py:26-31 (encode every document to a (mean, scale) pair) and knn.py:28-50 (neighbours of an
article under squared L2 of the means, cosine similarity of the means, and KL between the diagonal Gaussians).

The rows live on the device; every score and the selection run in libsvae's latent kernels (svae_latent_prepare /
svae_latent_scores / svae_latent_topk, csrc/latent.hip). There is no CPU fallback: an index built from CPU tensors
keeps its rows, saves and loads, but refuses to search."""
import numbers
from typing import Iterable, List, Optional, Sequence

import numpy as np
import torch
from torch.distributions.normal import Normal

from . import kernels as K

METRICS = ('l2', 'cosine', 'kl')


def _rows(t, Z, name):
    """[B, Z] or [B, 1, Z] -> f32 [B, Z]."""
    if t.dim() == 3 and t.shape[1] == 1:
        t = t[:, 0]
    if t.dim() == 1:
        t = t[None]
    if t.dim() != 2 or t.shape[-1] != Z:
        raise ValueError(f'{name}: expected [B, {Z}] or [B, 1, {Z}], got {tuple(t.shape)}')
    return t.to(torch.float32)


class LatentIndex:
    def __init__(self, latent_depth: int, device=None):
        if latent_depth % 4 or not 4 <= latent_depth <= 256:
            raise ValueError('latent_depth must be a multiple of 4 in 4..256 (svae_latent_* shapes)')
        self.latent_depth = int(latent_depth)
        self._device = torch.device(device) if device is not None else None
        self._n = 0
        self._cap = 0
        self._loc = self._scale = self._inv_var = self._logdet = self._inv_norm = None
        self._titles: List[str] = []
        self._by_title = None

    # ------------------------------------------------------------------ storage
    def __len__(self):
        return self._n

    @property
    def device(self):
        return self._device

    @property
    def loc(self):
        return self._loc[:self._n] if self._loc is not None else torch.empty(0, self.latent_depth)

    @property
    def scale(self):
        return self._scale[:self._n] if self._scale is not None else torch.empty(0, self.latent_depth)

    @property
    def titles(self):
        return self._titles

    def _reserve(self, n):
        if n <= self._cap:
            return
        cap = max(n, 2 * self._cap, 1024)        # geometric: a gather loop reallocates O(log N) times
        Z, dev = self.latent_depth, self._device

        def grown(old, *shape):
            new = torch.empty(*shape, dtype=torch.float32, device=dev)
            if old is not None and self._n:
                new[:self._n].copy_(old[:self._n])
            return new

        self._loc, self._scale = grown(self._loc, cap, Z), grown(self._scale, cap, Z)
        self._inv_var = grown(self._inv_var, cap, Z)
        self._logdet, self._inv_norm = grown(self._logdet, cap), grown(self._inv_norm, cap)
        self._cap = cap

    def add(self, loc, scale, titles: Optional[Sequence[str]] = None):
        """Append posteriors: loc, scale [B, Z] or [B, 1, Z]. titles: B strings (default: the running row numbers).
        On the device the rows' derived quantities are computed here, once (svae_latent_prepare); nothing
        synchronises."""
        Z = self.latent_depth
        loc, scale = _rows(loc, Z, 'loc'), _rows(scale, Z, 'scale')
        if loc.shape != scale.shape:
            raise ValueError('loc and scale differ in shape')
        if self._device is None:
            self._device = loc.device
        B, n0 = loc.shape[0], self._n
        if titles is None:
            titles = [str(n0 + i) for i in range(B)]
        titles = [str(t) for t in titles]
        if len(titles) != B:
            raise ValueError(f'{len(titles)} titles for {B} rows')
        if B == 0:
            return self
        self._reserve(n0 + B)
        self._loc[n0:n0 + B].copy_(loc, non_blocking=True)
        self._scale[n0:n0 + B].copy_(scale, non_blocking=True)
        if self._device.type == 'cuda':
            K.latent_prepare(self._loc[n0:n0 + B], self._scale[n0:n0 + B], self._inv_var[n0:n0 + B],
                             self._logdet[n0:n0 + B], self._inv_norm[n0:n0 + B])
        self._titles.extend(titles)
        self._by_title = None
        self._n = n0 + B
        return self

    def row_of(self, title: str) -> Optional[int]:
        """Row of the first posterior with this title, or None."""
        if self._by_title is None:
            self._by_title = {}
            for i, t in enumerate(self._titles):
                self._by_title.setdefault(t, i)
        return self._by_title.get(title)

    # ------------------------------------------------------------------ search
    def _corpus(self):
        if self._n == 0:
            raise ValueError('the index is empty')
        if self._device.type != 'cuda':
            raise RuntimeError('LatentIndex searches run on the MI355X HIP kernels (svae_latent_*): move the index to '
                               'a GPU (LatentIndex.load(path, device)). There is no CPU fallback.')
        n = self._n
        return self._loc[:n], self._inv_var[:n], self._logdet[:n], self._inv_norm[:n]

    def _query(self, query):
        """-> (mu, scale, logdet, inv_norm) of the queries, prepared like the rows."""
        Z = self.latent_depth
        if isinstance(query, numbers.Integral) or (torch.is_tensor(query) and not query.is_floating_point()):
            n = self._n
            if torch.is_tensor(query) and query.is_cuda:
                # not read back (that would synchronise): rows outside 0..n-1 are clamped to the nearest valid row
                # instead of reaching a device-side index assert
                idx = query.to(self._device, torch.int64).reshape(-1).clamp(0, n - 1)
            else:
                idx = torch.as_tensor(query if torch.is_tensor(query) else int(query), dtype=torch.int64).reshape(-1)
                if idx.numel() and not (0 <= int(idx.min()) and int(idx.max()) < n):
                    raise IndexError(f'row index outside the index (0..{n - 1}): {idx.tolist()[:8]}')
                idx = idx.to(self._device)
            return (self._loc[:n][idx].contiguous(), self._scale[:n][idx].contiguous(),
                    self._logdet[:n][idx].contiguous(), self._inv_norm[:n][idx].contiguous())
        if isinstance(query, Normal):
            loc, scale = query.loc, query.scale
        else:
            loc, scale = query
        loc = _rows(loc, Z, 'query loc').to(self._device).contiguous()
        scale = _rows(scale, Z, 'query scale').to(self._device).contiguous()
        _, logdet, inv_norm = K.latent_prepare(loc, scale)
        return loc, scale, logdet, inv_norm

    def search(self, query, k: int = 10, metric: str = 'l2'):
        """The k nearest rows per query, best first: (scores f32 [Q, k], indices int64 [Q, k]) on the device. query:
        a Normal, a (loc, scale) pair, or an int / int tensor of rows of this index (a row is its own first hit, as
        in knn.py). An int or a CPU int tensor outside 0..len-1 raises IndexError; a device int tensor is not read
        back, its rows are clamped into that range. metric: 'l2' (squared distance of the means, smallest first), 'cosine' (similarity of the
        means, largest first), 'kl' (KL(query || row), smallest first)."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got '{metric}'")
        corpus = self._corpus()
        scores, indices = K.latent_topk(metric, self._query(query), corpus, int(k))
        return scores, indices.to(torch.int64)

    def knn_graph(self, k: int, metric: str = 'l2', chunk: int = 512):
        """Every row's k nearest other rows, best first: (dist f32 [N, k], idx int32 [N, k]) on the device, the graph
        t-SNE starts from. metric: 'l2' or 'kl' (dissimilarities). Built on `search`: the rows go through
        svae_latent_topk in chunks of `chunk` queries with k + 1 hits each, and the row itself is taken out by index
        (duplicates tie and ties go to the lower row, so a row is not always its own first hit; where it is not among
        its k + 1 hits the last one is dropped). No score is recomputed: a distance is bit-identical to `search`'s.
        Nothing in the loop synchronises with the host."""
        if metric not in ('l2', 'kl'):
            raise ValueError(f"knn_graph: metric must be 'l2' or 'kl' (a dissimilarity), got '{metric}'")
        corpus = self._corpus()
        n, k, chunk = self._n, int(k), int(chunk)
        if not 1 <= k <= min(63, n - 1):
            raise ValueError(f'knn_graph: k = {k} outside 1..min(63, {n} rows - 1)')
        if chunk < 1:
            raise ValueError('knn_graph: chunk must be positive')
        dev = self._device
        dist = torch.empty(n, k, dtype=torch.float32, device=dev)
        idx = torch.empty(n, k, dtype=torch.int32, device=dev)
        rows = torch.arange(n, dtype=torch.int32, device=dev)
        for c0 in range(0, n, chunk):
            c1 = min(n, c0 + chunk)
            query = (self._loc[c0:c1], self._scale[c0:c1], self._logdet[c0:c1], self._inv_norm[c0:c1])
            s, i = K.latent_topk(metric, query, corpus, k + 1)
            drop = i == rows[c0:c1, None]
            drop[:, -1] |= ~drop.any(dim=1)
            keep = torch.argsort(drop.to(torch.int8), dim=1, stable=True)[:, :k]   # the k kept hits, in their order
            dist[c0:c1] = s.gather(1, keep)
            idx[c0:c1] = i.gather(1, keep)
        return dist, idx

    def scores(self, query, metric: str = 'l2'):
        """The dense [Q, N] score matrix of `metric` (svae_latent_scores)."""
        if metric not in METRICS:
            raise ValueError(f"metric must be one of {METRICS}, got '{metric}'")
        corpus = self._corpus()
        return K.latent_scores(metric, self._query(query), corpus)

    # ------------------------------------------------------------------ aggregate posterior
    def stats(self, threshold: float = 0.01):
        """Per latent dimension over the rows (svae_latent_colstats, f64 [Z] on the device): `mean_loc`, `var_loc`
        (unbiased) and `mean_kl`, the mean KL(q(z_d|x) || N(0, 1)); `active_units`: the number of dimensions with
        Var[mu_d] > threshold (Burda et al. 2016); `kl`: the sum of mean_kl (the mean KL term of the ELBO)."""
        self._corpus()
        n = self._n
        mean_loc, var_loc, mean_kl = K.latent_colstats(self._loc[:n], self._scale[:n])
        return {'mean_loc': mean_loc, 'var_loc': var_loc, 'mean_kl': mean_kl,
                'active_units': int((var_loc > threshold).sum().item()), 'kl': float(mean_kl.sum().item())}

    def mmd(self, kind: str = 'rbf', source: str = 'sample', seed: int = 0, standardize: bool = True):
        """MMD^2 between the aggregate posterior and a Gaussian, as a 0-dim f64 tensor on the device. source 'sample':
        one draw z_i ~ q(z|x_i) per row (svae_latent_draw, counter RNG keyed by `seed`): a sample of the aggregate
        posterior; 'mean': the posterior means. kind 'rbf': analytic_gaussian_rbf_mmd_sq against N(0, I); 'rbf_fitted':
        custom_gaussian_rbf_mmd_sq against the diagonal Gaussian with the rows' own mean and variance per dimension
        (svae_latent_colstats); 'imq': gaussian_imq_mmd_sq (not standardised; its prior samples come from `seed`)."""
        from .core import math_utils as MU
        if kind not in ('rbf', 'rbf_fitted', 'imq'):
            raise ValueError(f"mmd: kind must be 'rbf', 'rbf_fitted' or 'imq', got '{kind}'")
        if source not in ('sample', 'mean'):
            raise ValueError(f"mmd: source must be 'sample' or 'mean', got '{source}'")
        self._corpus()
        n = self._n
        if n < 2:
            raise ValueError('mmd: at least two rows')
        loc, scale = self._loc[:n], self._scale[:n]
        z = K.latent_draw(loc, scale, seed=seed) if source == 'sample' else loc
        if kind == 'rbf':
            return MU.analytic_gaussian_rbf_mmd_sq(z, standardize)
        if kind == 'imq':
            return MU.gaussian_imq_mmd_sq(z, seed=seed)
        mean, var, _ = K.latent_colstats(z, scale)
        return MU.custom_gaussian_rbf_mmd_sq(z, mean, var, standardize)

    def kmeans(self, n_clusters: int, **kw):
        """k-means of the posterior means (svae_kmeans_*): KMeans(n_clusters, **kw).fit(self), see sparse_vae.kmeans."""
        from .kmeans import KMeans
        return KMeans(n_clusters, **kw).fit(self)

    def fit_mixture(self, n_components: int, source: str = 'posterior', **kw):
        """A Gaussian-mixture prior of the index (svae_gmm_*): GaussianMixture(n_components, **kw) fitted to the
        posteriors N(loc, scale^2) ('posterior', the default) or to the means as points ('mean': a collapsed dimension
        then gets a variance of about reg_covar, see sparse_vae.mixture)."""
        from .mixture import GaussianMixture
        if source not in ('posterior', 'mean'):
            raise ValueError(f"source must be 'posterior' or 'mean', got {source!r}")
        gm = GaussianMixture(n_components, **kw)
        if source == 'posterior' or len(self) == 0 or self.device is None or self.device.type != 'cuda':
            return gm.fit(self)          # the empty and the CPU index are refused there
        return gm.fit(self.loc.contiguous())

    def log_density(self, z, per_dim: bool = False, skip=None):
        """log q(z) of the aggregate posterior q(z) = (1 / N) sum_j N(loc_j, scale_j^2) at the points z [M, Z], against
        every row of the index (svae_aggpost_logq): logq f32 [M] on the device, or with per_dim (logq, logq_dim f32
        [M, Z], the log-density of each dimension's marginal). skip: int [M], the row each point leaves out of the sum
        (-1: none), e.g. the row it was drawn from; the density is then over the N - 1 others."""
        loc, _, _, _ = self._corpus()
        z = _rows(torch.as_tensor(z), self.latent_depth, 'z').to(self._device).contiguous()
        if skip is not None:
            skip = torch.as_tensor(skip).reshape(-1).to(self._device, torch.int32).contiguous()
            if skip.numel() != z.shape[0]:
                raise ValueError(f'log_density: {skip.numel()} skip rows for {z.shape[0]} points')
        return K.aggpost_logq(z, loc, self._scale[:self._n], skip=skip, per_dim=per_dim)

    def elbo_surgery(self, samples: Optional[int] = None, seed: int = 0, leave_one_out: bool = False, eps=None,
                     rows=None):
        """The mean KL of the index split as I_q(x; z) + KL(q(z) || p(z)), and the marginal term as a total correlation
        plus per-dimension KLs: an ElboSurgery (sparse_vae.surgery, which says what each field is and which way each
        variant is biased). One z_i ~ q(z | x_i) is drawn per sampled row (svae_latent_draw keyed by `seed`, or
        loc + scale * eps with eps f32 [samples, Z] injected) and log q(z_i) is taken against all N rows. rows: the
        rows to draw from; default all of them when samples is None or >= N, else a sorted subset from a seeded
        torch.randperm on the CPU. leave_one_out: leave each point's own row out of q(z_i)."""
        from .surgery import elbo_surgery
        loc, _, _, _ = self._corpus()
        return elbo_surgery(loc, self._scale[:self._n], samples=samples, seed=seed, leave_one_out=leave_one_out,
                            eps=eps, rows=rows)

    # ------------------------------------------------------------------ persistence
    def save(self, path):
        """One .npz: loc, scale, titles. The derived rows are not stored (load recomputes them)."""
        with open(path, 'wb') as f:
            np.savez(f, loc=self.loc.detach().cpu().numpy(), scale=self.scale.detach().cpu().numpy(),
                     titles=np.asarray(self._titles, dtype=np.str_))

    @classmethod
    def load(cls, path, device=None):
        with np.load(path, allow_pickle=False) as z:
            loc, scale, titles = z['loc'], z['scale'], [str(t) for t in z['titles']]
        index = cls(loc.shape[1], device=device)
        if len(loc):
            dev = index._device if index._device is not None else torch.device('cpu')
            index.add(torch.from_numpy(loc).to(dev), torch.from_numpy(scale).to(dev), titles)
        return index


@torch.no_grad()
def gather_latents(model, batches: Iterable, titles_key: str = 'title') -> LatentIndex:
    """gather_latents.py:26-31: q(z|x) of every batch through model.encode (encoder only), appended on the device
    with no per-batch host synchronisation. Batches without `titles_key` get their running row numbers as titles."""
    index = LatentIndex(model.hparams.latent_depth, device=model.device)
    for batch in batches:
        q = model.encode(batch)
        titles = batch.get(titles_key) if hasattr(batch, 'get') else None
        if titles is not None:
            titles = [''.join(t) if not isinstance(t, str) else t for t in titles]
        index.add(q.loc, q.scale, titles)
    return index
