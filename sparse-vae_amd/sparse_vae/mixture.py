"""A Gaussian-mixture prior fitted to the aggregate posterior after training (ex-post density estimation, Ghosh et al.
2020): what to do when latent_stats.py shows that the aggregate posterior does not match N(0, I). It stands where the
reference has only torch.randn (transformer_vae.py:103): draw z from the mixture and hand it to sample_stream(z=...),
sample(z=...) or beam_search(z=...).

The fit takes each row as the Gaussian q_i = N(mu_i, diag(s2_i)), not as the point mu_i: a collapsed latent dimension
has mu ~ 0 and s2 ~ 1 in every row, so a mixture of the means would give it a variance of about reg_covar and feed the
decoder z_d ~ 0 where training always showed it z_d ~ N(0, 1). EM ascends

    L = (1 / N) sum_i logsumexp_k a_ik,  a_ik = E_{q_i} log pi_k N(z; m_k, v_k),

a lower bound on the aggregate posterior's expected log-density under the mixture; with points (no variances) it is the
textbook diagonal GMM and L is the mean log-likelihood.

The E-step, the M-step, the sampler and the density are libsvae's svae_gmm_* kernels (csrc/gmm.hip). None of them uses an
atomic, so one seed gives one result bit for bit. There is no CPU fallback."""
import numpy as np
import torch

from . import _native as N
from . import kernels as K
from .kmeans import KMeans
from .latent_index import LatentIndex, _rows

_NO_CPU = ('GaussianMixture runs on the MI355X HIP kernels (svae_gmm_*): give it a LatentIndex or tensors on a GPU '
           '(LatentIndex.load(path, device)). There is no CPU fallback.')


class GaussianMixture:
    """A mixture of n_components diagonal Gaussians fitted by EM.

    init: 'kmeans' (n_init starts; start r is KMeans(K, n_init=1, seed=seed + r) on the means followed by a hard
    M-step; the start with the highest final bound wins, ties go to the lower r, a NaN bound loses to every number) or a (weights [K], means [K, Z],
    variances [K, Z]) triple (one start; n_init is ignored).

    Which iterate is kept. Iteration t = 1, 2, ... is an E-step under the parameters theta_{t-1}, which gives their
    bound B_{t-1}, followed by an M-step, which gives theta_t. The fit stops at the first t >= 2 with
    |B_{t-1} - B_{t-2}| < tol (per row: sklearn's default and meaning) and keeps theta_t; lower_bound_ is B_{t-1}, the
    last bound computed, as sklearn reports it. Without such a t it keeps theta_{max_iter} and converged_ is False.
    The bounds stay on the device and are read back only every check_every iterations; the parameters of the last
    check_every iterations are kept there too, so the t found, and with it every result, is the same for every
    check_every: it only decides how many iterations run past t before the loop notices.

    After fit: weights_ f32 [K], means_, variances_ f32 [K, Z] (device tensors), nk_ f64 [K] (the responsibilities'
    column sums behind theta_t), lower_bound_ (a float, per row), lower_bounds_ (B_0 .. B_{t-1}, per row), n_iter_ = t,
    converged_."""

    def __init__(self, n_components, max_iter=100, tol=1e-3, reg_covar=1e-6, n_init=1, seed=0, check_every=4,
                 init='kmeans'):
        if isinstance(init, (tuple, list)):
            if len(init) != 3:
                raise ValueError('init: a (weights, means, variances) triple')
            w, m, v = (torch.as_tensor(t) for t in init)
            if m.dim() != 2 or m.shape[0] != n_components or v.shape != m.shape or w.shape != (n_components,):
                raise ValueError(f'init: expected weights [{n_components}] and means, variances [{n_components}, Z]')
            init = (w, m, v)
        elif init != 'kmeans':
            raise ValueError(f"init must be 'kmeans' or a (weights, means, variances) triple, got {init!r}")
        if int(n_components) < 1 or int(n_init) < 1 or int(max_iter) < 1 or int(check_every) < 1:
            raise ValueError('n_components, n_init, max_iter and check_every must be positive')
        if int(n_components) > N.GMM_MAX_K:
            raise ValueError(f'n_components = {n_components} exceeds SVAE_GMM_MAX_K = {N.GMM_MAX_K}')
        if not float(reg_covar) >= 0 or not float(tol) >= 0:
            raise ValueError('reg_covar and tol must not be negative')
        self.n_components, self.max_iter, self.n_init = int(n_components), int(max_iter), int(n_init)
        self.tol, self.reg_covar = float(tol), float(reg_covar)
        self.seed, self.check_every, self.init = int(seed), int(check_every), init
        self.weights_ = self.means_ = self.variances_ = self.nk_ = None
        self.lower_bound_ = self.lower_bounds_ = self.n_iter_ = self.converged_ = None
        self._params = None

    # ------------------------------------------------------------------ operands
    @staticmethod
    def _inputs(x, variances=None):
        """A LatentIndex (its posteriors) or f32 [N, Z] / [N, 1, Z] device tensors -> (x, s2 or None), contiguous."""
        if isinstance(x, LatentIndex):
            if len(x) == 0:
                raise ValueError('the index is empty')
            if x.device is None or x.device.type != 'cuda':
                raise RuntimeError(_NO_CPU)
            if variances is not None:
                raise ValueError('a LatentIndex brings its own variances')
            return x.loc.contiguous(), (x.scale * x.scale).contiguous()
        if not torch.is_tensor(x):
            raise TypeError('GaussianMixture takes a LatentIndex or tensors')
        if not x.is_cuda or (variances is not None and not variances.is_cuda):
            raise RuntimeError(_NO_CPU)
        if x.dim() == 3 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 2:
            raise ValueError(f'expected [N, Z] or [N, 1, Z], got {tuple(x.shape)}')
        Z = x.shape[-1]
        x = _rows(x, Z, 'x').contiguous()
        if variances is not None:
            variances = _rows(variances, Z, 'variances').contiguous()
            if variances.shape != x.shape:
                raise ValueError('x and variances differ in shape')
        return x, variances

    def _fitted(self, what, device=True):
        """(K, Z) of the model; with device, refuses a model that was made or loaded on the CPU."""
        if self.means_ is None:
            raise RuntimeError(f'GaussianMixture.{what} before fit')
        if device and self._params is None:
            raise RuntimeError(_NO_CPU)
        return self.means_.shape

    def _set(self, params, Z):
        k = self.n_components
        self._params = params
        self.weights_, self.means_ = K.gmm_view(params, k, Z, 'weight'), K.gmm_view(params, k, Z, 'mean')
        self.variances_ = K.gmm_view(params, k, Z, 'var')

    # ------------------------------------------------------------------ fit
    def _em(self, x, s2, params):
        """One start, from the block params -> (params, nk, bounds per row (list), n_iter, converged)."""
        n, dev, k = x.shape[0], x.device, self.n_components
        bounds = torch.zeros(self.max_iter, dtype=torch.float64, device=dev)   # bounds[t - 1] = sum lse under theta_{t-1}
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        kept = {}                                                              # t -> (theta_t, nk_t), the last ones
        for t in range(1, self.max_iter + 1):
            K.gmm_estep(x, s2, params, k, lse=lse, bound=bounds[t - 1:t], want_label=False)
            nk = K.gmm_mstep(x, s2, params, k, lse=lse, reg_covar=self.reg_covar)
            kept[t] = (params.clone(), nk)
            kept.pop(t - self.check_every - 1, None)
            if t % self.check_every == 0 or t == self.max_iter:               # the only read-back of the loop
                b = (bounds[:t] / n).tolist()
                for s in range(max(2, t - self.check_every + 1), t + 1):
                    if abs(b[s - 1] - b[s - 2]) < self.tol:
                        return kept[s] + (b[:s], s, True)
        return kept[self.max_iter] + (b, self.max_iter, False)

    def _start(self, x, s2, r):
        k, Z = self.n_components, x.shape[1]
        if self.init != 'kmeans':
            w, m, v = (t.to(x.device, torch.float32).contiguous() for t in self.init)
            if m.shape[1] != Z:
                raise ValueError(f'init: expected means [{k}, {Z}], got {tuple(m.shape)}')
            return K.gmm_pack(w, m, v)
        km = KMeans(k, n_init=1, seed=self.seed + r).fit(x)
        params = K.gmm_pack(torch.full((k,), 1.0 / k, device=x.device), km.cluster_centers_,
                            torch.ones(k, Z, device=x.device))
        K.gmm_mstep(x, s2, params, k, label=km.labels_.to(torch.int32), reg_covar=self.reg_covar)
        return params

    def fit(self, x, variances=None):
        """x: a LatentIndex (fitted to its posteriors N(loc, scale^2)), or the means f32 [N, Z] with their variances
        [N, Z], or points (variances None)."""
        x, s2 = self._inputs(x, variances)
        if self.init == 'kmeans' and self.n_components > x.shape[0]:
            raise ValueError(f'n_components = {self.n_components} exceeds the {x.shape[0]} rows')
        best = None
        for r in range(self.n_init if self.init == 'kmeans' else 1):
            out = self._em(x, s2, self._start(x, s2, r))
            if best is None or out[2][-1] > best[2][-1] or (best[2][-1] != best[2][-1] and out[2][-1] == out[2][-1]):
                best = out
        params, nk, bounds, n_iter, converged = best
        self._set(params, x.shape[1])
        self.nk_, self.lower_bounds_, self.lower_bound_ = nk, bounds, bounds[-1]
        self.n_iter_, self.converged_ = n_iter, converged
        return self

    # ------------------------------------------------------------------ density
    def _estep(self, x, variances, **kw):
        Z = self._fitted('score_samples')[1]
        x, s2 = self._inputs(x, variances)
        if x.shape[1] != Z:
            raise ValueError(f'expected rows of {Z}, got {x.shape[1]}')
        return K.gmm_estep(x, s2, self._params, self.n_components, **kw), x.shape[0]

    def score_samples(self, x, variances=None):
        """Per row logsumexp_k a_ik, f32 [N] on the device: the log-density of a point, or with variances (or a
        LatentIndex) the bound on E_{q_i} log p(z). In nats."""
        return self._estep(x, variances, want_label=False)[0][0]

    def score(self, x, variances=None):
        """The mean of score_samples, from the kernel's f64 sum: a float, nats per row."""
        (_, _, _, bound), n = self._estep(x, variances, want_label=False)
        return float(bound.item()) / n

    def predict(self, x, variances=None):
        """The component of largest a_ik per row: int64 [N] on the device."""
        return self._estep(x, variances)[0][1].to(torch.int64)

    def predict_proba(self, x, variances=None):
        """The responsibilities f32 [N, K] (N * K floats: meant for small N)."""
        return self._estep(x, variances, want_label=False, want_resp=True)[0][2]

    def bic(self, x, variances=None):
        """-2 sum_i score_i + (2 K Z + K - 1) log N."""
        (_, _, _, bound), n = self._estep(x, variances, want_label=False)
        k, Z = self.means_.shape
        return -2.0 * float(bound.item()) + (2 * k * Z + k - 1) * float(np.log(n))

    # ------------------------------------------------------------------ sampling
    def sample(self, n, seed=0):
        """n draws -> (z f32 [n, 1, Z], comp int64 [n]), z ready for sample_stream(z=), sample(z=) or beam_search(z=).
        The component and the normals come from the library's counter RNG keyed by seed."""
        k, Z = self._fitted('sample')
        z, comp = K.gmm_sample(self._params, k, Z, int(n), seed=seed)
        return z[:, None, :], comp.to(torch.int64)

    # ------------------------------------------------------------------ models
    @classmethod
    def from_parameters(cls, weights, means, variances, **kw):
        """A model from hand-made or loaded parameters. On the CPU it only keeps, saves and loads them."""
        gm = cls(means.shape[0], **kw)
        w, m, v = (t.to(means.device, torch.float32).contiguous() for t in (weights, means, variances))
        if m.dim() != 2 or v.shape != m.shape or w.shape != m.shape[:1]:
            raise ValueError('expected weights [K] and means, variances [K, Z]')
        if m.is_cuda:
            gm._set(K.gmm_pack(w, m, v), m.shape[1])
        else:
            gm.weights_, gm.means_, gm.variances_ = w, m, v
        return gm

    @classmethod
    def standard_normal(cls, latent_depth, device=None):
        """The K = 1 prior N(0, I): the baseline of every figure."""
        dev = torch.device(device if device is not None else 'cpu')
        return cls.from_parameters(torch.ones(1, device=dev), torch.zeros(1, latent_depth, device=dev),
                                   torch.ones(1, latent_depth, device=dev))

    _SETTINGS = ('max_iter', 'tol', 'reg_covar', 'n_init', 'seed', 'check_every')

    def save(self, path):
        """One .npz: weights, means, variances and the settings."""
        self._fitted('save', device=False)
        arrays = dict(weights=self.weights_.cpu().numpy(), means=self.means_.cpu().numpy(),
                      variances=self.variances_.cpu().numpy())
        for s in self._SETTINGS:
            arrays[s] = np.asarray(getattr(self, s))
        for s in ('lower_bound_', 'n_iter_', 'converged_'):
            if getattr(self, s) is not None:
                arrays[s] = np.asarray(getattr(self, s))
        np.savez(path, **arrays)

    @classmethod
    def load(cls, path, device=None):
        dev = torch.device(device if device is not None else 'cpu')
        with np.load(path) as f:
            kw = {s: f[s].item() for s in cls._SETTINGS}
            gm = cls.from_parameters(*(torch.from_numpy(f[a]).to(dev) for a in ('weights', 'means', 'variances')),
                                     **kw)
            for s in ('lower_bound_', 'n_iter_', 'converged_'):
                if s in f.files:
                    setattr(gm, s, f[s].item())
        return gm
