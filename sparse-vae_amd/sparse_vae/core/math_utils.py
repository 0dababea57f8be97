"""marginal_kl (math_utils.py:51-58 in the reference): the Monte-Carlo marginal KL behind the train_mc_mutual_info
diagnostic, on the fused HIP kernel pair (`svae_mutual_info`: mi_marginal + mi_final) the training step uses
through engine.mutual_info. Same signature as the reference (a Normal posterior [B, 1, Z], num_samples draws);
`eps` [num_samples, B, Z] injects the N(0, 1) draws (parity tests), otherwise they are drawn in-kernel from a seed
taken from torch's generator. No CPU fallback."""
import math

import torch

from .. import kernels as K


@torch.no_grad()
def marginal_kl(posteriors, num_samples: int = 10, eps=None):
    mu, scale = posteriors.loc, posteriors.scale
    if not mu.is_cuda:
        raise RuntimeError('marginal_kl runs on the MI355X HIP kernels (svae_mutual_info): no CPU fallback')
    B, Z = mu.shape[0], mu.shape[-1]
    if mu.numel() != B * Z:
        raise ValueError('marginal_kl expects a posterior of shape [B, 1, latent] (transformer_vae.py:52-61)')
    # the kernel's posterior statistics row: mu | logvar (scale = exp(logvar / 2))
    stats = torch.cat([mu.reshape(B, Z).float(), 2.0 * scale.reshape(B, Z).float().log()], dim=1).contiguous()
    zero = torch.zeros(1, dtype=torch.float32, device=mu.device)
    out = torch.empty((), dtype=torch.float32, device=mu.device)
    ws = torch.empty(2 * num_samples * B, dtype=torch.float32, device=mu.device)
    if eps is not None:
        eps = eps.to(mu.device, torch.float32).reshape(num_samples, B, Z).contiguous()
    seed = int(torch.randint(0, 2 ** 62, (1,)).item())
    K.mutual_info(stats, zero, B, Z, seed, out, ws, eps=eps, S=num_samples)   # out = 0 - marginal_kl
    return -out


@torch.no_grad()
def pairwise_gaussian_kl(gaussians):
    """math_utils.py:90-101: all pairwise KL divergences of a batch of diagonal Gaussians ([B, Z] or [B, 1, Z]) as a
    square matrix in the reference's [P, Q] convention: entry [p, q] = KL(gaussians[p] || gaussians[q]). Runs on the
    latent-score kernel (`svae_latent_scores`, the KL metric with the batch as both queries and corpus). No CPU
    fallback."""
    mu, scale = gaussians.loc, gaussians.scale
    if not mu.is_cuda:
        raise RuntimeError('pairwise_gaussian_kl runs on the MI355X HIP kernels (svae_latent_scores): no CPU fallback')
    mu = mu.flatten(1).float().contiguous()
    scale = scale.flatten(1).float().contiguous()
    inv_var, logdet, inv_norm = K.latent_prepare(mu, scale)
    return K.latent_scores('kl', (mu, scale, logdet, inv_norm), (mu, inv_var, logdet, inv_norm))


# ---- MMD estimators (math_utils.py:104-184) ---------------------------------------------------------------------------
# The O(N^2) pair sums and the O(N) row sums come from svae_pairsum / svae_mmd_rowterm as f64; everything else is
# scalar algebra on the host in Python floats (f64), factored below so that it is callable without a device.
IMQ_BASE_SCALES = (0.1, 0.2, 0.5, 1.0, 2.0, 5.0, 10.0)
IMQ_PRIOR_SAMPLES = 1000


def rbf_kernel_var(d):
    return 0.125 * d


def rbf_analytic_algebra(n, d):
    """(normalizer, first_term, null_variance) of analytic_gaussian_rbf_mmd_sq for n rows of dimension d."""
    kv = rbf_kernel_var(d)
    normalizer = (kv / (1 + kv)) ** (d / 2)
    first_term = (kv / (2 + kv)) ** (d / 2)
    ugly_term = 2 * (kv ** 2 / ((1 + kv) * (3 + kv))) ** (d / 2)
    variance = (2 / (n * (n - 1))) * (first_term ** 2 + (kv / (4 + kv)) ** (d / 2) - ugly_term)
    return normalizer, first_term, variance


def rbf_custom_algebra(n, var):
    """(normalizer, first_term, null_variance) of custom_gaussian_rbf_mmd_sq; var: the d variances as Python floats.
    The log-determinants are sums of math.log in the order of the dimensions."""
    d = len(var)
    kv = rbf_kernel_var(d)
    klv = math.log(kv)

    def logdet(c):
        return 0.5 * math.fsum(math.log(c * v + kv) for v in var)

    ld1, ld2, ld3, ld4 = logdet(1), logdet(2), logdet(3), logdet(4)
    normalizer = math.exp(klv * d / 2 - ld1)
    first_term = math.exp(klv * d / 2 - ld2)
    ugly_term = math.exp(math.log(2) + klv * d - ld1 - ld3)
    variance = 2 / (n * (n - 1)) * (first_term ** 2 + math.exp(klv * d / 2 - ld4) - ugly_term)
    return normalizer, first_term, variance


def rbf_combine(n, normalizer, first_term, variance, row_sum, pair_sum, standardize):
    """first - 2 normalizer mean(row terms) + mean(pair terms) from the two sums, over the null standard error if
    standardize."""
    mmd_sq = first_term - 2 * normalizer * (row_sum / n) + pair_sum / (n * (n - 1) / 2)
    return mmd_sq / variance ** 0.5 if standardize else mmd_sq


def imq_scales(d):
    """The seven scales as the f32 values the reference's tensor holds: fl32(fl32(base) * 2d)."""
    import numpy as np
    return [float(np.float32(b) * np.float32(2 * d)) for b in IMQ_BASE_SCALES]


def imq_combine(n, n_cross, n_pair, x_pair_sum, cross_sum, prior_pair_sum):
    """mean over scales and pairs of x - 2 mean over scales and the n x n_cross cross pairs + mean over scales and
    pairs of the n_pair prior samples; each *_sum is already summed over the seven scales."""
    s = len(IMQ_BASE_SCALES)
    return (x_pair_sum / (s * (n * (n - 1) / 2)) - 2 * cross_sum / (s * n * n_cross)
            + prior_pair_sum / (s * (n_pair * (n_pair - 1) / 2)))


def _device_rows(x, name):
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError(f'{name}: x must be a [N, Z] tensor')
    if not x.is_cuda:
        raise RuntimeError(f'{name} runs on the MI355X HIP kernels (svae_pairsum, svae_mmd_rowterm): no CPU fallback')
    n, d = x.shape
    if n < 2:
        raise ValueError(f'{name}: at least two rows')
    return x.to(torch.float32).contiguous(), n, d


def _scalar(v, dev):
    return torch.tensor(v, dtype=torch.float64, device=dev)


@torch.no_grad()
def analytic_gaussian_rbf_mmd_sq(x, standardize=True):
    """math_utils.py:107-123: the unbiased estimate of MMD^2 between the distribution of the rows of x [N, Z] and
    N(0, I) under a Gaussian RBF kernel of variance Z / 8; standardize: over its standard error under the null.
    Returns a 0-dim f64 tensor on x's device (one host synchronisation to read the two sums)."""
    x, n, d = _device_rows(x, 'analytic_gaussian_rbf_mmd_sq')
    kv = rbf_kernel_var(d)
    w = torch.full((d,), 1.0 / (1.0 + kv), dtype=torch.float32, device=x.device)
    row = K.mmd_rowterm(x, w)
    pair = K.pairsum(x, kind='rbf', params=[0.5 / kv])
    normalizer, first_term, variance = rbf_analytic_algebra(n, d)
    return _scalar(rbf_combine(n, normalizer, first_term, variance, row.item(), pair.item(), standardize), x.device)


@torch.no_grad()
def custom_gaussian_rbf_mmd_sq(x, mean, var, standardize=True):
    """math_utils.py:128-153: as analytic_gaussian_rbf_mmd_sq, against the diagonal Gaussian N(mean, diag(var)).
    mean and var: a scalar (the same in every dimension) or [Z]. The reference also accepts var of shape [N, Z] (a
    variance per row); that form is not provided and raises ValueError."""
    if not torch.is_tensor(x) or x.dim() != 2:
        raise ValueError('custom_gaussian_rbf_mmd_sq: x must be a [N, Z] tensor')
    d = x.shape[1]

    def vec(v, name):
        v = torch.as_tensor(v, dtype=torch.float64).detach().cpu()
        if v.dim() == 2:
            raise ValueError(f'custom_gaussian_rbf_mmd_sq: {name} of shape [N, Z] (one per row) is not supported; '
                             f'pass a scalar or [Z]')
        if v.numel() not in (1, d):
            raise ValueError(f'custom_gaussian_rbf_mmd_sq: {name} must be a scalar or [{d}]')
        return v.reshape(-1).expand(d)

    mean_v, var_v = vec(mean, 'mean'), vec(var, 'var')
    x, n, d = _device_rows(x, 'custom_gaussian_rbf_mmd_sq')
    var_l = [float(v) for v in var_v]
    if not all(v >= 0 for v in var_l):
        raise ValueError('custom_gaussian_rbf_mmd_sq: var must not be negative')
    kv = rbf_kernel_var(d)
    w = (1.0 / (kv + var_v)).to(torch.float32).to(x.device)
    m = mean_v.to(torch.float32).contiguous().to(x.device)
    row = K.mmd_rowterm(x, w, m)
    pair = K.pairsum(x, kind='rbf', params=[0.5 / kv])
    normalizer, first_term, variance = rbf_custom_algebra(n, var_l)
    return _scalar(rbf_combine(n, normalizer, first_term, variance, row.item(), pair.item(), standardize), x.device)


_IMQ_PRIOR = {}


def imq_prior_samples(d, seed=None, n=IMQ_PRIOR_SAMPLES):
    """Two sets of n draws from N(0, I_d) by one torch CPU generator (seed None: 0), one after the other, each
    standardised over all its elements to exactly zero mean and unit (unbiased) variance (math_utils.py:163-168):
    (cross, pair), f32 [n, d] each, on the CPU. The reference uses a first draw in its cross term and a second in its
    prior-prior term: its two helpers call the cached sampler with different argument lists, (d, device) and
    (d, device, n), so the cache holds two draws. After torch.manual_seed(seed) it draws exactly these."""
    g = torch.Generator().manual_seed(0 if seed is None else int(seed))
    out = []
    for _ in range(2):
        raw = torch.randn(n, d, generator=g)
        var, mean = torch.var_mean(raw)
        out.append((raw - mean) / var.sqrt())
    return tuple(out)


def _imq_prepare(cross, pair):
    """(cross samples, their column offsets d - |p|^2, the number of pair samples, the sum over the seven scales of
    the pair samples' own pair sums)."""
    d = cross.shape[1]
    off = (float(d) - cross.double().pow(2).sum(-1)).to(torch.float32).contiguous()
    prior_sum = K.pairsum(pair, kind='imq', params=imq_scales(d)).sum().item()
    return cross, off, pair.shape[0], prior_sum


def _imq_prior(d, seed, dev):
    """_imq_prepare of imq_prior_samples(d, seed), cached per (d, seed, device)."""
    key = (d, seed, str(dev))
    if key not in _IMQ_PRIOR:
        cross, pair = imq_prior_samples(d, seed)
        _IMQ_PRIOR[key] = _imq_prepare(cross.to(dev).contiguous(), pair.to(dev).contiguous())
    return _IMQ_PRIOR[key]


@torch.no_grad()
def gaussian_imq_mmd_sq(x, prior_samples=None, seed=None):
    """math_utils.py:156-184: the MMD^2 estimate between the rows of x [N, Z] and N(0, I) averaged over seven inverse
    multiquadratic kernels s / (s + d2) of scales s = (0.1 .. 10) * 2Z, the prior represented by 1000 standardised
    samples. prior_samples: a tensor [n, Z] (used as it is in both prior terms) or a pair of tensors (cross-term
    samples, prior-prior samples); None: the two draws of imq_prior_samples(Z, seed), as the reference draws them,
    cached per (Z, seed) with the sum over the second set's own pairs. As in the reference the cross term uses
    |x|^2 - 2 x.p + Z in place of the squared distance (an offset Z - |p|^2 per sample), which can make
    s + that quantity small or negative for an unlucky sample. Returns a 0-dim f64 tensor on x's device."""
    x, n, d = _device_rows(x, 'gaussian_imq_mmd_sq')
    if prior_samples is None:
        p, off, n_pair, prior_sum = _imq_prior(d, seed, x.device)
    else:
        sets = prior_samples if isinstance(prior_samples, (tuple, list)) else (prior_samples, prior_samples)
        sets = [torch.as_tensor(t).to(x.device, torch.float32).contiguous() for t in sets]
        if len(sets) != 2 or any(t.dim() != 2 or t.shape[1] != d or t.shape[0] < 2 for t in sets):
            raise ValueError(f'gaussian_imq_mmd_sq: prior_samples must be [n >= 2, {d}] or a pair of such')
        p, off, n_pair, prior_sum = _imq_prepare(*sets)
    scales = imq_scales(d)
    x_sum = K.pairsum(x, kind='imq', params=scales).sum().item()
    cross = K.pairsum(x, p, kind='imq', params=scales, col_off=off).sum().item()
    return _scalar(imq_combine(n, p.shape[0], n_pair, x_sum, cross, prior_sum), x.device)
