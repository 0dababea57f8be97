"""ELBO surgery of a latent index (Hoffman & Johnson 2016): the mean KL term of the ELBO split into what it says about
the document and what is mismatch with the prior,

    E_x KL(q(z|x) || p(z)) = I_q(x; z) + KL(q(z) || p(z)),

with q(z) = (1 / N) sum_j q(z | x_j) the aggregate posterior, and the marginal term split again (Chen et al. 2018) into a
total correlation and per-dimension KLs, KL(q(z) || p(z)) = TC + sum_d KL(q(z_d) || p(z_d)).

Training logs the same split estimated inside one batch (marginal_kl, math_utils.py:51-58 of the reference), which
cannot exceed log B. Here q(z) is the exact N-component mixture over the whole index, evaluated by libsvae's
svae_aggpost_logq (csrc/aggpost.hip) at one draw z_i ~ q(z | x_i) per sampled row; svae_aggpost_decompose forms the
means. There is no CPU fallback."""
import math
from dataclasses import dataclass

import torch

from . import kernels as K


@dataclass
class ElboSurgery:
    """The terms, in nats per document, as Monte-Carlo means over `samples` draws z_i ~ q(z | x_rows[i]):

    mutual_info        mean_i(log q(z_i | x_i) - log q(z_i)), the index-code mutual information I_q(x; z)
    marginal_kl        mean_i(log q(z_i) - log p(z_i)) = KL(q(z) || p(z)), p = N(0, I)
    total_correlation  mean_i(log q(z_i) - sum_d log q(z_id))
    dim_kl             f64 [Z] on the device: mean_i(log q(z_id) - log p(z_id)); marginal_kl = total_correlation +
                       dim_kl.sum() to f64 rounding
    kl_mc              mutual_info + marginal_kl: the Monte-Carlo estimate of the mean KL, to be read against
    kl_analytic        the closed-form mean KL of the same rows (LatentIndex.stats()['kl'] restricted to `rows`)
    mi_cap             log N (log(N - 1) with leave_one_out): no estimate of this kind can exceed it

    Which way each variant is biased. q(z_i) is estimated from the N rows of the index, and z_i was drawn from one of
    them. The inclusive estimate (leave_one_out=False) counts the point's own component, whose density at z_i is high
    because z_i came from it: it overstates q(z_i), so mutual_info is biased LOW (and is capped at log N: a model
    whose posteriors do not overlap reports exactly the cap, and then more rows are needed, not a better model) and
    marginal_kl HIGH. The leave-one-out estimate drops that component and divides by N - 1: it understates q(z_i)
    wherever a held-out document would have put mass near z_i, so mutual_info is biased HIGH and marginal_kl LOW. The
    two bracket the quantity. log q(z_i) cancels in kl_mc = mean_i(log q(z_i | x_i) - log p(z_i)), so kl_mc is the same
    for both variants and differs from kl_analytic by Monte-Carlo noise alone."""
    mutual_info: float
    marginal_kl: float
    total_correlation: float
    dim_kl: torch.Tensor
    kl_mc: float
    kl_analytic: float
    mi_cap: float
    rows: torch.Tensor
    samples: int
    seed: int
    leave_one_out: bool

    @property
    def saturated(self):
        """mutual_info within 1 % of its cap: the estimate reports the size of the index, not the model."""
        return self.mutual_info >= 0.99 * self.mi_cap if self.mi_cap > 0 else True

    def to_dict(self):
        return {'mutual_info': self.mutual_info, 'marginal_kl': self.marginal_kl,
                'total_correlation': self.total_correlation, 'dim_kl': self.dim_kl.detach().cpu().tolist(),
                'kl_mc': self.kl_mc, 'kl_analytic': self.kl_analytic, 'mi_cap': self.mi_cap,
                'rows': int(self.rows.numel()), 'samples': self.samples, 'seed': self.seed,
                'leave_one_out': self.leave_one_out, 'saturated': bool(self.saturated)}


def sample_rows(n, samples=None, seed=0):
    """The rows a surgery draws from: all n (samples None or >= n), else a sorted subset of `samples` rows from a seeded
    torch.randperm on a CPU generator, so the choice does not depend on the device's RNG. -> int64 [samples] on the CPU."""
    if samples is None or samples >= n:
        return torch.arange(n, dtype=torch.int64)
    if samples < 1:
        raise ValueError(f'elbo_surgery: samples must be positive, got {samples}')
    g = torch.Generator(device='cpu')
    g.manual_seed(int(seed))
    return torch.randperm(n, generator=g)[:samples].sort().values


def elbo_surgery(loc, scale, samples=None, seed=0, leave_one_out=False, eps=None, rows=None):
    """The surgery of the index rows loc, scale f32 [N, Z] (device tensors): see LatentIndex.elbo_surgery."""
    n, Z = loc.shape
    if leave_one_out and n < 2:
        raise ValueError('elbo_surgery: leave_one_out needs at least two rows')
    if rows is None:
        rows = sample_rows(n, samples, seed)
    else:
        rows = torch.as_tensor(rows, dtype=torch.int64).reshape(-1).cpu()
        if rows.numel() == 0 or not (0 <= int(rows.min()) and int(rows.max()) < n):
            raise IndexError(f'elbo_surgery: rows outside the index (0..{n - 1})')
    dev = loc.device
    src = rows.to(dev)
    full = rows.numel() == n and bool((rows == torch.arange(n)).all())
    rl, rs = (loc, scale) if full else (loc[src].contiguous(), scale[src].contiguous())
    if eps is not None:
        eps = eps.to(dev, torch.float32).contiguous()
    z = K.latent_draw(rl, rs, seed=seed, eps=eps)
    src32 = src.to(torch.int32)
    logq, logq_dim = K.aggpost_logq(z, loc, scale, skip=src32 if leave_one_out else None, per_dim=True)
    out = K.aggpost_decompose(z, src32, loc, scale, logq, logq_dim)
    _, _, mean_kl = K.latent_colstats(rl, rs)
    head = out[:4].tolist()
    return ElboSurgery(mutual_info=head[0], marginal_kl=head[1], total_correlation=head[2], dim_kl=out[4:].clone(),
                       kl_mc=head[3], kl_analytic=float(mean_kl.sum().item()),
                       mi_cap=math.log(n - 1 if leave_one_out else n), rows=rows, samples=int(rows.numel()),
                       seed=int(seed), leave_one_out=bool(leave_one_out))
