"""Plain torch restatements of the optimiser and latent kernels of csrc/elementwise.hip (svae_sumsq, svae_clip_grad,
svae_radam, svae_reparam_kl_fwd / _bwd), the inputs the GPU tests feed them and the error bounds those tests hold
them to. Every formula takes a `dtype`: float64 is the reference, float32 the same formulas at the kernels' precision
(test_optim_ref.py measures the distance between the two; that distance is what the bounds are built from). The
tensors stay on the device they came on. Nothing in this file runs product code."""
import math

import torch

f64 = torch.float64


# ---------------------------------------------------------------------------------------------- error measure
ATOL_FRAC = 1.0


def deviation(got, ref, rows=False):
    """max over elements of |got - ref| / (atol + |ref|), atol = ATOL_FRAC * rms(ref): relative where the reference
    is of its typical size, absolute (in units of that size) where a signed sum cancels. One wrong element is one
    large term of the max: nothing is averaged. rows: the rms is taken per row of a 2-D tensor (rows of very
    different scale, as the KL gradient's 1 / ntok[b], are each held to their own size)."""
    got, ref = got.double(), ref.double()
    if not rows:
        got, ref = got.reshape(1, -1), ref.reshape(1, -1)
    atol = ATOL_FRAC * ref.pow(2).mean(-1, keepdim=True).sqrt()
    return ((got - ref).abs() / (atol + ref.abs())).max().item()


# ---------------------------------------------------------------------------------------------- norm and clip
def sumsq(g, dtype=f64):
    return g.to(dtype).pow(2).sum()


def clip_coef(norm, max_norm):
    """min(1, max_norm / (norm + 1e-6)), language_model.py:120-122 (torch's clip_grad_norm_); norm a 0-d tensor."""
    return torch.clamp(max_norm / (norm + 1e-6), max=1.0)


def clip(g, max_norm, dtype=f64):
    """-> (g * coef, norm), norm the 2-norm before the clip."""
    g = g.to(dtype)
    norm = sumsq(g, dtype).sqrt()
    return g * clip_coef(norm, max_norm), norm


# ---------------------------------------------------------------------------------------------- RAdam
LR, BETA1, BETA2, EPS, WD = 1e-2, 0.9, 0.999, 1e-6, 0.01


def radam_scalars(step, max_norm, lr=LR, b1=BETA1, b2=BETA2, eps=EPS, wd=WD):
    """The nine scalars of svae_radam for the 1-indexed `step` (rectified_adam.py:16-88, host arithmetic in Python
    floats): {lr_eff, bcm, bcv, rho_ok, beta1, beta2, eps, wd, max_norm}."""
    b2t = b2 ** step
    bcv = (1 - b2t) ** 0.5
    rho_inf = 2.0 / (1.0 - b2) - 1.0
    rho = rho_inf - 2 * step * b2t / (1 - b2t)
    lr_eff = lr
    if rho > 4:
        lr_eff = lr * ((((rho - 4.0) * (rho - 2.0) * rho_inf) / ((rho_inf - 4.0) * (rho_inf - 2.0) * rho)) ** 0.5 * bcv)
    return [lr_eff, 1 - b1 ** step, bcv, float(rho > 4), b1, b2, eps, wd, float(max_norm)]


def radam_step(p, m, v, g, scal, dtype=f64):
    """One fused clip + RAdam step from the nine scalars (a sequence of numbers: the GPU tests pass the f32 values
    the kernel reads, so beta rounding is no part of the comparison). -> (p, m, v, norm); nothing is updated in place.
      g' = g * min(1, max_norm / (|g| + 1e-6));  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g'^2
      p = p (1 - lr wd) - lr / bcm * (m / (sqrt(v) / bcv + eps)   if rho_ok else   m)"""
    lr, bcm, bcv, rho_ok, b1, b2, eps, wd, max_norm = (torch.tensor(float(s), dtype=dtype, device=p.device)
                                                       for s in scal)
    p, m, v = p.to(dtype), m.to(dtype), v.to(dtype)
    gc, norm = clip(g, max_norm, dtype)
    m = m * b1 + (1 - b1) * gc
    v = v * b2 + (1 - b2) * gc * gc
    p = p * (1 - lr * wd)
    if float(rho_ok) != 0.0:
        p = p - (lr / bcm) * (m / (v.sqrt() / bcv + eps))
    else:
        p = p - (lr / bcm) * m
    return p, m, v, norm


RADAM_SIZES = (4, 1020, 10000, 5_243_028)
RADAM_STEPS = {0: (2, 3, 4), 1: (5, 6, 7)}    # rho_ok -> consecutive steps (rho_t crosses 4 between steps 4 and 5)
G_SCALE = {True: 3.0, False: 0.1}             # clip active -> |g| = 3 max_norm; inactive -> |g| = max_norm / 10


def radam_case(n, clip_active, rho_ok, device='cpu'):
    """The RAdam tests' inputs: p ~ N(0, 1), non-zero moments m ~ 0.3 N(0, 1), v ~ 0.09 U(0, 1) + 1e-3, three
    gradients N(0, 1) scaled to the norm G_SCALE * max_norm, max_norm = sqrt(n) (elements of size G_SCALE at every n).
    -> (p, m, v, [g0, g1, g2], [scal0, scal1, scal2]) f32 tensors (drawn on the CPU: the same on every device)."""
    gen = torch.Generator().manual_seed(1000 + n % 997 + 2 * int(clip_active) + int(rho_ok))
    p = torch.randn(n, generator=gen)
    m = torch.randn(n, generator=gen) * 0.3
    v = torch.rand(n, generator=gen) * 0.09 + 1e-3
    gs = []
    for _ in range(3):
        g = torch.randn(n, generator=gen)
        gs.append((g * (G_SCALE[bool(clip_active)] * math.sqrt(n) / g.double().norm().item())).to(device))
    scals = [radam_scalars(s, math.sqrt(n)) for s in RADAM_STEPS[int(rho_ok)]]
    assert all(s[3] == float(rho_ok) for s in scals)
    return p.to(device), m.to(device), v.to(device), gs, [torch.tensor(s, dtype=torch.float32) for s in scals]


# ---------------------------------------------------------------------------------------------- reparameterise + KL
LOG2E = 1.4426950408889634


def _exp(x):
    """exp. In float32 it is written as the kernels write it, exp2(x * log2 e) (__expf on the hardware's exp2 unit):
    rounding the product to f32 moves the result by up to |x| 2^-24 relative, an error every f32 evaluation of this
    form has and torch's correctly rounded f32 exp has not; the f32-vs-f64 measurement has to contain it. In
    float64 the two forms agree to 1e-16."""
    return x.exp() if x.dtype == f64 else torch.exp2(x * LOG2E)


def reparam_kl(stats, eps, ntok, dtype=f64):
    """conditional_gaussian.py:18-28, continuous_autoencoder.py:42-52. stats [B, 2Z] = (mu | logvar), eps [B, Z],
    ntok [B]. -> z [B, Z], raw_kl [B], kl_out [2] = (mean_b raw_kl[b] / ntok[b], mean_b raw_kl[b])."""
    Z = stats.shape[1] // 2
    stats, eps = stats.to(dtype), eps.to(dtype)
    mu, lv = stats[:, :Z], stats[:, Z:]
    var = _exp(lv)
    z = mu + eps * var.sqrt()
    raw = (0.5 * (mu * mu + var - lv - 1.0)).sum(-1)
    return z, raw, torch.stack([(raw / ntok.to(dtype)).mean(), raw.mean()])


def reparam_kl_bwd(stats, eps, ntok, dz, gkl):
    """float64 autograd of reparam_kl: d/d stats of sum(z * dz) + gkl * kl_out[0] (dz None: the KL term alone)."""
    s = stats.double().clone().requires_grad_()
    z, _, kl = reparam_kl(s, eps, ntok)
    loss = kl[0] * float(gkl)
    if dz is not None:
        loss = loss + (z * dz.double()).sum()
    loss.backward()
    return s.grad


REPARAM_SHAPES = ((1, 4), (5, 64), (16, 32), (17, 32), (64, 64), (64, 128), (65, 96), (130, 256), (130, 96))
LOGVAR_RANGE = (-6.0, 3.0)


def reparam_case(B, Z, wide, device='cpu'):
    """The reparam tests' inputs: mu ~ N(0, 1); logvar uniform over LOGVAR_RANGE (`wide`) or 0.5 N(0, 1); eps and
    dz ~ N(0, 1); ntok differs per row and starts at 1. -> (stats, eps, ntok, dz)."""
    gen = torch.Generator().manual_seed(7000 + 131 * B + Z + int(wide))
    mu = torch.randn(B, Z, generator=gen)
    if wide:
        lv = torch.rand(B, Z, generator=gen) * (LOGVAR_RANGE[1] - LOGVAR_RANGE[0]) + LOGVAR_RANGE[0]
    else:
        lv = torch.randn(B, Z, generator=gen) * 0.5
    eps, dz = torch.randn(B, Z, generator=gen), torch.randn(B, Z, generator=gen)
    ntok = 1 + 7 * torch.arange(B, dtype=torch.int64)
    return torch.cat([mu, lv], 1).contiguous().to(device), eps.to(device), ntok.to(device), dz.to(device)


def reparam_bwd_f32(stats, eps, ntok, dz, gkl):
    """The backward's closed form in float32 (what the f32-vs-f64 measurement evaluates; the reference is autograd)."""
    Z = stats.shape[1] // 2
    mu, lv = stats[:, :Z].float(), stats[:, Z:].float()
    var = _exp(lv)
    w = (torch.tensor(float(gkl), dtype=torch.float32, device=stats.device)
         / (torch.tensor(float(stats.shape[0]), dtype=torch.float32, device=stats.device) * ntok.float()))[:, None]
    g = dz.float() if dz is not None else torch.zeros_like(mu)
    return torch.cat([g + w * mu, g * eps.float() * var.sqrt() * 0.5 + w * 0.5 * (var - 1.0)], 1)


# ---------------------------------------------------------------------------------------------- recorded deviations
# Largest deviation() of the float32 evaluation of the formulas above from the float64 one, measured on the CPU by
# test_optim_ref.py (which re-measures them and fails if one has moved by more than a quarter; the f32 sum of
# squares is summed in whatever order the host's torch build takes, so the last digit may differ between machines):
#   RAdam: over radam_case(n, clip, rho_ok) for every n of RADAM_SIZES, both clip states, both rho_ok, after each of
#          the three steps (the f32 run carries its own f32 state from step to step, as the kernel does);
#   reparam: over reparam_case(B, Z, wide) for every shape of REPARAM_SHAPES and both logvar distributions.
# The GPU bound is TOL_FACTOR times the constant: the kernels evaluate the same formulas in another, equally valid
# order (fused multiply-adds, a tree-ordered norm). Beside each: the largest value seen from the kernels on an MI355X.
TOL_FACTOR = 4.0
F32_DEV_P = 2.4e-7        # kernels on an MI355X: 2.4e-7 (bound 9.60e-07)
F32_DEV_M = 3.8e-7        # kernels on an MI355X: 2.4e-7 (bound 1.52e-06)
F32_DEV_V = 1.7e-7        # kernels on an MI355X: 9.6e-8 (bound 6.80e-07)
F32_DEV_Z = 1.9e-7        # kernels on an MI355X: 1.7e-7 (bound 7.60e-07)
F32_DEV_RAW_KL = 8.1e-8   # kernels on an MI355X: 8.2e-8 (bound 3.24e-07)
F32_DEV_KL = 9.7e-8       # kernels on an MI355X: 1.5e-7 (bound 3.88e-07)
F32_DEV_DSTATS = 3.0e-7   # kernels on an MI355X: 3.0e-7 (bound 1.20e-06)


def radam_bound(dev):
    return TOL_FACTOR * dev


def reparam_bound(dev):
    return TOL_FACTOR * dev
