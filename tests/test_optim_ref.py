"""CPU checks of tests/optim_ref.py, the float64 restatements the optimiser / latent kernel GPU tests compare against:

* the clip and the RAdam step against oracle.clip_grad_norm / oracle.radam_step (themselves pinned to the reference's
  goldens) over 12 steps from zero moments, which spans the step at which rho_t crosses 4;
* reparameterise + KL against torch.distributions, its autograd backward against the closed form;
* the recorded f32-vs-f64 deviations (optim_ref.F32_DEV_*): re-measured here on the GPU tests' own inputs; each
  constant has to lie within a quarter of its measurement.
"""
import functools
import math

import pytest
import torch

import oracle
import optim_ref as R


def test_clip_matches_oracle():
    g = torch.randn(1000, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    for max_norm, active in ((10.0, True), (100.0, False)):
        total, (gc,) = oracle.clip_grad_norm([g], max_norm)
        got, norm = R.clip(g, max_norm)
        assert (norm.item() > max_norm) == active
        assert abs(norm.item() - total.item()) < 1e-12 * total.item()
        assert torch.allclose(got, gc, rtol=1e-14, atol=0)
        if not active:
            assert torch.equal(got, g)


def test_radam_step_matches_oracle_across_the_rectification_threshold():
    gen = torch.Generator().manual_seed(2)
    n, max_norm = 500, 30.0
    p = torch.randn(n, generator=gen, dtype=torch.float64)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    st = oracle.RAdamState()
    ref = {'p': p.clone()}
    flags = []
    for step in range(1, 13):
        g = torch.randn(n, generator=gen, dtype=torch.float64) * (3.0 if step % 2 else 0.3)   # clip on / off
        total, (gc,) = oracle.clip_grad_norm([g], max_norm)
        assert st.step == step
        ref = oracle.radam_step(ref, {'p': gc}, st, lr=R.LR, betas=(R.BETA1, R.BETA2), eps=R.EPS, weight_decay=R.WD)
        scal = R.radam_scalars(step, max_norm)
        flags.append(scal[3])
        p, m, v, norm = R.radam_step(p, m, v, g, scal)
        assert abs(norm.item() - total.item()) < 1e-12 * total.item()
        for got, want in ((p, ref['p']), (m, st.exp_avg['p']), (v, st.exp_avg_sq['p'])):
            assert torch.allclose(got, want, rtol=1e-12, atol=1e-15), step
    assert flags == [0.0] * 4 + [1.0] * 8          # both branches, the switch between steps 4 and 5
    assert {k: tuple(R.radam_scalars(s, 1.0)[3] for s in v) for k, v in R.RADAM_STEPS.items()} == \
        {0: (0.0, 0.0, 0.0), 1: (1.0, 1.0, 1.0)}


def test_reparam_kl_matches_torch_distributions():
    from torch.distributions import Normal, kl_divergence
    stats, eps, ntok, dz = R.reparam_case(17, 32, True)
    z, raw, kl = R.reparam_kl(stats, eps, ntok)
    mu, lv = stats[:, :32].double(), stats[:, 32:].double()
    q = Normal(mu, (0.5 * lv).exp())
    want = kl_divergence(q, Normal(torch.zeros_like(mu), torch.ones_like(mu))).sum(-1)
    assert torch.allclose(raw, want, rtol=1e-12)
    assert torch.allclose(z, mu + eps.double() * q.scale, rtol=1e-13, atol=1e-15)
    assert abs(kl[0].item() - (want / ntok).mean().item()) < 1e-12 and abs(kl[1].item() - want.mean().item()) < 1e-12
    assert ntok[0].item() == 1 and ntok.unique().numel() == 17
    assert stats[:, 32:].min().item() < -5 and stats[:, 32:].max().item() > 2
    for d in (dz, None):                          # the autograd backward against the closed form
        got = R.reparam_kl_bwd(stats, eps, ntok, d, 0.7)
        w = 0.7 / (17 * ntok.double())[:, None]
        g = d.double() if d is not None else torch.zeros_like(mu)
        want = torch.cat([g + w * mu, g * eps.double() * q.scale * 0.5 + w * 0.5 * (lv.exp() - 1)], 1)
        assert torch.allclose(got, want, rtol=1e-12, atol=1e-15)
        assert R.deviation(R.reparam_bwd_f32(stats, eps, ntok, d, 0.7), got) < 1e-4


# ------------------------------------------------------------------------------------------ the recorded deviations
@functools.lru_cache(maxsize=None)
def measured_radam():
    worst = {'p': 0.0, 'm': 0.0, 'v': 0.0}
    for n in R.RADAM_SIZES:
        for clip_active in (True, False):
            for rho_ok in (0, 1):
                p, m, v, gs, scals = R.radam_case(n, clip_active, rho_ok)
                lo, hi = (p, m, v), (p, m, v)
                for g, scal in zip(gs, scals):
                    s = scal.double().tolist()               # the f32 values the kernel reads, for both
                    lo = R.radam_step(*lo, g, s, torch.float32)[:3]
                    hi = R.radam_step(*hi, g, s)[:3]
                    for k, a, b in zip('pmv', lo, hi):
                        worst[k] = max(worst[k], R.deviation(a, b))
    return worst


@functools.lru_cache(maxsize=None)
def measured_reparam():
    worst = {'z': 0.0, 'raw_kl': 0.0, 'kl': 0.0, 'dstats': 0.0}
    for B, Z in R.REPARAM_SHAPES:
        for wide in (True, False):
            stats, eps, ntok, dz = R.reparam_case(B, Z, wide)
            lo, hi = R.reparam_kl(stats, eps, ntok, torch.float32), R.reparam_kl(stats, eps, ntok)
            for k, a, b in (('z', lo[0], hi[0]), ('raw_kl', lo[1], hi[1]), ('kl', lo[2][:1], hi[2][:1]),
                            ('kl', lo[2][1:], hi[2][1:])):      # the two entries of kl_out each on their own scale
                worst[k] = max(worst[k], R.deviation(a, b))
            for d in (dz, None):
                worst['dstats'] = max(worst['dstats'], R.deviation(R.reparam_bwd_f32(stats, eps, ntok, d, 0.7),
                                                                   R.reparam_kl_bwd(stats, eps, ntok, d, 0.7), rows=True))
    return worst


def _recorded(const, measured, what):
    print(f'{what}: measured f32-vs-f64 deviation {measured:.3e}, recorded {const:.3e}')
    assert abs(measured / const - 1.0) <= 0.25, (what, measured, const)


@pytest.mark.parametrize('key,const', [('p', 'F32_DEV_P'), ('m', 'F32_DEV_M'), ('v', 'F32_DEV_V')])
def test_recorded_radam_deviation_is_the_measurement(key, const):
    _recorded(getattr(R, const), measured_radam()[key], const)


@pytest.mark.parametrize('key,const', [('z', 'F32_DEV_Z'), ('raw_kl', 'F32_DEV_RAW_KL'), ('kl', 'F32_DEV_KL'),
                                       ('dstats', 'F32_DEV_DSTATS')])
def test_recorded_reparam_deviation_is_the_measurement(key, const):
    _recorded(getattr(R, const), measured_reparam()[key], const)


def test_deviation_sees_one_wrong_element():
    ref = torch.randn(100000, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    got = ref.float()
    assert R.deviation(got, ref) < 2.0 ** -24
    got[77777] += 1e-3
    assert R.deviation(got, ref) > 1e-4
    assert math.isclose(R.radam_bound(1e-7), 4e-7) and math.isclose(R.reparam_bound(1e-7), 4e-7)
