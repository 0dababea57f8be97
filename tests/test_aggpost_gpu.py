"""The aggregate-posterior kernels (csrc/aggpost.hip), LatentIndex.log_density / .elbo_surgery and elbo_surgery.py on the
device, against the float64 restatement of tests/aggpost_ref.py. Every output is held, row by row, within the bound
aggpost_ref.py derives from the orders the kernel states; the worst error / bound of each case is printed. Outputs are
views into sentinel-filled buffers (tests/sentinels.py), and two runs must agree bit for bit."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import aggpost_ref as R
import sentinels as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def gpu(a, dtype=None):
    if a is None:
        return None
    t = torch.from_numpy(np.array(a))              # a copy: the cached cases are read-only
    return (t if dtype is None else t.to(dtype)).cuda()


def kernels():
    from sparse_vae import kernels as K
    return K


def run_logq(z, loc, scale, skip, per_dim):
    """One guarded launch -> (logq f64 [M], logq_dim f64 [M, Z] or None) as numpy, and the raw device tensors."""
    K = kernels()
    M, Z = z.shape
    zt, lt, st, kt = gpu(z), gpu(loc), gpu(scale), gpu(skip)
    fq, vq = S.flat(M)
    fd, vd = S.flat(M * Z) if per_dim else (None, None)
    K.aggpost_logq(zt, lt, st, skip=kt, logq=vq, logq_dim=vd)
    torch.cuda.synchronize()
    assert S.intact(fq) and (fd is None or S.intact(fd))
    return vq, (vd.view(M, Z) if per_dim else None)


def check_logq(z, loc, scale, skip=None, per_dim=True, what=''):
    want = R.logq(z, loc, scale, skip, per_dim=per_dim)
    q1, d1 = run_logq(z, loc, scale, skip, per_dim)
    q2, d2 = run_logq(z, loc, scale, skip, per_dim)
    assert torch.equal(q1, q2) and (not per_dim or torch.equal(d1, d2))               # bit for bit
    got = q1.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    over = np.abs(got - want['logq']) / want['logq_err']
    print(f'{what}logq: worst error / bound {over.max():.3f}')
    assert (over <= 1).all(), (over.max(), int(over.argmax()))
    if per_dim:
        gd = d1.cpu().numpy().astype(np.float64)
        assert np.isfinite(gd).all()
        over = np.abs(gd - want['logq_dim']) / want['logq_dim_err']
        print(f'{what}logq_dim: worst error / bound {over.max():.3f}')
        assert (over <= 1).all(), (over.max(), int(over.argmax()))
    return q1, d1, want


def test_geometry_of_the_cases():
    """Each size hits the boundary it is named for, read from the library's own geometry."""
    from sparse_vae import _native
    K = kernels()
    assert (_native.AGGPOST_POINTS_PER_BLOCK, _native.AGGPOST_TILE_ROWS, _native.AGGPOST_PASS_DIMS) == \
        (R.POINTS_PER_BLOCK, R.TILE_ROWS, R.PASS_DIMS)
    shapes = R.shapes()
    for Z in R.ZS:
        P, _, _, rps, T, _ = K.aggpost_geometry(65, 65, Z, True)
        assert (P, T, rps) == (R.POINTS_PER_BLOCK, R.TILE_ROWS, R.MIN_SLICE_ROWS)
        ms = {m for m, n, z in shapes if z == Z}
        ns = {n for m, n, z in shapes if z == Z}
        assert {1, 63, 65, P + 1} <= ms and {1, 2, T - 1, T + 1, rps + 1, 2 * rps + 1} <= ns
        for per_dim in (False, True):
            assert K.aggpost_geometry(P, 8, Z, per_dim)[1] == 1 and K.aggpost_geometry(P + 1, 8, Z, per_dim)[1] == 2
            g = K.aggpost_geometry(65, rps + 1, Z, per_dim)
            assert g[2] == 2 and g[3] == rps                        # one row in the last slice
            assert K.aggpost_geometry(65, 2 * rps + 1, Z, per_dim)[2] == 3
            assert K.aggpost_geometry(65, rps, Z, per_dim)[2] == 1
        held = K.aggpost_geometry(65, 65, Z, True)[5]
        assert held == min(Z, R.PASS_DIMS) and K.aggpost_geometry(65, 65, Z, False)[5] == Z
        if Z in (68, 256):
            assert held < Z and -(-Z // held) > 1                   # more than one dimension pass
            if Z == 68:
                assert Z % held                                     # and a last pass that is not full
    for m, n, z in shapes:
        assert K.aggpost_geometry(m, n, z, True) == R.geometry(m, n, z, True)


@pytest.mark.parametrize('per_dim', [False, True])
@pytest.mark.parametrize('M,N,Z', R.shapes())
def test_logq_within_the_derived_bounds(M, N, Z, per_dim):
    z, src, loc, scale = R.case(M, N, Z, 'vae')
    check_logq(z, loc, scale, None, per_dim, what=f'M={M} N={N} Z={Z} ')


@pytest.mark.parametrize('M,N,Z', [(65, 2, 4), (65, R.MIN_SLICE_ROWS + 1, 64), (R.POINTS_PER_BLOCK + 1, 130, 68)])
def test_skip_minus_one_is_no_skip(M, N, Z):
    z, src, loc, scale = R.case(M, N, Z, 'vae')
    a_q, a_d = run_logq(z, loc, scale, None, True)
    b_q, b_d = run_logq(z, loc, scale, np.full(M, -1, np.int32), True)
    assert torch.equal(a_q, b_q) and torch.equal(a_d, b_d)


def test_separated_rows_report_the_cap():
    """loc_j0 = 64 j, scale 1: the inclusive estimate can only report log N. Nothing underflows into a NaN."""
    K = kernels()
    N, Z = 2 * R.MIN_SLICE_ROWS + 1, 8
    z, src, loc, scale = R.case(N, N, Z, 'separated')
    q, d, want = check_logq(z, loc, scale, None, True, what='separated ')
    out = K.aggpost_decompose(gpu(z), gpu(src), gpu(loc), gpu(scale), q.contiguous(), d.contiguous()).cpu().numpy()
    assert np.isfinite(out).all()
    ref = R.surgery(loc, scale, src, z)
    assert abs(ref['out'][0] - math.log(N)) <= 1e-12
    allow = want['logq_err'].mean() + 1e-12
    print(f'separated mi - log N: {out[0] - math.log(N):.3e} (bound {allow:.3e})')
    assert abs(out[0] - math.log(N)) <= allow


@pytest.mark.parametrize('Z', [4, 68])
def test_extreme_scales_in_one_index(Z):
    """Scales from 1e-4 to 1e2 in one index: terms down to -1e9 beside terms of order 1, outputs finite and in bound."""
    M, N = 65, 2 * R.MIN_SLICE_ROWS + 1
    z, src, loc, scale = R.case(M, N, Z, 'extreme')
    assert scale.min() < 1e-3 and scale.max() > 10
    check_logq(z, loc, scale, None, True, what=f'extreme Z={Z} ')
    check_logq(z, loc, scale, src, True, what=f'extreme leave-one-out Z={Z} ')


@pytest.mark.parametrize('Z', [4, 64, 68])
def test_leave_one_out(Z):
    M, N = R.POINTS_PER_BLOCK + 1, R.MIN_SLICE_ROWS + 1
    z, src, loc, scale = R.case(M, N, Z, 'vae')
    q, d, want = check_logq(z, loc, scale, src, True, what=f'leave-one-out Z={Z} ')
    inc = R.logq(z, loc, scale, None)['logq']
    assert (want['logq'] + math.log(N - 1) < inc + math.log(N)).all()
    # every point skips the only row of the last slice: that slice leaves (-inf, 0) for all of them
    skip = np.full(M, N - 1, np.int32)
    assert kernels().aggpost_geometry(M, N, Z, True)[2:4] == (2, N - 1)
    check_logq(z, loc, scale, skip, True, what=f'skip the last slice Z={Z} ')
    # and a mixture of points that skip it and points that skip nothing
    skip = np.where(np.arange(M) % 3 == 0, N - 1, -1).astype(np.int32)
    check_logq(z, loc, scale, skip, True, what=f'skip the last slice, every third point Z={Z} ')


def test_leave_one_out_with_two_rows():
    z, src, loc, scale = R.case(65, 2, 8, 'vae')
    q, d, want = check_logq(z, loc, scale, src, True, what='two rows ')
    other = R.logq(z[:1], loc[1:], scale[1:], None)['logq']             # point 0 skips row 0: the density is row 1's
    assert abs(want['logq'][0] - other[0]) <= 1e-12


def test_skip_with_one_row_is_refused():
    from sparse_vae import _native
    K = kernels()
    z, src, loc, scale = R.case(5, 1, 4, 'vae')
    zt, lt, st, kt = gpu(z), gpu(loc), gpu(scale), gpu(src)
    with pytest.raises(ValueError, match='two rows'):
        K.aggpost_logq(zt, lt, st, skip=kt)
    fq, vq = S.flat(5)
    ws = torch.full((64,), S.SENTINEL, dtype=torch.float64, device='cuda')
    rc = _native.lib.svae_aggpost_logq(zt.data_ptr(), 5, lt.data_ptr(), st.data_ptr(), 1, 4, kt.data_ptr(),
                                       vq.data_ptr(), None, ws.data_ptr(), ws.numel() * 8, None)
    torch.cuda.synchronize()
    assert rc == 1 and bool((fq == S.SENTINEL).all()) and bool((ws == S.SENTINEL).all())


def test_refused_shapes_write_nothing():
    from sparse_vae import _native
    lib = _native.lib
    M, N, Z = 8, 8, 8
    z, src, loc, scale = R.case(M, N, Z, 'vae')
    zt, lt, st, kt = gpu(z), gpu(loc), gpu(scale), gpu(src)
    fq, vq = S.flat(M)
    fd, vd = S.flat(M * Z)
    out = torch.full((4 + Z,), S.SENTINEL, dtype=torch.float64, device='cuda')
    ws = torch.full((4096,), S.SENTINEL, dtype=torch.float64, device='cuda')
    need = lib.svae_aggpost_ws_bytes(M, N, Z, 1)
    assert 0 < need <= ws.numel() * 8

    def logq(M=M, N=N, Z=Z, ws_bytes=ws.numel() * 8, z=zt.data_ptr(), skip=None):
        return lib.svae_aggpost_logq(z, M, lt.data_ptr(), st.data_ptr(), N, Z, skip, vq.data_ptr(), vd.data_ptr(),
                                     ws.data_ptr(), ws_bytes, None)

    for bad in (dict(M=0), dict(N=0), dict(Z=6), dict(Z=260), dict(ws_bytes=need - 1), dict(z=zt.data_ptr() + 4),
                dict(z=None), dict(N=1, skip=kt.data_ptr())):
        assert logq(**bad) == 1, bad
    dbytes = lib.svae_aggpost_decompose_ws_bytes(M, Z)
    for bad in (dict(M=0), dict(Z=6), dict(ws_bytes=dbytes - 1)):
        a = dict(M=M, Z=Z, ws_bytes=ws.numel() * 8)
        a.update(bad)
        assert lib.svae_aggpost_decompose(zt.data_ptr(), kt.data_ptr(), lt.data_ptr(), st.data_ptr(), vq.data_ptr(),
                                          vd.data_ptr(), a['M'], a['Z'], ws.data_ptr(), a['ws_bytes'], out.data_ptr(),
                                          None) == 1, bad
    torch.cuda.synchronize()
    for t in (fq, fd, out, ws):
        assert bool((t == S.SENTINEL).all())


@pytest.mark.parametrize('M,N,Z', [(1, 1, 4), (65, 17, 64), (R.POINTS_PER_BLOCK + 1, 65, 68), (600, 40, 256)])
def test_decompose_follows_the_reference(M, N, Z):
    """svae_aggpost_decompose on the device's own logq and logq_dim against the f64 restatement on the same values, and
    the identity marginal_kl = tc + sum_d dim_kl on the device's outputs."""
    K = kernels()
    z, src, loc, scale = R.case(M, N, Z, 'vae')
    q, d = run_logq(z, loc, scale, None, True)
    q, d = q.contiguous(), d.contiguous()
    full = torch.full((4 + Z + S.GUARD,), S.SENTINEL, dtype=torch.float64, device='cuda')
    args = (gpu(z), gpu(src), gpu(loc), gpu(scale), q, d)
    out = K.aggpost_decompose(*args, out=full[:4 + Z])
    again = K.aggpost_decompose(*args)
    torch.cuda.synchronize()
    assert S.intact(full) and torch.equal(out, again)
    got = out.cpu().numpy()
    lq, lqd = q.cpu().numpy(), d.cpu().numpy()
    want = R.decompose(z, src, loc, scale, lq, lqd)
    bound = R.dec_bound(z, src, loc, scale, lq, lqd)
    over = np.abs(got - want) / bound
    print(f'M={M} N={N} Z={Z} decompose: worst error / bound {over.max():.3f}')
    assert (over <= 1).all(), (over.max(), int(over.argmax()))
    assert got[3] == got[0] + got[1]
    assert abs(got[1] - (got[2] + got[4:].sum())) <= bound[1] + bound[2] + bound[4:].sum()
    if N == 1:             # one row: log q(z) is log q(z|x), to the rounding of the device's logq
        assert abs(got[0]) <= bound[0] + R.logq(z, loc, scale)['logq_err'].mean()


def test_decompose_clamps_device_rows_and_refuses_cpu_rows_outside():
    K = kernels()
    z, src, loc, scale = R.case(8, 5, 4, 'vae')
    q, d = run_logq(z, loc, scale, None, True)
    args = (gpu(z), gpu(loc), gpu(scale), q.contiguous(), d.contiguous())
    with pytest.raises(IndexError):
        K.aggpost_decompose(args[0], torch.full((8,), 5, dtype=torch.int64), *args[1:])
    a = K.aggpost_decompose(args[0], torch.full((8,), 99, dtype=torch.int64, device='cuda'), *args[1:])
    b = K.aggpost_decompose(args[0], torch.full((8,), 4, dtype=torch.int32), *args[1:])
    assert torch.equal(a, b)


@pytest.mark.parametrize('loo', [False, True])
def test_elbo_surgery_end_to_end(loo):
    """LatentIndex.elbo_surgery with injected eps against the reference: the draws are svae_latent_draw's (checked
    against the f64 fmaf), the rows a seeded subset, the terms within the bounds their inputs' bounds imply."""
    from sparse_vae import ElboSurgery, LatentIndex
    from sparse_vae.surgery import sample_rows
    K = kernels()
    N, Z, M = 300, 8, 100
    _, _, loc, scale = R.case(1, N, Z, 'vae', seed=5)
    index = LatentIndex(Z, device='cuda').add(gpu(loc), gpu(scale))
    rows = sample_rows(N, M, seed=11)
    eps = np.clip(np.random.default_rng(2).standard_normal((M, Z)), -4, 4).astype(np.float32)
    s = index.elbo_surgery(samples=M, seed=11, leave_one_out=loo, eps=torch.from_numpy(eps))
    assert isinstance(s, ElboSurgery) and torch.equal(s.rows, rows) and s.samples == M and s.seed == 11
    assert s.leave_one_out is loo and s.dim_kl.dtype == torch.float64 and tuple(s.dim_kl.shape) == (Z,)
    r = rows.numpy()
    z = K.latent_draw(gpu(loc[r]), gpu(scale[r]), seed=11, eps=gpu(eps)).cpu().numpy()
    assert np.array_equal(z, R.draw(loc[r], scale[r], eps))
    want = R.surgery(loc, scale, r, z, leave_one_out=loo)
    out = want['out']
    eq, ed = want['logq_err'].mean(), want['logq_dim_err'].sum(axis=1).mean()
    slack = 1e-12 * (1 + np.abs(out).max())
    for name, got, ref, allow in (('mutual_info', s.mutual_info, out[0], eq), ('marginal_kl', s.marginal_kl, out[1], eq),
                                  ('total_correlation', s.total_correlation, out[2], eq + ed),
                                  ('kl_mc', s.kl_mc, out[3], 0.0)):
        print(f'{name}: {got:.9g} against {ref:.9g}, error / bound {abs(got - ref) / (allow + slack):.3f}')
        assert abs(got - ref) <= allow + slack, name
    dk = s.dim_kl.cpu().numpy()
    assert (np.abs(dk - out[4:]) <= want['logq_dim_err'].mean(axis=0) + slack).all()
    assert abs(s.kl_analytic - want['kl_analytic']) <= 1e-9 * (1 + abs(want['kl_analytic']))
    assert s.mi_cap == want['mi_cap'] == math.log(N - 1 if loo else N)
    lq = index.log_density(torch.from_numpy(z), skip=torch.from_numpy(r) if loo else None)
    assert (np.abs(lq.cpu().numpy() - want['logq']) <= want['logq_err']).all()
    if not loo:
        assert s.mutual_info <= s.mi_cap + eq
        full = index.elbo_surgery(seed=3)
        assert full.samples == N and torch.equal(full.rows, torch.arange(N))
        assert torch.equal(index.elbo_surgery(samples=N + 5, seed=3).dim_kl, full.dim_kl)


def test_script_matches_its_json(tmp_path):
    """elbo_surgery.py in a child process on a small saved index: what it prints is what it writes, and what it writes
    is what the library returns."""
    from sparse_vae import LatentIndex
    N, Z = 200, 8
    _, _, loc, scale = R.case(1, N, Z, 'vae', seed=9)
    index = LatentIndex(Z, device='cuda').add(gpu(loc), gpu(scale))
    path, js = str(tmp_path / 'latents.npz'), str(tmp_path / 'out.json')
    index.save(path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'elbo_surgery.py'), path, '--samples', '64', '--seed', '4',
                        '--leave-one-out', '--json', js], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    rep = json.load(open(js))
    inc, loo = rep['inclusive'], rep['leave_one_out']
    for name, leave in (('inclusive', False), ('leave_one_out', True)):
        s = index.elbo_surgery(samples=64, seed=4, leave_one_out=leave)
        d = rep[name]
        assert (d['mutual_info'], d['marginal_kl'], d['total_correlation'], d['kl_mc'], d['kl_analytic']) == \
            (s.mutual_info, s.marginal_kl, s.total_correlation, s.kl_mc, s.kl_analytic)
        assert d['dim_kl'] == s.dim_kl.cpu().tolist() and d['samples'] == 64 and d['leave_one_out'] is leave
    assert inc['mutual_info'] < loo['mutual_info'] and inc['kl_mc'] == pytest.approx(loo['kl_mc'], abs=1e-9)
    text = r.stdout
    assert f'{N} posteriors of {Z} dimensions, 64 samples (seed 4)' in text
    assert f"analytic {inc['kl_analytic']:.6g} nats, Monte Carlo {inc['kl_mc']:.6g} nats" in text
    assert f"mutual information I_q(x; z): {inc['mutual_info']:.6g} nats (cap {math.log(N):.6g})" in text
    assert f"mutual information I_q(x; z): {loo['mutual_info']:.6g} nats (cap {math.log(N - 1):.6g})" in text
    assert f"total correlation:            {inc['total_correlation']:.6g} nats" in text
    assert ('saturated' in text) == (inc['saturated'] or loo['saturated'])
    lines = [ln for ln in text.splitlines() if ln.startswith('  dim ')]
    order = sorted(range(Z), key=lambda k: -inc['dim_kl'][k])
    assert [int(ln.split()[1]) for ln in lines] == order
    assert f"mean kl {rep['mean_kl'][order[0]]:.6g}" in lines[0]
