"""The LayerNorm kernels of csrc/layernorm.hip one at a time (svae_layernorm_fwd / _fwd_multi, svae_layernorm_bwd /
_bwd_drop / _bwd_gelu / _bwd_multi, svae_colsum / _colsum_multi) and the small passes the fused tests of
test_kernels_gpu.py take as their reference (svae_dropout_bwd_cast, svae_cast_bf16, svae_gelu_bwd, svae_extract_rows),
against the float64 restatements of tests/ln_ref.py: per row and per column, at every layout's filled and partly
filled width, and at the smallest row counts at which a wave takes a second and a third row (the forward's prefetch
loop, the backward's accumulation of the affine partials over rows). The f32 bounds are ln_ref.bound(): 4 x the
f32-vs-f64 deviation of the same formulas on these inputs (measured on the CPU by test_ln_ref.py, recorded in
tests/golden/ln_bounds.json), never below 2^-21; bf16 outputs carry bf16's unit roundoff 2^-8 on top. Every output is a
view into a sentinel-guarded buffer, every partial slab is NaN before the launch."""
import ctypes
import functools

import pytest
import torch

import ln_ref as R
import sentinels as S

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae import _native as N

dev = 'cuda'
f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
NAN = float('nan')
XDT = [f32, bf16]
XID = ['x-f32', 'x-bf16']


@functools.lru_cache(maxsize=2)
def case(rows, D, n=1, integer_dy=False):
    """ln_ref.inputs on the device (shared by the tests of one shape; nothing writes to it)."""
    c = R.inputs(rows, D, n, integer_dy)
    d = R.Case()
    d.x, d.dres, d.gp = c.x.to(dev), c.dres.to(dev), c.gp.to(dev)
    d.ws, d.bs, d.dys = [w.to(dev) for w in c.ws], [b.to(dev) for b in c.bs], [t.to(dev) for t in c.dys]
    return d


def bits(t):
    return t.view(torch.int16) if t.dtype == bf16 else t.view(torch.int32)


def fwd(x, w, b, rows, D):
    """svae_layernorm_fwd into guarded buffers -> (y, mean, rstd)."""
    yf, y = S.matrix(rows, D, D, bf16)
    mf, mean = S.flat(rows)
    rf, rstd = S.flat(rows)
    K.layernorm_fwd(x, w, b, y, mean, rstd, rows, D)
    torch.cuda.synchronize()
    assert S.intact(yf, rows, D) and S.intact(mf) and S.intact(rf)
    return y, mean, rstd


def slabs(rows, D, n=1):
    """The backward's partial slabs, NaN before the launch: a block that skipped its slab shows in dw / db."""
    return S.flat(n * R.bwd_nblk(rows) * 2 * D, fill=NAN)


def check_affine(tag, wg, dw, db, key):
    D = dw.numel()
    S.report(f'{tag} dw', R.deviation(wg[:D], dw, rows=False), R.bound(f'{key}.dw'))
    S.report(f'{tag} db', R.deviation(wg[D:], db, rows=False), R.bound(f'{key}.db'))


# ================================================================================================ forward
@pytest.mark.parametrize('xdt', XDT, ids=XID)
@pytest.mark.parametrize('rows,D', R.FWD_CASES)
def test_layernorm_fwd(rows, D, xdt):
    """y per element, mean[r] and rstd[r] per row. The loop shapes are the smallest at which a wave of ln_fwd_kernel
    takes a second row (a third at 16387 x 64) while other waves take one fewer: the row loaded ahead has to become
    the current one, and the last trip must not load past the end."""
    for r, d, most in R.FWD_LOOP:
        if (r, d) == (rows, D):
            assert R.fwd_rows_per_wave(rows, D) == (most - 1, most)      # the dispatch changed: move the shape
    c = case(rows, D)
    x = c.x.to(xdt)
    y, mean, rstd = fwd(x, c.ws[0], c.bs[0], rows, D)
    yr, mr, rr = R.ln_fwd(x, c.ws[0], c.bs[0])
    tag = f'ln_fwd {rows}x{D} MAXV {R.fwd_maxv(D)} {xdt}'
    S.report(f'{tag} mean', R.deviation(mean, mr, rows=False), R.bound('fwd.mean'))
    S.report(f'{tag} rstd', R.deviation(rstd, rr, rows=False), R.bound('fwd.rstd'))
    S.ratio(f'{tag} y', R.bf16_excess(y, yr, R.bound('fwd.y')))


@pytest.mark.parametrize('n', [1, R.LN_MULTI_MAX])
@pytest.mark.parametrize('rows,D,most', R.FWD_LOOP)
def test_layernorm_fwd_multi(rows, D, most, n):
    """ln_fwd_multi_kernel's own row loop against float64; the affines differ visibly (w_j ~ j + 1, b_j ~ j), so an
    output written from another LayerNorm's w or b is off by its whole size."""
    assert R.fwd_rows_per_wave(rows, D) == (most - 1, most)
    c = case(rows, D, R.LN_MULTI_MAX)
    outs = [S.matrix(rows, D, D, bf16) for _ in range(n)]
    mf, mean = S.flat(rows)
    rf, rstd = S.flat(rows)
    K.layernorm_fwd_multi(c.x, c.ws[:n], c.bs[:n], [o[1] for o in outs], mean, rstd, rows, D)
    torch.cuda.synchronize()
    assert all(S.intact(o[0], rows, D) for o in outs) and S.intact(mf) and S.intact(rf)
    tag = f'ln_fwd_multi n={n} {rows}x{D}'
    for j in range(n):
        yr, mr, rr = R.ln_fwd(c.x, c.ws[j], c.bs[j])
        S.ratio(f'{tag} y[{j}]', R.bf16_excess(outs[j][1], yr, R.bound('fwd.y')))
    S.report(f'{tag} mean', R.deviation(mean, mr, rows=False), R.bound('fwd.mean'))
    S.report(f'{tag} rstd', R.deviation(rstd, rr, rows=False), R.bound('fwd.rstd'))


# ================================================================================================ backward
@pytest.mark.parametrize('xdt', XDT, ids=XID)
@pytest.mark.parametrize('rows,D', R.BWD_CASES)
def test_layernorm_bwd(rows, D, xdt):
    """dx per element, dw and db per column, from the forward kernel's own mean / rstd (as the engine calls it)
    against float64 with float64 statistics; dres absent, given, and aliasing dx. At the loop shapes a wave
    accumulates its affine partials over two rows (three at 8195 x 64) before the block's LDS reduction."""
    for r, d, most in R.BWD_LOOP:
        if (r, d) == (rows, D):
            assert R.bwd_rows_per_wave(rows) == (most - 1, most)
    c = case(rows, D)
    x = c.x.to(xdt)
    _, mean, rstd = fwd(x, c.ws[0], c.bs[0], rows, D)
    dxr, dwr, dbr, _ = R.ln_bwd(c.dys[0], x, c.ws[0])
    for mode in ('none', 'given', 'alias'):
        dxf, dx = S.matrix(rows, D, D, f32)
        ref = dxr
        dres = None
        if mode == 'given':
            dres = c.dres
        elif mode == 'alias':
            dx.copy_(c.dres)
            dres = dx
        if dres is not None:
            ref = dxr + c.dres.double()
        bff, dxb = S.matrix(rows, D, D, bf16) if mode != 'alias' else (None, None)
        pf, part = slabs(rows, D)
        wf, wg = S.flat(2 * D, fill=0.0)
        K.layernorm_bwd(c.dys[0], x, c.ws[0], mean, rstd, dres, dx, dxb, wg, rows, D, part)
        torch.cuda.synchronize()
        assert S.intact(dxf, rows, D) and S.intact(pf) and S.intact(wf)
        assert bool(torch.isfinite(part).all().item())                  # every block wrote its slab
        tag = f'ln_bwd {rows}x{D} MAXV {R.bwd_maxv(D)} {xdt} dres {mode}'
        S.report(f'{tag} dx', R.deviation(dx, ref), R.bound('bwd.dx'))
        check_affine(tag, wg, dwr, dbr, 'bwd')
        if dxb is not None:
            assert S.intact(bff, rows, D)
            S.ratio(f'{tag} dx_bf', R.bf16_excess(dxb, ref, R.bound('bwd.dx')))
            assert torch.equal(bits(dxb), bits(dx.bfloat16()))          # the copy is the rounding of what dx holds


def _exact_db(dys):
    return [dy.double().sum(0) for dy in dys]


@pytest.mark.parametrize('rows,D,most', R.BWD_LOOP)
def test_layernorm_bwd_counts_every_row_once(rows, D, most):
    """Integer dy in {-2 .. 2}: every partial sum of db is an integer below 2^24, so db must equal the float64 column
    sum exactly: each row is counted once and only once through the wave's row loop, the 4-wave LDS reduction, the
    slab write and colsum. The same for the GELU form and (LN_MULTI_MAX LayerNorms) the multi kernel."""
    assert R.bwd_rows_per_wave(rows) == (most - 1, most)
    n = R.LN_MULTI_MAX
    c = case(rows, D, n, True)
    _, mean, rstd = fwd(c.x, c.ws[0], c.bs[0], rows, D)
    want = _exact_db(c.dys)
    assert all(w.abs().max().item() > 8 for w in want)
    for form in ('plain', 'gelu'):
        pf, part = slabs(rows, D)
        wf, wg = S.flat(2 * D, fill=0.0)
        if form == 'plain':
            of, out = S.matrix(rows, D, D, f32)
            K.layernorm_bwd(c.dys[0], c.x, c.ws[0], mean, rstd, None, out, None, wg, rows, D, part)
        else:
            of, out = S.matrix(rows, D, D, bf16)
            K.layernorm_bwd_gelu(c.dys[0], c.x, c.ws[0], mean, rstd, c.gp, out, wg, rows, D, part)
        torch.cuda.synchronize()
        assert S.intact(of, rows, D) and S.intact(pf) and S.intact(wf)
        diff = (wg[D:].double() - want[0]).abs().max().item()
        print(f'ln_bwd {form} {rows}x{D}: largest |db - exact count| {diff}')
        assert torch.equal(wg[D:].double(), want[0])
    pf, part = slabs(rows, D, n)
    wgs = [S.flat(2 * D, fill=0.0) for _ in range(n)]
    dxf, dx = S.matrix(rows, D, D, f32)
    K.layernorm_bwd_multi(c.dys, c.x, c.ws, mean, rstd, None, dx, [w[1] for w in wgs], rows, D, part)
    torch.cuda.synchronize()
    assert S.intact(dxf, rows, D) and S.intact(pf) and all(S.intact(w[0]) for w in wgs)
    for j in range(n):
        assert torch.equal(wgs[j][1][D:].double(), want[j]), j
    assert not torch.equal(want[0], want[1])


@pytest.mark.parametrize('xdt', XDT, ids=XID)
@pytest.mark.parametrize('rows,D', R.GELU_CASES)
def test_layernorm_bwd_gelu(rows, D, xdt):
    """out = bf16(LN'(dy) gp) against float64 LN' times gp; the affine gradients are the LayerNorm's own."""
    c = case(rows, D)
    x = c.x.to(xdt)
    _, mean, rstd = fwd(x, c.ws[0], c.bs[0], rows, D)
    ref, dwr, dbr, _ = R.ln_bwd(c.dys[0], x, c.ws[0], gmul=c.gp)
    of, out = S.matrix(rows, D, D, bf16)
    pf, part = slabs(rows, D)
    wf, wg = S.flat(2 * D, fill=0.0)
    K.layernorm_bwd_gelu(c.dys[0], x, c.ws[0], mean, rstd, c.gp, out, wg, rows, D, part)
    torch.cuda.synchronize()
    assert S.intact(of, rows, D) and S.intact(pf) and S.intact(wf)
    tag = f'ln_bwd_gelu {rows}x{D} {xdt} ({R.bwd_rows_per_wave(rows)[1]} rows / wave)'
    S.ratio(f'{tag} out', R.bf16_excess(out, ref, R.bound('gelu.out')))
    check_affine(tag, wg, dwr, dbr, 'bwd')


@pytest.mark.parametrize('mode', ['zrow', 'zrow_bf', 'both'])
@pytest.mark.parametrize('rows,D', R.ZSPLICE_CASES)
def test_layernorm_bwd_zsplice(rows, D, mode):
    """zero_mod = 37: the moved rows fall on different waves of their blocks (rows 0, 37, 74, 111: waves 0, 1, 2, 3).
    The moved rows equal the float64 reference (and, bit for bit, the rows a plain launch leaves in dx), their places
    in dx and dx_bf are zero, every other row is the plain launch's; an output that was not passed is not written."""
    zm = R.ZERO_MOD
    c = case(rows, D)
    _, mean, rstd = fwd(c.x, c.ws[0], c.bs[0], rows, D)
    dxr, dwr, dbr, zr = R.ln_bwd(c.dys[0], c.x, c.ws[0], c.dres, zero_mod=zm)
    nz = zr.shape[0]
    plain = torch.empty(rows, D, device=dev)
    pf, part = slabs(rows, D)
    K.layernorm_bwd(c.dys[0], c.x, c.ws[0], mean, rstd, c.dres, plain, None, torch.zeros(2 * D, device=dev), rows, D,
                    part)
    dxf, dx = S.matrix(rows, D, D, f32)
    bff, dxb = S.matrix(rows, D, D, bf16)
    zf, zrow = S.matrix(nz, D, D, f32)
    zbf, zrow_bf = S.matrix(nz, D, D, bf16)
    pf, part = slabs(rows, D)
    wf, wg = S.flat(2 * D, fill=0.0)
    K.layernorm_bwd(c.dys[0], c.x, c.ws[0], mean, rstd, c.dres, dx, dxb, wg, rows, D, part,
                    zsplice=(zm, zrow if mode != 'zrow_bf' else None, zrow_bf if mode != 'zrow' else None))
    torch.cuda.synchronize()
    assert all(S.intact(b, r, D) for b, r in ((dxf, rows), (bff, rows), (zf, nz), (zbf, nz)))
    assert S.intact(pf) and S.intact(wf)
    moved = torch.arange(rows, device=dev) % zm == 0
    assert int(moved.sum()) == nz and {int(r) % 4 for r in moved.nonzero().flatten()[:4]} == {0, 1, 2, 3}
    tag = f'ln_bwd zsplice {mode} {rows}x{D}'
    if mode != 'zrow_bf':
        S.report(f'{tag} zrow', R.deviation(zrow, zr), R.bound('bwd.dx'))
        assert torch.equal(bits(zrow), bits(plain[moved]))
    else:
        assert bool((zrow == S.SENTINEL).all().item())
    if mode != 'zrow':
        S.ratio(f'{tag} zrow_bf', R.bf16_excess(zrow_bf, zr, R.bound('bwd.dx')))
        assert torch.equal(bits(zrow_bf), bits(plain[moved].bfloat16()))
    else:
        assert bool((zrow_bf == torch.tensor(S.SENTINEL, dtype=bf16)).all().item())
    assert bool((dx[moved] == 0).all().item()) and bool((dxb[moved] == 0).all().item())
    assert torch.equal(bits(dx[~moved]), bits(plain[~moved]))
    assert torch.equal(bits(dxb[~moved]), bits(plain[~moved].bfloat16()))
    S.report(f'{tag} dx', R.deviation(dx[~moved], dxr[~moved]), R.bound('bwd.dx'))
    check_affine(tag, wg, dwr, dbr, 'bwd')                       # the moved rows still count in dw / db


@pytest.mark.parametrize('p', [0.25])
@pytest.mark.parametrize('rows,D', [(333, 576), (333, 132)])
def test_layernorm_bwd_zsplice_with_bf_drop(rows, D, p):
    """The z splice together with the bf16 copy's dropout: the kept set is ln_ref.dropout_keep's (the restatement of
    rand_uniform4, counter (r D + c) >> 2), kept elements are dx / (1 - p), position-0 rows of dx_bf are zero."""
    zm, seed = R.ZERO_MOD, 0x9E3779B97F4A7C15
    c = case(rows, D)
    _, mean, rstd = fwd(c.x, c.ws[0], c.bs[0], rows, D)
    dxr, _, _, zr = R.ln_bwd(c.dys[0], c.x, c.ws[0], c.dres, zero_mod=zm)
    keep = R.dropout_keep(seed, rows, D, p).to(dev)
    dxf, dx = S.matrix(rows, D, D, f32)
    bff, dxb = S.matrix(rows, D, D, bf16)
    zf, zrow = S.matrix(zr.shape[0], D, D, f32)
    zbf, zrow_bf = S.matrix(zr.shape[0], D, D, bf16)
    pf, part = slabs(rows, D)
    K.layernorm_bwd(c.dys[0], c.x, c.ws[0], mean, rstd, c.dres, dx, dxb, torch.zeros(2 * D, device=dev), rows, D, part,
                    bf_drop=(p, seed, zm), zsplice=(zm, zrow, zrow_bf))
    torch.cuda.synchronize()
    assert all(S.intact(b, r, D) for b, r in ((dxf, rows), (bff, rows), (zf, zr.shape[0]), (zbf, zr.shape[0])))
    moved = torch.arange(rows, device=dev) % zm == 0
    tag = f'ln_bwd zsplice + drop {rows}x{D} p={p}'
    S.report(f'{tag} dx', R.deviation(dx[~moved], dxr[~moved]), R.bound('bwd.dx'))
    assert bool((dx[moved] == 0).all().item())
    S.report(f'{tag} zrow', R.deviation(zrow, zr), R.bound('bwd.dx'))
    assert torch.equal(bits(zrow_bf), bits(zrow.bfloat16()))             # the moved rows carry no dropout
    assert bool((dxb[moved] == 0).all().item())
    live = ~moved
    assert torch.equal(dxb[live] != 0, keep[live] & (dx[live] != 0))     # the kept set, exactly
    frac = 1 - keep[live].float().mean().item()
    print(f'{tag}: dropped {frac:.4f}')
    assert abs(frac - p) < 0.02
    ref = torch.where(keep, dxr / (1 - float(torch.tensor(p, dtype=f32))), torch.zeros_like(dxr))
    S.ratio(f'{tag} dx_bf', R.bf16_excess(dxb[live], ref[live], R.bound('bwd.dx'), extra=2.0 ** -23))
    want = torch.where(keep, dx * R.dropout_scale(p), torch.zeros_like(dx)).bfloat16()
    assert torch.equal(bits(dxb[live]), bits(want[live]))                # and bf16(dx * f32(1 / (1 - p))) bit for bit


@pytest.mark.parametrize('n', R.MULTI_N)
@pytest.mark.parametrize('rows,D', R.MULTI_BWD_CASES)
def test_layernorm_bwd_multi(rows, D, n):
    """ln_bwd_multi_kernel against float64 (not against the single kernel, whose row program it shares): dx per
    element, every LayerNorm's dw and db per column; dres None (the `ok && dres` branch), given, aliasing dx."""
    c = case(rows, D, R.LN_MULTI_MAX)
    dys, ws = c.dys[:n], c.ws[:n]
    _, mean, rstd = fwd(c.x, c.ws[0], c.bs[0], rows, D)
    dxr, grads = R.ln_bwd_multi(dys, c.x, ws)
    for mode in ('none', 'given', 'alias'):
        dxf, dx = S.matrix(rows, D, D, f32)
        dres, ref = None, dxr
        if mode != 'none':
            ref = dxr + c.dres.double()
            dres = c.dres
            if mode == 'alias':
                dx.copy_(c.dres)
                dres = dx
        pf, part = slabs(rows, D, n)
        wgs = [S.flat(2 * D, fill=0.0) for _ in range(n)]
        K.layernorm_bwd_multi(dys, c.x, ws, mean, rstd, dres, dx, [w[1] for w in wgs], rows, D, part)
        torch.cuda.synchronize()
        assert S.intact(dxf, rows, D) and S.intact(pf) and all(S.intact(w[0]) for w in wgs)
        assert bool(torch.isfinite(part).all().item())
        tag = f'ln_bwd_multi n={n} {rows}x{D} ({R.bwd_rows_per_wave(rows)[1]} rows / wave) dres {mode}'
        S.report(f'{tag} dx', R.deviation(dx, ref), R.bound('multi.dx'))
        for j in range(n):
            check_affine(f'{tag} [{j}]', wgs[j][1], grads[j][0], grads[j][1], 'multi')


# ================================================================================================ colsum
def _colsum_input(rows, cols, ld, dt, integer, seed):
    gen = torch.Generator().manual_seed(seed)
    v = torch.randint(-3, 4, (rows, cols), generator=gen).float() if integer else torch.randn(rows, cols, generator=gen)
    full = torch.full((rows, ld), 1.0e4, dtype=dt, device=dev)           # a read past `cols` is off by 1e4
    full[:, :cols] = v.to(dev).to(dt)
    return full


def _colsum_check(tag, out, inp, cols, out0, integer):
    """Per column against float64. Integers: exact. Otherwise the worst case of a sum of k + 1 f32 terms in any
    order (the kernel's tree, then atomic adds), k 2^-24 sum |terms|."""
    v = inp[:, :cols].double()
    ref = v.sum(0) + out0.double()
    if integer:
        assert torch.equal(out.double(), ref), tag
        return
    allow = (v.shape[0] + 1) * 2.0 ** -24 * (v.abs().sum(0) + out0.double().abs())
    S.ratio(tag, ((out.double() - ref).abs() / allow).max().item())


@pytest.mark.parametrize('dt', [f32, bf16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('rows', [1, 16, 17, 127, 128, 129, 1024 + 1])
def test_colsum(rows, dt):
    """Around the 16-row thread group, the 128-row unrolled trip and the first row counts that split (129: two splits
    of 65 rows; 1025: nine of 114), with ld = cols and ld > cols, overwriting a NaN-filled out (accumulate = False)
    and adding to a known one."""
    for cols, ld in ((4, 4), (64, 64), (132, 140), (1024, 1032)):
        for integer in (True, False):
            inp = _colsum_input(rows, cols, ld, dt, integer, rows + cols)
            of, out = S.flat(cols, fill=NAN)
            K.colsum(inp, rows, cols, ld, out, accumulate=False)
            out0 = (torch.arange(cols, device=dev) % 7 - 3).float()
            af, acc = S.flat(cols)
            acc.copy_(out0)
            K.colsum(inp, rows, cols, ld, acc, accumulate=True)
            torch.cuda.synchronize()
            assert S.intact(of) and S.intact(af)
            tag = f'colsum {rows}x{cols} ld {ld} {dt} integer={integer}'
            _colsum_check(f'{tag} overwrite', out, inp, cols, torch.zeros_like(out0), integer)
            _colsum_check(f'{tag} accumulate', acc, inp, cols, out0, integer)


@pytest.mark.parametrize('integer', [True, False])
def test_colsum_multi_segments_keep_apart(integer):
    """COLSUM_MAX segments of different rows, cols and ld in one launch: every out gets its own segment's sums on top
    of what it held, and nothing else (each sits in its own guarded buffer)."""
    rows = [1, 16, 17, 127, 128, 129, 1025, 300]
    cols = [4, 64, 68, 132, 512, 1024, 2048, 260]
    lds = [4, 72, 68, 140, 512, 1032, 2048, 264]
    assert len(rows) == R.COLSUM_MAX == N.COLSUM_MAX
    inps = [_colsum_input(r, c, ld, f32, integer, 50 + i) for i, (r, c, ld) in enumerate(zip(rows, cols, lds))]
    out0 = [(torch.arange(c, device=dev) % 5 + i).float() for i, c in enumerate(cols)]
    outs = [S.flat(c) for c in cols]
    for (_, o), o0 in zip(outs, out0):
        o.copy_(o0)
    K.colsum_multi([(inp, r, c, ld, o[1]) for inp, r, c, ld, o in zip(inps, rows, cols, lds, outs)])
    torch.cuda.synchronize()
    for i in range(len(rows)):
        assert S.intact(outs[i][0])
        _colsum_check(f'colsum_multi segment {i} ({rows[i]}x{cols[i]})', outs[i][1], inps[i], cols[i], out0[i], integer)


# ================================================================================================ the small passes
@pytest.mark.parametrize('rows,cols,pad,p', [(37, 132, 0, 0.0), (37, 132, 8, 0.0), (37, 132, 8, 0.25),
                                             (333, 576, 8, 0.1), (4096 + 1, 1024, 0, 0.1)])
def test_dropout_bwd_cast_is_the_restated_mask(rows, cols, pad, p):
    """out = bf16(g keep / (1 - p)) bit for bit with keep = ln_ref.dropout_keep: the mask of rand_uniform4 pinned to
    its restatement. ld_in = cols + 8 (the padding holds 1e4); 4097 x 1024 = 4096 blocks' worth + 1024 elements: the
    first block takes a second trip of the grid stride."""
    seed = 0x1234567 + rows
    ld = cols + pad
    g = torch.full((rows, ld), 1.0e4, device=dev)
    g[:, :cols] = torch.randn(rows, cols, generator=torch.Generator().manual_seed(rows + cols)).to(dev)
    of, out = S.flat(rows * cols, bf16)
    K.dropout_bwd_cast(g, out, p, seed, rows, cols, ld_in=ld)
    torch.cuda.synchronize()
    assert S.intact(of)
    keep = R.dropout_keep(seed, rows, cols, p).to(dev)
    want = torch.where(keep, g[:, :cols] * R.dropout_scale(p), torch.zeros(rows, cols, device=dev)).bfloat16()
    dropped = 1 - keep.float().mean().item()
    print(f'dropout_bwd_cast {rows}x{cols} ld {ld} p={p}: dropped {dropped:.4f}')
    assert bool(keep.all().item()) if p == 0 else abs(dropped - p) < 0.02
    assert torch.equal(bits(out.view(rows, cols)), bits(want))


@pytest.mark.parametrize('n', [1, 3, 4, 5, 1023, 4096 * 1024 + 3])
def test_cast_bf16(n):
    """The scalar tail (n % 4 != 0) and, at 4096 x 1024 + 3, the grid-stride loop's second trip."""
    x = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(dev)
    of, out = S.flat(n, bf16)
    K.cast_bf16(x, out, n)
    torch.cuda.synchronize()
    assert S.intact(of) and torch.equal(bits(out), bits(x.bfloat16()))


@pytest.mark.parametrize('n', [1, 255, 4096 * 256 + 1])
def test_gelu_bwd(n):
    gen = torch.Generator().manual_seed(n)
    dx = torch.randn(n, generator=gen).to(dev)
    gp = (torch.rand(n, generator=gen) * 1.2 - 0.1).to(bf16).to(dev)
    of, out = S.flat(n, bf16)
    K.gelu_bwd(dx, gp, out, n)
    torch.cuda.synchronize()
    assert S.intact(of) and torch.equal(bits(out), bits((dx * gp.float()).bfloat16()))


@pytest.mark.parametrize('D', [8, 300, 512])
def test_extract_rows(D):
    """Rows r % mod == 0 of x (leading dimension D + 8) move to out and are zeroed; every other element of x, the
    padding of the moved rows included, is unchanged."""
    rows, mod, ld = 6 * 37, 37, D + 8
    x = torch.randn(rows, ld, generator=torch.Generator().manual_seed(D)).to(dev)
    before = x.clone()
    of, out = S.matrix(rows // mod, D, D, f32)
    K.extract_rows(x, ld, rows, mod, D, out)
    torch.cuda.synchronize()
    assert S.intact(of, rows // mod, D)
    assert torch.equal(bits(out), bits(before[::mod, :D]))
    want = before.clone()
    want[::mod, :D] = 0
    assert torch.equal(bits(x), bits(want))


# ================================================================================================ rejected calls
def test_rejected_arguments_launch_nothing():
    """The argument checks the entries make today: status SVAE_EINVAL (1) before any launch, outputs untouched."""
    rows, D = 8, 64
    c = case(rows, D, R.LN_MULTI_MAX)
    _, mean, rstd = fwd(c.x, c.ws[0], c.bs[0], rows, D)
    big = torch.zeros(rows, 1028, device=dev)
    wbig = torch.ones(1028, device=dev)
    yf, y = S.matrix(rows, 1028, 1028, bf16)
    mf, m = S.flat(rows)
    dxf, dx = S.matrix(rows, 1028, 1028, f32)
    pf, part = slabs(rows, 1028, R.LN_MULTI_MAX)
    wf, wg = S.flat(2 * 1028)
    dyb = torch.zeros(rows, 1028, device=dev, dtype=bf16)
    calls = []
    for d in (130, 1028):                                        # D % 4 != 0, D > 1024
        calls += [lambda d=d: K.layernorm_fwd(big, wbig, wbig, y, m, m, rows, d),
                  lambda d=d: K.layernorm_fwd_multi(big, [wbig], [wbig], [y], m, m, rows, d),
                  lambda d=d: K.layernorm_bwd(dyb, big, wbig, mean, rstd, None, dx, None, wg, rows, d, part),
                  lambda d=d: K.layernorm_bwd_gelu(dyb, big, wbig, mean, rstd, dyb, y, wg, rows, d, part),
                  lambda d=d: K.layernorm_bwd_multi([dyb], big, [wbig], mean, rstd, None, dx, [wg], rows, d, part)]
    calls += [lambda: K.layernorm_fwd(big, wbig, wbig, y, m, m, 0, D),                         # rows = 0
              lambda: K.layernorm_fwd_multi(big, [wbig], [wbig], [y], m, m, 0, D),
              lambda: K.layernorm_bwd(dyb, big, wbig, mean, rstd, None, dx, None, wg, 0, D, part),
              lambda: K.layernorm_fwd_z(big, big, 4, wbig, wbig, y, m, m, rows, 132),         # fwd_z: D % 8 != 0
              lambda: K.layernorm_bwd(dyb, big, wbig, mean, rstd, None, dx, None, wg, rows, D, part,
                                      bf_drop=(0.1, 7, 0))]                                    # drop without dx_bf
    for call in calls:
        with pytest.raises(RuntimeError, match='status 1'):
            call()
    over = R.LN_MULTI_MAX + 1                                    # n > LN_MULTI_MAX, at the C entries themselves
    arr = lambda t: (ctypes.c_void_p * over)(*[t.data_ptr()] * over)
    assert N.lib.svae_layernorm_fwd_multi(big.data_ptr(), arr(wbig), arr(wbig), arr(y), over, m.data_ptr(),
                                          m.data_ptr(), rows, D, K.stream()) == 1
    assert N.lib.svae_layernorm_bwd_multi(arr(dyb), big.data_ptr(), arr(wbig), mean.data_ptr(), rstd.data_ptr(), None,
                                          dx.data_ptr(), arr(part), R.bwd_nblk(rows), over, rows, D, K.stream()) == 1
    torch.cuda.synchronize()
    assert S.intact(yf, 0, 0) and S.intact(mf) and S.intact(dxf, 0, 0) and S.intact(wf)
    assert bool((m == S.SENTINEL).all().item()) and bool((wg == S.SENTINEL).all().item())
    assert bool(torch.isnan(part).all().item()) and S.intact(pf)
