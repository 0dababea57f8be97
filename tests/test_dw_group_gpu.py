"""The grouped weight-gradient pass (svae_gemm_group / kernels.linear_dw_group, and the engine's deferral of every
layer's dW GEMMs to it) against float64 products and against the per-layer path (GPU only).

Tolerance on random data: the relative Frobenius error bar test_kernels_gpu.py puts on its f32-output GEMMs, 1e-5
(that file checks the dW entry points on integer data only, exactly). It holds with room here: the operands are
exact bf16 values, every product is exact in f32, and only the f32 accumulation rounds -- about sqrt(K) 2^-24 relative
for K <= 1088 rows, ~2e-6; between the grouped and the per-layer path only the summation order over K differs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K

dev = 'cuda'
SHAPES = [(512, 256), (256, 768), (320, 192), (64, 64)]   # (n_out, n_in): an edge tile in M, in N, and < one tile
BIAS = [True, False, True, False]
MODES = {   # splits per GEMM, blocks per launch (0: one per tile)
    'unsplit': ((1, 1, 1, 1), 0),
    'mixed': ((1, 3, 2, 1), 0),
    'capped': ((1, 1, 1, 1), 5),          # 8 tiles on <= 5 blocks: blocks walk several tiles
    'capped_mixed': ((1, 3, 2, 1), 2),    # 3 whole-K tiles on 2 blocks, 13 slices on 2
}


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _jobs(rows, integer, seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    jobs, refs = [], []
    for (n_out, n_in), with_bias in zip(SHAPES, BIAS):
        if integer:   # sums stay below 2^24: exact in f32 in any order
            dY = torch.randint(-2, 3, (rows, n_out), device=dev, generator=g).float().bfloat16()
            X = torch.randint(-2, 3, (rows, n_in), device=dev, generator=g).float().bfloat16()
            Wg = torch.full((n_out, n_in), 0.5, device=dev)
            bg = torch.full((n_out,), 1.5, device=dev) if with_bias else None
        else:
            dY = torch.randn(rows, n_out, device=dev, generator=g).bfloat16()
            X = torch.randn(rows, n_in, device=dev, generator=g).bfloat16()
            Wg = torch.randn(n_out, n_in, device=dev, generator=g)
            bg = torch.randn(n_out, device=dev, generator=g) if with_bias else None
        refs.append((Wg.double() + dY.double().t() @ X.double(),
                     bg.double() + dY.double().sum(0) if with_bias else None))
        jobs.append((dY, X, Wg, rows, n_out, n_in, None, None, bg))
    return jobs, refs


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('rows', [200, 1088])   # a K tail (200 = 3 x 64 + 8; its third of 3 slices is empty) and 17 K-tiles
def test_group_kernel(rows, mode):
    """Four GEMMs of different shapes in one grouped pass, accumulating into non-zero gradients, two with bias row
    sums: exact on small-integer data, within the f32 GEMM bar on random data; the table is re-uploaded when the
    operands change and reused when they do not."""
    splits, cap = MODES[mode]
    state = K.DwGroupState(torch.device(dev))
    jobs, refs = _jobs(rows, True, rows + len(mode))
    K.linear_dw_group(jobs, splits, state, max_blocks=cap)
    torch.cuda.synchronize()
    for j, (w_ref, b_ref) in zip(jobs, refs):
        assert torch.equal(j[2].double(), w_ref), (j[4], j[5])
        if b_ref is not None:
            assert torch.equal(j[8].double(), b_ref), (j[4], j[5])
    # the same operands again (the table is not uploaded): accumulates the same product once more
    K.linear_dw_group(jobs, splits, state, max_blocks=cap)
    torch.cuda.synchronize()
    for j, (w_ref, b_ref) in zip(jobs, refs):
        assert torch.equal(j[2].double(), 2 * w_ref - 0.5), (j[4], j[5])
        if b_ref is not None:
            assert torch.equal(j[8].double(), 2 * b_ref - 1.5), (j[4], j[5])
    # other operands through the same state (a changed table)
    jobs, refs = _jobs(rows, False, rows + 77)
    K.linear_dw_group(jobs, splits, state, max_blocks=cap)
    torch.cuda.synchronize()
    for j, (w_ref, b_ref) in zip(jobs, refs):
        e = _rel(j[2], w_ref)
        print(f'{mode} rows {rows} {j[4]}x{j[5]}: rel {e:.2e}')
        assert e < 1e-5, (j[4], j[5], e)
        if b_ref is not None:
            assert _rel(j[8], b_ref) < 1e-5, (j[4], j[5])


def test_group_rejects_a_second_round_of_whole_k_tiles():
    """More whole-K tiles than compute units with no block cap given: refused before any launch."""
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    n = ncu // 16 + 1                                   # 16 tiles each
    dY = torch.zeros(64, 1024, device=dev, dtype=torch.bfloat16)
    X = torch.zeros(64, 1024, device=dev, dtype=torch.bfloat16)
    Wg = torch.zeros(1024, 1024, device=dev)
    jobs = [(dY, X, Wg, 64, 1024, 1024, None, None, None)] * n
    with pytest.raises(RuntimeError):
        K.linear_dw_group(jobs, [1] * n, K.DwGroupState(torch.device(dev)))


def _tiny_grads(monkeypatch, group):
    import oracle
    from oracle.params import portable_ids, portable_normal
    from sparse_vae.engine import FlatParams, VAEEngine
    monkeypatch.setenv('SVAE_DW_GROUP', group)
    hp = oracle.HParams(d_model=128, num_heads=8, num_layers=4, kl_weight=0.5)
    params = oracle.init_params(hp, 31)
    B, L = 4, 128
    ids = torch.from_numpy(portable_ids((B, L), 32)).to(dev)
    ntok = torch.full((B,), L, dtype=torch.int64, device=dev)
    eps = torch.from_numpy(portable_normal(B * 64, 'eps', 31).reshape(B, 1, 64).astype('float32')).to(dev)
    flat = FlatParams(hp, torch.device(dev))
    for n in flat.offsets:
        flat.view(n).copy_(params[n])
    eng = VAEEngine(hp, flat)
    assert eng.dw_group == (group == '1')
    out = eng.forward(ids, ntok, eps=eps, dropout=0.1, seed=5, kl_weight=0.5)
    eng.backward(torch.ones((), device=dev), 0.5)
    torch.cuda.synchronize()
    return out['loss'].clone(), {n: flat.g(n).clone() for n in flat.live_names}


def test_engine_grouped_matches_per_layer(monkeypatch):
    """The tiny model (4 layers, d 128, seq 128) at batch 4, dropout on, same weights, tokens and noise: the forward
    is untouched (bit-identical loss), and every parameter's gradient agrees with the per-layer path within the bar
    (only the order of the f32 sums over the token rows differs)."""
    loss1, g1 = _tiny_grads(monkeypatch, '1')
    loss0, g0 = _tiny_grads(monkeypatch, '0')
    assert torch.equal(loss1, loss0)
    worst = max((_rel(g1[n], g0[n]), n) for n in g0)
    print(f'worst gradient difference grouped vs per layer: {worst[0]:.2e} ({worst[1]})')
    for n in g0:
        assert _rel(g1[n], g0[n]) < 1e-5, (n, _rel(g1[n], g0[n]))
    assert any(g0[n].abs().max() > 0 for n in g0 if n.endswith('ffn.0.weight'))
