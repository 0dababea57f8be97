"""TransformerVAE.sample_stream end to end: the streaming bulk sampler must give, for every sample, exactly the ids
`sample()` gives for the same latent and seed, whatever the slot count and however often slots are refilled.

All comparisons are exact: StreamDecoder runs KVDecoder's arithmetic per row (the same kernel bodies, the same
split rule), and a sample's multinomial draws are keyed by (seed, position, sample number), which in `sample()`
is (seed, position, row).

Slot counts: svae_dec_linear's split rule reads the number of 64-row blocks, not M, so the summation order of the
narrow linears is the same for any two row counts within the same number of blocks. Every compared pair stays
within one: 5 / 7 / 48 rows (one block), 3 / 20 rows (one block), 70 / 100 rows (two blocks).

Lengths vary under nucleus sampling because a constant is added to the end token's output bias: ln(q V / (1 - q))
makes the end token's probability about q per step on the near-uniform logits of a random-init model. q per
configuration is chosen so that the refill tests' preconditions hold (asserted in `lengths_vary`).
"""
import functools
import math
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.params import HParams, TIED_ALIASES, init_params  # noqa: E402

if torch.cuda.is_available():
    from sparse_vae import TransformerVAE, TransformerVAEHparams, trim_samples

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END, V = 2, 32768
#          d_model, window, N, T, q (end-token probability per step under nucleus sampling)
CONFIGS = {'dense': (128, 0, 48, 40, 0.05), 'window2': (128, 2, 20, 140, 0.012), 'd512': (512, 0, 100, 24, 0.05)}
MODES = {'greedy': dict(temperature=0.0), 'nucleus': dict(temperature=1.0, top_p=0.9, repetition_penalty=1.2)}


def end_bias(q):
    return math.log(q * V / (1 - q))


@functools.lru_cache(maxsize=None)
def model_params(d):
    return init_params(HParams(latent_depth=64, kl_weight=1.0, d_model=d, num_heads=8, num_layers=4), 77 + d)


@functools.lru_cache(maxsize=None)
def model(cfg, mode):
    """greedy: the plain weights, never ending (end_token -1); nucleus: the end token's bias raised."""
    d, window, _, _, q = CONFIGS[cfg]
    mhp = TransformerVAEHparams(latent_depth=64, sparse_self_attention=bool(window), attn_window_size=window or 4,
                                kl_weight=1.0, d_model=d, num_heads=8, num_layers=4)
    m = TransformerVAE(mhp, device='cuda')
    sd = dict(model_params(d))
    for alias in TIED_ALIASES:
        sd[alias] = sd['input_layer.0.weight']
    if mode == 'nucleus':
        bias = sd['output_layer.3.bias'].clone()
        bias[END] += end_bias(q)
        sd['output_layer.3.bias'] = bias
    m.load_state_dict(sd, strict=True)
    m.eval()
    m.start_token, m.end_token = 1, (END if mode == 'nucleus' else -1)
    return m


@functools.lru_cache(maxsize=None)
def latent(cfg):
    N = CONFIGS[cfg][2]
    return torch.randn(N, 1, 64, generator=torch.Generator().manual_seed(N)).cuda()


@functools.lru_cache(maxsize=None)
def reference(cfg, mode):
    """sample() on all N rows at once: computed once per (configuration, mode), never modified."""
    _, _, N, T, _ = CONFIGS[cfg]
    m, z = model(cfg, mode), latent(cfg)         # built before seeding: construction draws from the generator
    torch.manual_seed(1234)
    return m.sample(T, N, z=z, **MODES[mode])


def stream(cfg, mode, slots, **kw):
    _, _, N, T, _ = CONFIGS[cfg]
    m, z = model(cfg, mode), latent(cfg)
    torch.manual_seed(1234)
    return m.sample_stream(T, N, slots=slots, z=z, **MODES[mode], **kw)


def lengths_vary(cfg):
    """The preconditions of the refill tests, on the nucleus reference: at least a quarter of the samples end
    before T / 2, at least two run to full length, and every sample is complete (ended, or full length)."""
    _, _, N, T, _ = CONFIGS[cfg]
    ref = reference(cfg, 'nucleus')
    lens = np.array([len(r) for r in trim_samples(ref, END)])
    full = int((lens == T - 1).sum())
    print(f'{cfg}: lengths min {lens.min()} median {np.median(lens)} max {lens.max()}, '
          f'{int((lens < T / 2).sum())} of {N} before T/2, {full} full length')
    assert (lens < T / 2).sum() * 4 >= N and full >= 2
    rows = ref.cpu()
    for r, n in zip(rows, lens):
        assert (r[n:] == 0).all() and (n == T - 1 or r[n - 1] == END)
        assert r[T - 2] == 0                     # the last column is never written (KVDecoder.run's bound)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('cfg', list(CONFIGS))
def test_no_refill_equals_sample(cfg, mode):
    """slots = N: every slot holds one sample from the first step to its end."""
    _, _, N, T, _ = CONFIGS[cfg]
    out = stream(cfg, mode, N)
    assert out.dtype == torch.int16 and out.shape == (N, T - 1) and out.is_cuda
    assert torch.equal(out.long(), reference(cfg, mode))
    if mode == 'nucleus':
        lengths_vary(cfg)


@pytest.mark.parametrize('mode', list(MODES))
@pytest.mark.parametrize('cfg,slots', [('dense', 5), ('dense', 7), ('window2', 3), ('d512', 70)])
def test_refill_does_not_change_a_sample(cfg, slots, mode):
    """Fewer slots than samples: slots are refilled as samples end, at positions unrelated to their neighbours',
    on cache rows a previous sample left behind. The slot counts stay within the reference's number of 64-row
    blocks (see the module docstring)."""
    N = CONFIGS[cfg][2]
    assert (slots + 63) // 64 == (N + 63) // 64
    if mode == 'nucleus':
        lengths_vary(cfg)
    assert torch.equal(stream(cfg, mode, slots).long(), reference(cfg, mode))


@pytest.mark.parametrize('mode', list(MODES))
def test_graph_replay_equals_eager_steps(mode):
    eager = stream('dense', mode, 5, use_graph=False)
    assert torch.equal(eager, stream('dense', mode, 5)) and torch.equal(eager.long(), reference('dense', mode))


# ------------------------------------------------------------------------------------------------ edges
def test_one_sample():
    m = model('dense', 'nucleus')
    z = latent('dense')[:1]
    torch.manual_seed(1234)
    want = m.sample(40, 1, z=z, **MODES['nucleus'])
    torch.manual_seed(1234)
    assert torch.equal(m.sample_stream(40, 1, z=z, **MODES['nucleus']).long(), want)


def test_fewer_samples_than_slots():
    """Slots 20 .. 47 are idle from the first step."""
    _, _, N, T, _ = CONFIGS['dense']
    m = model('dense', 'nucleus')
    torch.manual_seed(1234)
    out = m.sample_stream(T, 20, slots=N, z=latent('dense')[:20], **MODES['nucleus'])
    assert torch.equal(out.long(), reference('dense', 'nucleus')[:20])


def test_no_samples_and_low_kl_weight():
    m = model('dense', 'nucleus')
    out = m.sample_stream(40, 0)
    assert out.shape == (0, 39) and out.dtype == torch.int16
    m.hparams.kl_weight = 0.5
    try:
        assert m.sample_stream(40, 4) is None
    finally:
        m.hparams.kl_weight = 1.0


def test_max_length_three_is_one_step_per_sample():
    m = model('dense', 'nucleus')
    z = latent('dense')[:12]
    torch.manual_seed(1234)
    want = m.sample(3, 12, z=z, **MODES['nucleus'])
    torch.manual_seed(1234)
    out = m.sample_stream(3, 12, slots=5, z=z, **MODES['nucleus'])
    assert out.shape == (12, 2) and torch.equal(out.long(), want) and (out[:, 1] == 0).all()


def test_cpu_model_raises_the_no_fallback_error():
    m = TransformerVAE(TransformerVAEHparams(d_model=128, num_layers=4, num_heads=8, sparse_self_attention=False),
                       device='cpu')
    with pytest.raises(RuntimeError, match='no CPU fallback|There is no CPU fallback'):
        m.sample_stream(8, 4)


def test_two_identical_calls_agree():
    assert torch.equal(stream('dense', 'nucleus', 7), stream('dense', 'nucleus', 7))


# ------------------------------------------------------------------------------------------------ sample.py
def test_sample_py_end_to_end(tmp_path):
    """The tool on the `tiny` preset: the .npz rows are sample_stream's for the same weights and seed, and --loop
    (batch_generate_samples over model.sample) writes the same number of samples."""
    sys.path.insert(0, ROOT)
    try:
        import sample as tool
        from train import build_config
    finally:
        sys.path.remove(ROOT)
    config = build_config(['preset=tiny'])
    m = TransformerVAE(TransformerVAEHparams(**config['model']), device='cuda')
    m.eval()
    weights, out, out_loop = tmp_path / 'w.pt', tmp_path / 's.npz', tmp_path / 'l.npz'
    torch.save(m.state_dict(), weights)
    argv = ['--preset', 'tiny', '--weights', str(weights), '--num-samples', '40', '--slots', '8', '--max-length', '32',
            '--seed', '99']
    tool.main(argv + ['--out', str(out)])
    torch.manual_seed(99)
    want = m.sample_stream(32, 40, slots=8).cpu().numpy()
    got = np.load(out)
    assert got['ids'].dtype == np.int16 and np.array_equal(got['ids'], want)
    lens = np.array([len(r) for r in trim_samples(torch.from_numpy(want), 2)])
    assert np.array_equal(got['lengths'], lens) and 'd_model' in str(got['hparams'])
    tool.main(argv + ['--out', str(out_loop), '--loop'])
    loop = np.load(out_loop)
    assert loop['ids'].shape == (40, 31) and loop['lengths'].shape == (40,)
