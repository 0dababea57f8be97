"""Latent index, the parts that need no GPU: the three svae_latent_* entry points are declared, bound and exported;
bad arguments are refused before any launch; LatentIndex keeps its books on CPU tensors, round-trips through .npz and
refuses to search there (no CPU fallback); the two command-line scripts parse their documented arguments."""
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ('svae_latent_prepare', 'svae_latent_scores', 'svae_latent_topk')
P = 4096          # a non-NULL, 16-byte aligned stand-in pointer: validation never dereferences it


def test_entry_points_declared_bound_and_exported():
    from sparse_vae import _native
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'svae.h')).read(), flags=re.S)
    for n in NAMES + ('svae_latent_topk_ws_bytes',):
        assert re.search(r'\b%s\s*\(' % n, hdr), n
        assert n in _native.EXPORTED and hasattr(_native.lib, n), n
    assert re.search(r'SVAE_LATENT_L2 = 0, SVAE_LATENT_COSINE = 1, SVAE_LATENT_KL = 2', hdr)
    assert (_native.LATENT_L2, _native.LATENT_COSINE, _native.LATENT_KL) == (0, 1, 2)
    assert '#define SVAE_LATENT_MAX_BLOCKS 1024' in hdr and _native.LATENT_MAX_BLOCKS == 1024
    assert _native.lib.svae_latent_topk_ws_bytes(3, 10) == 3 * 1024 * 10 * 8


def _topk(metric=0, Q=1, N=100, Z=64, k=10, q=(P, P, P, P), c=(P, P, P, P), ws=P, ws_bytes=None, out=(P, P)):
    from sparse_vae import _native
    if ws_bytes is None:
        ws_bytes = max(Q, 1) * 1024 * max(k, 1) * 8
    return _native.lib.svae_latent_topk(metric, *q, Q, *c, N, Z, k, ws, ws_bytes, *out, None)


def _scores(metric=0, Q=1, N=100, Z=64, q=(P, P, P, P), c=(P, P, P, P), out=P):
    from sparse_vae import _native
    return _native.lib.svae_latent_scores(metric, *q, Q, *c, N, Z, out, None)


@pytest.mark.parametrize('kw', [dict(Z=6), dict(Z=260), dict(Z=0), dict(k=0), dict(k=65), dict(k=11, N=10),
                                dict(metric=3), dict(metric=-1), dict(Q=0), dict(N=0),
                                dict(q=(None, P, P, P)), dict(c=(None, P, P, P)), dict(ws=None), dict(ws_bytes=8),
                                dict(out=(None, P)), dict(out=(P, None)), dict(q=(P + 4, P, P, P)),
                                dict(metric=1, c=(P, P, P, None)), dict(metric=2, c=(P, None, P, P)),
                                dict(metric=2, q=(P, None, P, P))])
def test_topk_rejects_bad_arguments_without_launch(kw):
    assert _topk(**kw) == 1


@pytest.mark.parametrize('kw', [dict(Z=6), dict(Z=260), dict(metric=3), dict(Q=0), dict(N=0), dict(out=None),
                                dict(q=(None, P, P, P)), dict(c=(None, P, P, P)), dict(metric=2, c=(P, P, None, P))])
def test_scores_rejects_bad_arguments_without_launch(kw):
    assert _scores(**kw) == 1


def test_prepare_rejects_bad_arguments_without_launch():
    from sparse_vae import _native
    f = _native.lib.svae_latent_prepare
    assert f(None, P, P, P, P, 10, 64, None) == 1
    assert f(P, P, P, None, P, 10, 64, None) == 1
    assert f(P, P, P, P, P, 10, 6, None) == 1
    assert f(P, P, P, P, P, 10, 260, None) == 1
    assert f(P, P, P, P, P, 0, 64, None) == 1
    assert _native.lib.svae_latent_topk_ws_bytes(1, 65) == 0


def _posteriors(n, Z=8, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, Z, generator=g), torch.rand(n, Z, generator=g) + 0.1


def test_index_bookkeeping_across_growth():
    from sparse_vae import LatentIndex
    index = LatentIndex(8)
    assert len(index) == 0 and index.titles == []
    loc, scale = _posteriors(3000)
    index.add(loc[:10], scale[:10])                                      # [B, Z], default titles
    index.add(loc[10:1500].unsqueeze(1), scale[10:1500].unsqueeze(1),    # [B, 1, Z], grows past the first block
              [f'doc {i}' for i in range(10, 1500)])
    caps = {index._cap}
    for lo in range(1500, 3000, 100):                                    # a gather loop: few reallocations
        index.add(loc[lo:lo + 100], scale[lo:lo + 100])
        caps.add(index._cap)
    assert len(index) == 3000 and len(caps) <= 3
    assert torch.equal(index.loc, loc) and torch.equal(index.scale, scale)
    assert index.titles[:10] == [str(i) for i in range(10)] and index.titles[10] == 'doc 10'
    assert index.titles[1500] == '1500' and len(index.titles) == 3000
    assert index.row_of('doc 77') == 77 and index.row_of('2999') == 2999 and index.row_of('nope') is None
    with pytest.raises(ValueError):
        index.add(loc[:2], scale[:2], ['one title'])
    with pytest.raises(ValueError):
        index.add(torch.zeros(2, 12), torch.ones(2, 12))
    with pytest.raises(ValueError):
        LatentIndex(6)


def test_index_save_load_roundtrip(tmp_path):
    from sparse_vae import LatentIndex
    loc, scale = _posteriors(37, Z=64, seed=3)
    titles = [f'Article {i} é' for i in range(37)]
    index = LatentIndex(64).add(loc, scale, titles)
    path = tmp_path / 'index.npz'
    index.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert sorted(z.files) == ['loc', 'scale', 'titles']
    back = LatentIndex.load(path, 'cpu')
    assert len(back) == 37 and back.latent_depth == 64
    assert torch.equal(back.loc, loc) and torch.equal(back.scale, scale) and back.titles == titles


def test_cpu_index_refuses_to_search():
    from sparse_vae import LatentIndex
    loc, scale = _posteriors(20)
    index = LatentIndex(8).add(loc, scale)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        index.search(0, k=3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        index.scores((loc[:2], scale[:2]), 'kl')
    with pytest.raises(ValueError):
        index.search(0, metric='manhattan')


def test_pairwise_gaussian_kl_refuses_cpu():
    from torch.distributions.normal import Normal
    from sparse_vae import pairwise_gaussian_kl
    loc, scale = _posteriors(4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pairwise_gaussian_kl(Normal(loc, scale))


def test_encode_refuses_cpu():
    from sparse_vae import TransformerVAE, TransformerVAEHparams, TextDataModule
    m = TransformerVAE(TransformerVAEHparams(d_model=128, num_layers=4, num_heads=8, sparse_self_attention=False),
                       device='cpu')
    batch = TextDataModule(dataset_name='synthetic', seq_len=128, batch_size=2).synthetic_batch(0)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m.encode(batch)


def test_collate_keeps_titles():
    """Real-data batches carry their documents' titles for gather_latents (a dataset without the column: no key)."""
    from sparse_vae import TextDataModule
    dm = TextDataModule(dataset_name='synthetic')
    docs = [{'text': np.arange(3, 9, dtype=np.uint16), 'num_tokens': 6, 'num_bytes': 20, 'title': 'Anarchism'},
            {'text': np.arange(3, 7, dtype=np.uint16), 'num_tokens': 4, 'num_bytes': 11, 'title': 'Autism'}]
    assert dm.collate(docs)['title'] == ['Anarchism', 'Autism']
    assert 'title' not in dm.collate([{k: v for k, v in d.items() if k != 'title'} for d in docs])


def _script(name):
    spec = importlib.util.spec_from_file_location(name + '_script', os.path.join(ROOT, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_gather_latents_parser():
    ap = _script('gather_latents').build_parser()
    a = ap.parse_args(['--preset', 'tiny', '--weights', 'w.pt', '--out', 'o.npz', 'data.batch_size=4', 'model.d_model=128'])
    assert (a.preset, a.weights, a.out, a.split) == ('tiny', 'w.pt', 'o.npz', 'test')
    assert a.overrides == ['data.batch_size=4', 'model.d_model=128'] and a.max_batches is None
    a = ap.parse_args(['--out', 'o.npz', '--split', 'train', '--max-batches', '3'])
    assert a.split == 'train' and a.max_batches == 3 and a.weights is None
    with pytest.raises(SystemExit):
        ap.parse_args(['--preset', 'tiny'])                # --out is required


def test_knn_parser_and_query_resolution():
    knn = _script('knn')
    a = knn.build_parser().parse_args(['idx.npz', '--query', 'Anarchism', '--query', '12'])
    assert (a.index, a.query, a.k) == ('idx.npz', ['Anarchism', '12'], 10)
    assert knn.build_parser().parse_args(['idx.npz']).query == []
    assert knn.build_parser().parse_args(['idx.npz', '-k', '5']).k == 5
    from sparse_vae import LatentIndex
    loc, scale = _posteriors(5)
    index = LatentIndex(8).add(loc, scale, ['a', 'b', '4', 'd', 'e'])
    assert knn.resolve(index, 'b') == 1 and knn.resolve(index, '4') == 2       # a title wins over a row number
    assert knn.resolve(index, '3') == 3 and knn.resolve(index, '9') is None and knn.resolve(index, 'zzz') is None
    assert [m for m, _ in knn.TABLES] == ['l2', 'cosine', 'kl']
