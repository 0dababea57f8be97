"""Latent index on the GPU: svae_latent_prepare / _scores / _topk against the float64 restatement of tests/latent_ref.py,
and the Python surface above them (LatentIndex, pairwise_gaussian_kl, TransformerVAE.encode, gather_latents).

Inputs are f32; the reference is computed in float64 from those same f32 values. Score bound per entry:
|err| <= 4 (Z + 8) 2^-24 A, A the float64 sum of the absolute values of the score's terms (latent_ref.bound)."""
import functools

import numpy as np
import pytest
import torch

import latent_ref as R

pytestmark = pytest.mark.gpu

DEV = torch.device('cuda', 0)
QMAX = 9


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class Case:
    """A seeded corpus (N rows) and QMAX queries on the device, prepared, with the float64 scores per metric."""

    def __init__(self, N, Z, integer=False, identical=False):
        from sparse_vae import kernels as K
        self.N, self.Z = N, Z
        self.mu, self.scale = R.random_posteriors(N, Z, 1000 + N + Z, integer=integer)
        if identical:
            self.mu[:], self.scale[:] = self.mu[0], self.scale[0]
        self.q_mu, self.q_scale = R.random_posteriors(QMAX, Z, 77 + Z, integer=integer)
        self.d_mu, self.d_scale = _t(self.mu), _t(self.scale)
        self.d_q_mu, self.d_q_scale = _t(self.q_mu), _t(self.q_scale)
        self.prep = K.latent_prepare(self.d_mu, self.d_scale)
        self.q_prep = K.latent_prepare(self.d_q_mu, self.d_q_scale)
        self._ref = {}

    def ref(self, metric):
        if metric not in self._ref:
            self._ref[metric] = R.scores64(metric, self.q_mu, self.q_scale, self.mu, self.scale)
        return self._ref[metric]

    def operands(self, Q, N=None):
        N = self.N if N is None else N
        iv, ld, inn = self.prep
        _, qld, qin = self.q_prep
        return ((self.d_q_mu[:Q], self.d_q_scale[:Q], qld[:Q], qin[:Q]),
                (self.d_mu[:N], iv[:N], ld[:N], inn[:N]))


@functools.lru_cache(maxsize=None)
def case(N, Z, integer=False, identical=False):
    return Case(N, Z, integer, identical)


# ---------------------------------------------------------------------------------------------------- prepare / scores
@pytest.mark.parametrize('Z', [4, 32, 64, 128, 256])
def test_prepare_matches_float64(Z):
    c = case(1000, Z)
    iv, ld, inn = (t.cpu().double().numpy() for t in c.prep)
    mu, s = c.mu.astype(np.float64), c.scale.astype(np.float64)
    np.testing.assert_allclose(iv, 1.0 / s ** 2, rtol=4 * R.EPS24, atol=0)
    assert np.all(np.abs(ld - np.log(s).sum(-1)) <= (Z + 8) * R.EPS24 * np.abs(np.log(s)).sum(-1))
    np.testing.assert_allclose(inn, 1.0 / np.sqrt((mu ** 2).sum(-1)), rtol=(Z + 8) * R.EPS24, atol=0)


@pytest.mark.parametrize('metric', R.METRICS)
@pytest.mark.parametrize('Z', [4, 32, 64, 128, 256])
def test_scores_match_float64(metric, Z):
    """N in {1, 63, 65, 1000} x Q in {1, 3, 9} (the query-tile tail) on prefixes of one seeded corpus."""
    from sparse_vae import kernels as K
    c = case(1000, Z)
    ref, A = c.ref(metric)
    for N in (1, 63, 65, 1000):
        for Q in (1, 3, 9):
            q, cp = c.operands(Q, N)
            got = K.latent_scores(metric, q, cp).cpu().double().numpy()
            err = np.abs(got - ref[:Q, :N])
            lim = R.bound(A[:Q, :N], Z)
            print(f'{metric} Z={Z} N={N} Q={Q}: max err / bound = {np.max(err / np.maximum(lim, 1e-300)):.4f}')
            assert np.all(err <= lim), (metric, Z, N, Q, float(np.max(err / np.maximum(lim, 1e-300))))


# ---------------------------------------------------------------------------------------------------- top-k
def _check_topk(c, metric, N, Q, k):
    from sparse_vae import kernels as K
    q, cp = c.operands(Q, N)
    scores, idx = K.latent_topk(metric, q, cp, k)
    dense = K.latent_scores(metric, q, cp)
    scores, idx, dense = scores.cpu().numpy(), idx.cpu().numpy(), dense.cpu().numpy()
    ref, A = c.ref(metric)
    ref, lim = ref[:Q, :N], R.bound(A[:Q, :N], c.Z)
    largest = R.LARGEST[metric]
    assert scores.shape == (Q, k) and idx.shape == (Q, k) and idx.dtype == np.int32
    for qi in range(Q):
        ids, sc = idx[qi], scores[qi]
        assert ids.min() >= 0 and ids.max() < N and len(set(ids.tolist())) == k, (metric, N, Q, k, qi)
        assert np.all(np.diff(sc) <= 0) if largest else np.all(np.diff(sc) >= 0), (metric, N, Q, k, qi)
        assert np.array_equal(sc.view(np.uint32), dense[qi, ids].view(np.uint32)), (metric, N, Q, k, qi)
        key = -ref[qi] if largest else ref[qi]              # smaller key = better
        kth = R.stable_topk(ref[qi], k, largest)[k - 1]
        slack = lim[qi] + lim[qi, kth]
        assert np.all(key[ids] <= key[kth] + slack[ids]), (metric, N, Q, k, qi)
        must = np.nonzero(key < key[kth] - slack)[0]
        assert set(must.tolist()) <= set(ids.tolist()), (metric, N, Q, k, qi)


@pytest.mark.parametrize('metric', R.METRICS)
@pytest.mark.parametrize('N', [1, 64, 65, 4097, 70001])
def test_topk_general(metric, N):
    c = case(N, 64)
    for k in (1, 10, 64):
        if k > N:
            continue
        for Q in (1, 9):
            _check_topk(c, metric, N, Q, k)


@pytest.mark.parametrize('metric', R.METRICS)
def test_topk_general_z32(metric):
    _check_topk(case(4097, 32), metric, 4097, 9, 10)


@pytest.mark.parametrize('metric', R.METRICS)
@pytest.mark.parametrize('Z', [68, 128, 160, 200, 256])
def test_topk_wide_latents(metric, Z):
    """Z > 64 runs phase 1's other form (queries re-read from LDS, 4 or 2 row groups per wave and iteration): 2, 2, 3, 4
    and 4 chunks per lane; Z = 68, 160 and 200 leave the last chunk partly masked."""
    for N in (65, 4097):
        c = case(N, Z)
        for k in (10, 64):
            _check_topk(c, metric, N, QMAX, k)


@pytest.mark.parametrize('metric', R.METRICS)
def test_ties_across_workgroups_wide_latents(metric):
    from sparse_vae import kernels as K
    c = case(70001, 128, identical=True)
    q, cp = c.operands(2)
    scores, idx = K.latent_topk(metric, q, cp, 64)
    assert torch.equal(idx.cpu(), torch.arange(64, dtype=torch.int32).expand(2, 64))
    assert torch.equal(scores, scores[:, :1].expand(2, 64))


@pytest.mark.parametrize('N', [4097, 70001])
def test_topk_exact_with_ties(N):
    """Integer means under L2: every f32 score is exact, ties are plentiful, so the indices must be exactly the first k
    of a stable float64 argsort."""
    from sparse_vae import kernels as K
    c = case(N, 64, integer=True)
    ref, _ = c.ref('l2')
    q, cp = c.operands(QMAX)
    scores, idx = K.latent_topk('l2', q, cp, 64)
    scores, idx = scores.cpu().numpy(), idx.cpu().numpy()
    for qi in range(QMAX):
        want = R.stable_topk(ref[qi], 64, False)
        assert len(np.unique(ref[qi][want])) < 64          # the case does contain ties
        assert np.array_equal(idx[qi], want), qi
        assert np.array_equal(scores[qi].astype(np.float64), ref[qi][want]), qi


@pytest.mark.parametrize('metric', R.METRICS)
def test_ties_across_workgroups(metric):
    """70,001 identical rows: every score ties, in every workgroup; the first 64 rows win."""
    from sparse_vae import kernels as K
    c = case(70001, 64, identical=True)
    q, cp = c.operands(2)
    scores, idx = K.latent_topk(metric, q, cp, 64)
    assert torch.equal(idx.cpu(), torch.arange(64, dtype=torch.int32).expand(2, 64))
    assert torch.equal(scores, scores[:, :1].expand(2, 64))


@pytest.mark.parametrize('metric', R.METRICS)
def test_small_corpus_has_no_sentinels(metric):
    from sparse_vae import kernels as K
    c = case(65, 64)
    q, cp = c.operands(QMAX, 3)
    scores, idx = K.latent_topk(metric, q, cp, 3)
    assert torch.equal(idx.sort(dim=1).values.cpu(), torch.arange(3, dtype=torch.int32).expand(QMAX, 3))
    assert torch.isfinite(scores).all()


def test_nan_rows_rank_last():
    """A NaN score (only from NaN input) never displaces a number."""
    from sparse_vae import kernels as K
    mu, scale = R.random_posteriors(300, 64, 5)
    mu[::3] = np.nan
    d_mu, d_scale = _t(mu), _t(scale)
    prep = K.latent_prepare(d_mu, d_scale)
    c = case(65, 64)
    q = c.operands(2)[0]
    for metric in R.METRICS:
        scores, idx = K.latent_topk(metric, q, (d_mu, *prep), 64)
        assert torch.isfinite(scores).all() and (idx % 3 != 0).all(), metric
    scores, idx = K.latent_topk('l2', q, (d_mu[:6], *(t[:6] for t in prep)), 6)
    assert torch.isfinite(scores[:, :4]).all() and torch.isnan(scores[:, 4:]).all()
    assert torch.equal(idx[:, 4:].cpu(), torch.tensor([[0, 3], [0, 3]], dtype=torch.int32))


# ---------------------------------------------------------------------------------------------------- Python surface
def _index(c):
    from sparse_vae import LatentIndex
    index = LatentIndex(c.Z)
    for lo, hi in ((0, 700), (700, 701), (701, c.N)):      # grows across adds
        index.add(c.d_mu[lo:hi], c.d_scale[lo:hi].unsqueeze(1))
    return index


def test_search_by_row_returns_the_row_first():
    c = case(4097, 64)
    index = _index(c)
    assert len(index) == c.N and torch.equal(index.loc, c.d_mu) and torch.equal(index.scale, c.d_scale)
    rows = torch.tensor([0, 5, 4096], device=DEV)
    scores, idx = index.search(rows, k=10, metric='l2')
    assert idx.dtype == torch.int64 and idx.shape == (3, 10)
    assert torch.equal(idx[:, 0], rows) and (scores[:, 0] == 0).all()
    scores, idx = index.search(rows, k=10, metric='kl')
    assert torch.equal(idx[:, 0], rows)
    _, A = R.scores64('kl', c.mu[[0, 5, 4096]], c.scale[[0, 5, 4096]], c.mu[[0, 5, 4096]], c.scale[[0, 5, 4096]])
    assert np.all(np.abs(scores[:, 0].cpu().double().numpy()) <= R.bound(np.diag(A), c.Z))
    s1, i1 = index.search(5, k=3, metric='cosine')
    assert i1.shape == (1, 3) and i1[0, 0].item() == 5 and abs(s1[0, 0].item() - 1.0) < 1e-5
    # a Normal and a (loc, scale) pair are the same query; the dense matrix carries the same bits
    from torch.distributions.normal import Normal
    qn = Normal(c.d_q_mu[:3].unsqueeze(1), c.d_q_scale[:3].unsqueeze(1), validate_args=False)
    sa, ia = index.search(qn, k=7, metric='kl')
    sb, ib = index.search((c.d_q_mu[:3], c.d_q_scale[:3]), k=7, metric='kl')
    assert torch.equal(sa, sb) and torch.equal(ia, ib)
    assert torch.equal(index.scores(qn, 'kl').gather(1, ia), sa)


@pytest.mark.parametrize('B', [5, 33])
def test_pairwise_gaussian_kl(B):
    from torch.distributions import kl_divergence
    from torch.distributions.normal import Normal
    from sparse_vae import pairwise_gaussian_kl
    mu, scale = R.random_posteriors(B, 64, 300 + B)
    got = pairwise_gaussian_kl(Normal(_t(mu).unsqueeze(1), _t(scale).unsqueeze(1), validate_args=False))
    assert got.shape == (B, B)
    m, s = torch.from_numpy(mu).double(), torch.from_numpy(scale).double()
    want = kl_divergence(Normal(m[:, None], s[:, None]), Normal(m[None], s[None])).sum(-1)     # [p, q] = KL(p || q)
    _, A = R.scores64('kl', mu, scale, mu, scale)
    err = (got.cpu().double() - want).abs().numpy()
    assert np.all(err <= R.bound(A, 64)), float(np.max(err / R.bound(A, 64)))


@functools.lru_cache(maxsize=None)
def _tiny_model():
    from sparse_vae import TransformerVAE, TransformerVAEHparams
    torch.manual_seed(11)
    model = TransformerVAE(TransformerVAEHparams(d_model=128, num_layers=4, num_heads=8, latent_depth=64,
                                                 sparse_self_attention=False), device=DEV)
    model.initialize_weights()
    model.eval()
    return model


def _batch(index, B):
    from sparse_vae import TextDataModule
    dm = TextDataModule(dataset_name='synthetic', seq_len=256, batch_size=B, padded=True)
    return dm.synthetic_batch(index, device=DEV)


def test_encode_equals_predict():
    """The same encoder kernels at dropout 0: bit-equal."""
    model = _tiny_model()
    batch = _batch(0, 4)
    q = model.encode(batch)
    p = model.predict(batch)
    assert q.loc.shape == (4, 1, 64) and q.scale.shape == (4, 1, 64)
    assert torch.equal(q.loc, p.loc) and torch.equal(q.scale, p.scale)


def test_gather_latents_save_load_search(tmp_path):
    from sparse_vae import LatentIndex, gather_latents
    model = _tiny_model()
    batches = [_batch(i, B) for i, B in enumerate((3, 5, 2))]
    index = gather_latents(model, batches)
    enc = [model.encode(b) for b in batches]
    assert len(index) == 10 and index.titles == [str(i) for i in range(10)]
    assert torch.equal(index.loc, torch.cat([e.loc[:, 0] for e in enc]))
    assert torch.equal(index.scale, torch.cat([e.scale[:, 0] for e in enc]))
    path = tmp_path / 'latents.npz'
    index.save(path)
    loaded = LatentIndex.load(path, DEV)
    assert torch.equal(loaded.loc, index.loc) and torch.equal(loaded.scale, index.scale)
    assert loaded.titles == index.titles
    for metric in R.METRICS:
        s0, i0 = index.search(0, k=10, metric=metric)
        s1, i1 = loaded.search(0, k=10, metric=metric)
        assert torch.equal(s0, s1) and torch.equal(i0, i1), metric


def test_gather_latents_uses_the_batches_titles():
    from sparse_vae import gather_latents
    model = _tiny_model()
    batches = []
    for i, B in enumerate((2, 3)):
        b = dict(_batch(i, B))
        b['title'] = [f'doc {i}.{j}' for j in range(B)]
        batches.append(b)
    index = gather_latents(model, batches)
    assert index.titles == ['doc 0.0', 'doc 0.1', 'doc 1.0', 'doc 1.1', 'doc 1.2']
    assert index.row_of('doc 1.1') == 3


def test_row_index_queries_are_validated():
    c = case(65, 64)
    index = _index(c)
    s_int, i_int = index.search(7, k=3)
    s_np, i_np = index.search(np.int64(7), k=3)
    s_cpu, i_cpu = index.search(torch.tensor([7]), k=3)
    assert torch.equal(i_int, i_np) and torch.equal(i_int, i_cpu) and torch.equal(s_int, s_np)
    for bad in (65, -1, np.int64(65), torch.tensor([0, 65]), torch.tensor([-1])):
        with pytest.raises(IndexError):
            index.search(bad, k=3)
    # a device tensor is not read back: out-of-range rows are clamped, nothing asserts on the device
    _, i_dev = index.search(torch.tensor([-5, 7, 1000], device=DEV), k=1)
    assert i_dev[:, 0].tolist() == [0, 7, 64]


def _script(name):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name + '_script', os.path.join(root, name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_scripts_end_to_end_on_synthetic_data(tmp_path, capsys):
    """gather_latents.py on the synthetic data mode, then knn.py on its output: main(argv) of both."""
    out = str(tmp_path / 'tiny.npz')
    index = _script('gather_latents').main(['--preset', 'tiny', '--out', out, '--max-batches', '2'])
    assert len(index) == 128 and index.titles[:2] == ['0', '1']
    capsys.readouterr()
    knn = _script('knn')
    assert knn.main([out, '--query', '5', '--query', 'no such article', '-k', '4']) == 0
    text = capsys.readouterr().out
    for _, heading in knn.TABLES:
        assert text.count(heading) == 1
    rows = [ln for ln in text.splitlines() if ' - ' in ln]
    assert len(rows) == 12 and rows[0].split(' - ') == ['5'.ljust(len(rows[0].split(' - ')[0])), '0.0']
    assert all(r.split(' - ')[0].strip() == '5' for r in (rows[0], rows[4], rows[8]))
    assert "'no such article' is neither a title nor a row number" in text
    with pytest.raises(SystemExit):
        knn.main([out, '--query', '5', '-k', '65'])


def test_scores_beyond_one_launch_of_query_tiles():
    """More query tiles than a grid's y dimension holds (65535 tiles of 8): the entry point loops."""
    from sparse_vae import kernels as K
    Q = 65535 * 8 + 5
    q_mu, q_scale = R.random_posteriors(Q, 4, 9)
    mu, scale = R.random_posteriors(2, 4, 10)
    d_q, d_m, d_s = _t(q_mu), _t(mu), _t(scale)
    got = K.latent_scores('l2', (d_q, None, None, None), (d_m, None, None, None)).cpu().double().numpy()
    want, A = R.scores64('l2', q_mu, q_scale, mu, scale)
    assert got.shape == (Q, 2) and np.all(np.abs(got - want) <= R.bound(A, 4))
