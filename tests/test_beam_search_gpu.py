"""TransformerVAE.beam_search / BeamDecoder end to end on the model of tests/test_decode_gpu.py (d 512, 8 heads,
4 layers, seed 77): one beam against greedy `sample`, graph replay against eager steps, every step's decisions and the
reported log-probabilities against the float64 oracle, and autoencode(num_beams=...)."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_ref as BR  # noqa: E402
import oracle  # noqa: E402
from oracle.params import HParams, TIED_ALIASES, init_params  # noqa: E402

if torch.cuda.is_available():
    from sparse_vae import BeamDecoder, BeamResult, TextDataModule, TransformerVAE, TransformerVAEHparams
    from sparse_vae import score_reconstructions

MODEL = dict(d_model=512, num_heads=8, num_layers=4)
MODEL_SEED = 77
START = 1


@functools.lru_cache(maxsize=None)
def model_params():
    return init_params(HParams(latent_depth=64, kl_weight=1.0, **MODEL), MODEL_SEED)


@functools.lru_cache(maxsize=None)
def model(window):
    mhp = TransformerVAEHparams(latent_depth=64, sparse_self_attention=bool(window), attn_window_size=window or 4,
                                kl_weight=1.0, **MODEL)
    m = TransformerVAE(mhp, device='cuda')
    params = model_params()
    sd = dict(params)
    for alias in TIED_ALIASES:
        sd[alias] = params['input_layer.0.weight']
    m.load_state_dict(sd, strict=True)
    m.eval()
    m.start_token, m.end_token = START, -1
    return m


def latent(B):
    g = torch.Generator().manual_seed(B)
    return torch.randn(B, 1, 64, generator=g)


def with_end(m, end):
    class _Ctx:
        def __enter__(self):
            self.old, m.end_token = m.end_token, end

        def __exit__(self, *a):
            m.end_token = self.old
    return _Ctx()


# ---------------------------------------------------------------------------------------------- one beam = greedy
@pytest.mark.parametrize('window,B,T', [(0, 37, 40), (2, 17, 140)], ids=['dense-B37-T40', 'window2-B17-T140'])
def test_one_beam_without_length_penalty_is_greedy(window, B, T):
    """Same kernels on the same number of rows up to the logits, then the row maximum with the lowest id either way:
    equality, not a tolerance."""
    m, z = model(window), latent(B).cuda()
    want = m.sample(T, B, z=z.clone(), temperature=0.0, repetition_penalty=1.0)
    got = m.beam_search(T, z.clone(), num_beams=1, length_penalty=0.0)
    assert isinstance(got, BeamResult) and got.ids.shape == (B, 1, T - 1) and got.ids.dtype == torch.int64
    assert torch.equal(got.ids[:, 0], want)
    assert (got.lengths == T - 2).all() and torch.equal(got.scores, got.log_probs)


# ---------------------------------------------------------------------------------------------- graph = eager
PS_END = 15248               # chosen on the CPU (see test_step_decisions_match_float64): hypotheses end early with it


@pytest.mark.parametrize('window,B,T', [(0, 5, 40), (2, 3, 140)], ids=['dense-B5-T40', 'window2-B3-T140'])
def test_graph_replay_equals_eager_steps(window, B, T):
    m, z = model(window), latent(B).cuda()
    out = []
    with with_end(m, PS_END):
        for use_graph in (True, False):
            out.append(m.beam_search(T, z.clone(), num_beams=4, length_penalty=1.0, num_return=4, use_graph=use_graph,
                                     return_history=True))
    a, b = out
    assert a.ids.shape == (B, 4, T - 1) and a.scores.shape == (B, 4) and a.lengths.dtype == torch.int32
    assert torch.equal(a.ids, b.ids) and torch.equal(a.lengths, b.lengths)
    assert torch.equal(a.scores.view(torch.int32), b.scores.view(torch.int32))
    assert torch.equal(a.log_probs.view(torch.int32), b.log_probs.view(torch.int32))
    for k in ('parent', 'token'):
        assert torch.equal(a.history[k], b.history[k])
    assert torch.equal(a.history['score'].view(torch.int32), b.history['score'].view(torch.int32))
    assert (a.scores[:, :-1] >= a.scores[:, 1:]).all()


def test_beam_search_argument_checks():
    m, z = model(0), latent(2).cuda()
    for kw in (dict(num_beams=0), dict(num_beams=17), dict(num_beams=2, num_return=3), dict(num_beams=2, num_return=0)):
        with pytest.raises(ValueError):
            m.beam_search(12, z, **kw)
    old = m.hparams.kl_weight
    m.hparams.kl_weight = 0.5
    try:
        with pytest.raises(RuntimeError, match='kl_weight'):
            m.beam_search(12, z)
    finally:
        m.hparams.kl_weight = old


# ---------------------------------------------------------------------------------------------- decisions vs float64
PS_B, PS_W, PS_T, PS_ALPHA = 3, 4, 14, 1.0


def decision_latent():
    """Three nearby latents (one draw of scale 4 plus 0.08 of noise each), so that one end token is among the likely
    continuations of every document."""
    base = 4.0 * torch.randn(PS_B, 1, 64, generator=torch.Generator().manual_seed(10))[2:3]
    return base + 0.08 * torch.randn(PS_B, 1, 64, generator=torch.Generator().manual_seed(5))


def oracle_passes(prefix, zrows):
    """Teacher forcing over the id prefixes [n, c]: -> (float64 logits [n, c, V], max |f32 pass - f64 pass|)."""
    hp = HParams(latent_depth=64, kl_weight=1.0, attn_window=0, **MODEL)
    p32 = model_params()
    p64 = oracle_passes.p64 = getattr(oracle_passes, 'p64', None) or {k: v.double() for k, v in p32.items()}
    ids = torch.as_tensor(prefix, dtype=torch.long)
    with torch.no_grad():
        x32 = torch.nn.functional.embedding(ids, p32['input_layer.0.weight'])
        l32 = oracle.reconstruct(p32, x32, zrows, None, hp)
        l64 = oracle.reconstruct(p64, x32.double(), zrows.double(), None, hp)
    return l64, float((l32.double() - l64).abs().max())


def walk_live(cands, W, end):
    """The live rows a step selects from its sorted candidates: -> ([(parent, token)], candidates consumed)."""
    live, walked = [], 0
    for rank, (s, w, tok, *_) in enumerate(cands[:2 * W]):
        if len(live) == W:
            break
        walked = rank + 1
        if tok != end:
            live.append((w, tok))
    return live, walked


def step_decisions(parent, token, z, B, W, T, end):
    """Rebuild the live prefixes from a decode's history and judge every step against the float64 oracle.
    -> (list of (step, doc, margin, agrees), e_ref, lse_err, prefixes of the last step)."""
    Rr = B * W
    zrows = z.repeat_interleave(W, dim=0)
    prefix = np.full((Rr, 1), START, np.int64)
    live = np.zeros(Rr, bool)
    live[::W] = True
    open_docs = np.ones(B, bool)
    out, e_ref, lse_err = [], 0.0, 0.0
    for c in range(1, T - 1):
        open_docs &= (parent[c].reshape(B, W) >= 0).any(axis=1)         # a done document writes no history
        if not open_docs.any():
            break
        l64, e = oracle_passes(prefix, zrows)
        e_ref = max(e_ref, e)
        logp = torch.log_softmax(l64, dim=-1).numpy()                   # [R, c, V]
        cum = np.array([sum(logp[r, t, prefix[r, t + 1]] for t in range(c - 1)) for r in range(Rr)], np.float64)
        cum[~live] = -np.inf
        for b in np.flatnonzero(open_docs):
            rows = slice(b * W, (b + 1) * W)
            cands = BR.top_candidates(cum[rows], logp[rows, c - 1], W)
            want, walked = walk_live(cands, W, end)
            margin = BR.step_margin([t[0] for t in cands], walked)
            got = [(int(p), int(t)) for p, t in zip(parent[c, rows], token[c, rows]) if p >= 0]
            out.append((c, int(b), margin, got == want))
            for s, w, tok, *_ in cands[:walked]:
                x = l64[b * W + w, c - 1].numpy()
                lse_err = max(lse_err, float(BR.topk_score_bound(x, np.array([tok]), cum[b * W + w])[0]))
        new = np.zeros((Rr, c + 1), np.int64)
        for r in range(Rr):
            b0, p = (r // W) * W, parent[c, r]
            src = b0 + p if (p >= 0 and open_docs[r // W]) else r
            new[r, :c] = prefix[src]
            new[r, c] = token[c, r] if (p >= 0 and open_docs[r // W]) else 0
            live[r] = bool(p >= 0 and open_docs[r // W])
        prefix = new
    return out, e_ref, lse_err


def test_step_decisions_match_float64():
    """Dense, B 3, W 4, T 14. PS_END and the latents were picked on the CPU from beam_search64 runs with the float64
    oracle: every document finishes a hypothesis before T - 2 (lengths 4, 2 and 2), and of the reference's own 36
    step decisions one is unclear (margin / tolerance 0.80; the next smallest is above 1). The random-init model is
    close to uniform over 32768 tokens, so no choice tried left none unclear. The tolerance is
    beam_ref.decision_tol: 2 * step * (16 e_ref + the kernel's own log-sum-exp bound)."""
    B, W, T, end = PS_B, PS_W, PS_T, PS_END
    m, z = model(0), decision_latent()
    with with_end(m, end):
        res = m.beam_search(T, z.cuda(), num_beams=W, length_penalty=PS_ALPHA, num_return=W, return_history=True)
    parent, token = res.history['parent'].cpu().numpy(), res.history['token'].cpu().numpy()
    decisions, e_ref, lse_err = step_decisions(parent, token, z, B, W, T, end)
    unclear = [d for d in decisions if not d[2] > BR.decision_tol(e_ref, lse_err, d[0])]
    wrong = [d for d in decisions if d[2] > BR.decision_tol(e_ref, lse_err, d[0]) and not d[3]]
    print(f'beam decisions: {len(decisions)} steps, {len(unclear)} unclear, e_ref {e_ref:.3e}, lse bound {lse_err:.3e}, '
          f'smallest margin / tolerance {min(d[2] / BR.decision_tol(e_ref, lse_err, d[0]) for d in decisions):.2f}')
    assert not wrong, wrong
    assert len(unclear) * 10 <= len(decisions), (len(unclear), len(decisions))
    # the reported log-probabilities are the float64 sums along the returned ids
    ids, lengths, logp = res.ids.cpu().numpy(), res.lengths.cpu().numpy(), res.log_probs.cpu().numpy().astype(np.float64)
    scores = res.scores.cpu().numpy().astype(np.float64)
    worst = 0.0
    for b in range(B):
        assert any(lengths[b, i] < T - 2 and ids[b, i, lengths[b, i] - 1] == end for i in range(W)), (b, lengths[b])
        for i in range(W):
            n = int(lengths[b, i])
            seq = np.concatenate([[START], ids[b, i, :n]])[None]
            assert (ids[b, i, n:] == 0).all() and (end not in seq[0, :n])
            l64, _ = oracle_passes(seq[:, :n], z[b:b + 1])
            lp = torch.log_softmax(l64, dim=-1).numpy()[0]
            ref = sum(lp[t, seq[0, t + 1]] for t in range(n))
            tol = n * BR.logp_tol(e_ref, lse_err)
            worst = max(worst, abs(logp[b, i] - ref) / tol)
            assert abs(logp[b, i] - ref) <= tol, (b, i, logp[b, i], ref, tol)
            pen = np.float64(np.float32(np.float64(n) ** PS_ALPHA))
            assert abs(scores[b, i] - logp[b, i] / pen) <= 2 * BR.EPS24 * abs(scores[b, i])
    print(f'beam log-probs: worst err / tolerance {worst:.3f}')


# ---------------------------------------------------------------------------------------------- autoencode
def test_autoencode_with_beams():
    T, B = 24, 6
    m = model(0)
    batch = TextDataModule(dataset_name='synthetic', seq_len=20, batch_size=B, padded=True).synthetic_batch(1, device='cuda')
    with with_end(m, PS_END):
        ids, posterior = m.autoencode(batch, max_length=T, num_beams=3)
        want = m.beam_search(T, posterior.loc, num_beams=3)
    assert ids.dtype == torch.int16 and ids.shape == (B, T - 1) and ids.is_cuda
    assert torch.equal(ids.long(), want.ids[:, 0])
    assert torch.equal(m.last_beam_result.scores, want.scores)
    for r in range(B):                                   # zero after the end
        n = int(want.lengths[r, 0])
        assert (ids[r, n:] == 0).all()
    scores = score_reconstructions(ids, ids.clone(), end_token=PS_END)
    assert len(scores) == B
    # without num_beams nothing changed: two calls under one seed agree, and differ from the beam rows
    outs = []
    for _ in range(2):
        torch.manual_seed(99)
        outs.append(m.autoencode(batch, max_length=T)[0])
    assert outs[0].dtype == torch.int16 and outs[0].shape == (B, T - 1) and torch.equal(outs[0], outs[1])
