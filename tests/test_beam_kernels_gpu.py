"""The beam search kernels (csrc/beam.hip), each called directly and compared with tests/beam_ref.py:

* beam_attn: bit for bit svae_dec_attn with the identity table, and svae_dec_attn on caches gathered through a random
  table; within decode_ref.attn_bound of the float64 softmax over the keys the table names; only the row's own
  cache cells at p are written. Caches are NaN wherever no visible key lives.
* beam_topk: ids exactly the float64 order (value descending, id ascending), planted duplicates lowest id first,
  scores within the bound derived in beam_ref.py, dead rows and rows of done documents untouched.
* beam_select / beam_finalize: scores that are multiples of 1/8 (every sum and comparison exact; the only rounded
  operation, s / l^alpha, is one IEEE f32 division on both sides), whole decodes compared exactly, state by state.
* the chain beam_topk -> beam_select -> beam_finalize on a Markov model against beam_search64.
"""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import beam_ref as BR  # noqa: E402
import decode_ref as R  # noqa: E402

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae.decoding import BeamState

f32 = torch.float32
POISON = 0x7FC0BEEF          # a quiet NaN with a payload: untouched cells are recognised bit for bit


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return t if dtype is None else t.to(dtype)


def poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device='cuda').view(f32)


def cur_tensor(c):
    return torch.tensor([c], dtype=torch.int32, device='cuda')


def bits(t):
    return t.contiguous().view(torch.int32)


# ============================================================================================== beam_attn
ATTN_HEADS = {16: 5, 64: 3, 96: 2, 128: 4}
ATTN_B, ATTN_W, ATTN_T = 3, 4, 140


@pytest.mark.parametrize('window', [0, 2])
@pytest.mark.parametrize('hd', [16, 64, 96, 128])
def test_beam_attn(hd, window):
    B, W, T, H = ATTN_B, ATTN_W, ATTN_T, ATTN_HEADS[hd]
    Rr, d, scale = B * W, H * hd, hd ** -0.5
    worst = {}
    for p in (0, 1, 37, 139):
        rng = np.random.default_rng(1000 * hd + 10 * window + p)
        vis = R.visible_keys(p, window)
        old = vis[vis < p]
        kc = np.full((Rr, H, T, hd), np.nan, dtype=np.float32)       # NaN beyond p and at every invisible key
        vc = np.full((Rr, H, T, hd), np.nan, dtype=np.float32)
        kc[:, :, old] = 0.5 * rng.standard_normal((Rr, H, old.size, hd)).astype(np.float32)
        vc[:, :, old] = rng.standard_normal((Rr, H, old.size, hd)).astype(np.float32)
        q = rng.standard_normal((Rr, H, hd)).astype(np.float32)
        kp = 0.5 * rng.standard_normal((Rr, H, hd)).astype(np.float32)
        vp = rng.standard_normal((Rr, H, hd)).astype(np.float32)
        qkv = dev(np.concatenate([a.reshape(Rr, d) for a in (q, kp, vp)], axis=1))
        kc_d, vc_d, cur = dev(kc), dev(vc), cur_tensor(p + 1)
        doc0 = (np.arange(Rr) // W) * W
        ident = np.broadcast_to((np.arange(Rr) % W)[:, None], (Rr, T)).astype(np.uint8)
        table = rng.integers(0, W, size=(Rr, T)).astype(np.uint8)    # each column a random map within the document

        def run_beam(anc):
            k2, v2, O = kc_d.clone(), vc_d.clone(), poisoned(Rr, d)
            K.beam_attn(qkv, k2, v2, dev(anc), O, Rr, W, H, hd, T, cur, window)
            return O, k2, v2

        def run_dec(k_in, v_in):
            k2, v2, O = k_in.clone(), v_in.clone(), poisoned(Rr, d)
            K.dec_attn(qkv, k2, v2, O, Rr, H, hd, T, cur, window)
            return O, k2, v2

        # identity table: dec_attn bit for bit, outputs and caches
        Oi, ki, vi = run_beam(ident)
        O0, k0, v0 = run_dec(kc_d, vc_d)
        assert torch.equal(bits(Oi), bits(O0)) and torch.equal(bits(ki), bits(k0)) and torch.equal(bits(vi), bits(v0))
        # random table: dec_attn on the caches gathered through it
        rows = dev(doc0[:, None] + table.astype(np.int64))                       # [R, T] source cache rows
        cols = torch.arange(T, device='cuda')[None].expand(Rr, T)
        kg = kc_d[rows, :, cols].permute(0, 2, 1, 3).contiguous()                # [R, T, H, hd] -> [R, H, T, hd]
        vg = vc_d[rows, :, cols].permute(0, 2, 1, 3).contiguous()
        Ob, kb, vb = run_beam(table)
        Og, _, _ = run_dec(kg, vg)
        assert torch.equal(bits(Ob), bits(Og))
        # only the row's own cells at p were written, with its k | v slices bit for bit
        for got, orig, new in ((kb, kc_d, kp), (vb, vc_d, vp)):
            assert torch.equal(bits(got[:, :, p]), bits(dev(new)))
            keep = torch.ones(T, dtype=torch.bool, device='cuda')
            keep[p] = False
            assert torch.equal(bits(got[:, :, keep]), bits(orig[:, :, keep]))
        got = Ob.cpu().numpy().reshape(Rr, H, hd).astype(np.float64)
        assert np.isfinite(got).all(), 'a key or value outside the visible set of the table was read'
        w = 0.0
        for r in range(Rr):
            for h in range(H):
                (ref, A, S, spread), n = BR.attn64(q[r, h], kc, vc, table[r], doc0[r], h, p, window, kp[r, h], vp[r, h],
                                                   scale)
                assert spread <= 16.0, spread
                w = max(w, float((np.abs(got[r, h] - ref) / R.attn_bound(A, S, n, hd)).max()))
        worst[p] = w
    print(f'beam_attn hd {hd} window {window}: err / bound per p = ' + ', '.join(f'{p}: {w:.3f}' for p, w in worst.items()))
    assert max(worst.values()) <= 1.0, worst


def test_beam_attn_rejects_bad_arguments():
    from sparse_vae._native import lib
    assert lib.svae_beam_attn(16, 48, 16, 16, None, 4, 2, 1, 16, 8, 16, 0, 1.0, 16, 16, None) == 1      # no table
    assert lib.svae_beam_attn(16, 48, 16, 16, 16, 4, 17, 1, 16, 8, 16, 0, 1.0, 16, 16, None) == 1       # W > 16
    assert lib.svae_beam_attn(16, 48, 16, 16, 16, 5, 2, 1, 16, 8, 16, 0, 1.0, 16, 16, None) == 1        # R % W
    assert lib.svae_beam_topk(16, 8, 8, 4, 8, 16, None, 16, 16, None) == 1                              # V < 2W
    assert lib.svae_beam_finalize(16, 16, 2, 2, 8, 16, 16, 16, 16, 16, 16, 16, 3, 16, 16, 16, 16, None) == 1  # n > W


# ============================================================================================== beam_topk
TOPK_ROWS = 5


@pytest.mark.parametrize('W', [1, 4, 16])
@pytest.mark.parametrize('V', [1000, 5000, 32768])
def test_beam_topk(V, W):
    C, rows = 2 * W, TOPK_ROWS
    rng = np.random.default_rng(V + W)
    x = (3.0 * rng.standard_normal((rows, V))).astype(np.float32)
    dup = [V - 1, 3, V // 2, 1027 % V]
    x[0, dup] = x[0].max() + 1.0                     # exact duplicates at the top: lowest id first
    x[2, dup] = np.sort(x[2])[-W]                    # and across the rank the beams split at
    cum = np.array([-1.5, -np.inf, 0.0, -7.25, -120.0], dtype=np.float32)
    ndoc = -(-rows // W)
    logits = dev(x)

    def run(done):
        cs, ct = poisoned(rows, C), torch.full((rows, C), POISON, dtype=torch.int32, device='cuda')
        K.beam_topk(logits, V, rows, W, dev(cum), dev(done), cs, ct)
        torch.cuda.synchronize()
        return cs, ct

    cs, ct = run(np.zeros(ndoc, np.uint8))
    worst = 0.0
    for r in range(rows):
        if not cum[r] > -np.inf:                     # a dead row: outputs untouched
            assert (bits(cs[r]) == POISON).all() and (ct[r] == POISON).all()
            continue
        ids, logp, gaps = BR.topk64(x[r], W)
        got_ids = ct[r].cpu().numpy()
        assert np.array_equal(got_ids, ids), (r, got_ids, ids)
        err = np.abs(cs[r].cpu().numpy().astype(np.float64) - (np.float64(cum[r]) + logp))
        worst = max(worst, float((err / BR.topk_score_bound(x[r], ids, np.float64(cum[r]))).max()))
    got0 = ct[0].cpu().numpy()
    assert got0[:min(C, 4)].tolist() == sorted(set(dup))[:min(C, 4)]
    print(f'beam_topk V {V} W {W}: worst err / bound {worst:.3f}')
    assert worst <= 1.0, worst
    # the last document done: its rows keep the poison, the others are written as before
    done = np.zeros(ndoc, np.uint8)
    done[-1] = 1
    cs2, ct2 = run(done)
    for r in range(rows):
        if r // W == ndoc - 1 or not cum[r] > -np.inf:
            assert (bits(cs2[r]) == POISON).all() and (ct2[r] == POISON).all()
        else:
            assert torch.equal(bits(cs2[r]), bits(cs[r])) and torch.equal(ct2[r], ct[r])


# ============================================================================================== beam_select / finalize
SEL_B, SEL_T, SEL_V, SEL_END = 5, 12, 24, 7
SEL_ALPHA = {1: 1.0, 3: 0.6, 8: 0.3}


def select_candidates(rng, docs, c, W, T):
    """One step's candidate arrays for the reference's current state: scores cum - k / 8 (k = 1..10, so ties across
    beams are common), tokens distinct within a row, the end token in about a third of the rows; at the last step the
    best live row of every open document ends at rank 0 (a hypothesis ending on the last allowed position). Dead rows
    and the rows of done documents carry NaN scores and out-of-range tokens: they must not be read."""
    C = 2 * W
    score = np.full((len(docs), W, C), np.nan, dtype=np.float32)
    tok = np.full((len(docs), W, C), 1 << 30, dtype=np.int32)
    for b, d in enumerate(docs):
        if d.done:
            continue
        for w in range(W):
            if not d.cum[w] > -np.inf:
                continue
            # document b's scores fall b + 1 eighths at a time: the steep ones are done early, the flat ones never
            drop = (b + 1) * rng.integers(1, 11, size=C)
            score[b, w] = np.float32(d.cum[w]) - drop.astype(np.float32) / np.float32(8)
            t = rng.permutation([v for v in range(SEL_V) if v != SEL_END])[:C]
            if rng.random() < 0.5:                  # an end token, more often than not among the row's best
                order = np.argsort(drop, kind='stable')
                t[order[rng.integers(0, min(3, C)) if rng.random() < 0.7 else rng.integers(0, C)]] = SEL_END
            order = np.lexsort((t, -score[b, w]))   # as beam_topk emits a row: score descending, token ascending
            score[b, w], tok[b, w] = score[b, w][order], t[order]
        if c == T - 2:
            w = int(np.argmax(d.cum))
            score[b, w, 0] += np.float32(0.125)        # (row w stays sorted: its first candidate only gets better)
            tok[b, w, 0] = SEL_END
    return score, tok


def select_reference(W, seed):
    """The whole scenario on the CPU: -> per step (score, tok, snapshot of the reference after the step)."""
    B, T = SEL_B, SEL_T
    alpha = SEL_ALPHA[W]
    pen = BR.len_pen_table(T, alpha)
    rng = np.random.default_rng(seed)
    docs = [BR.Doc(W, T, 1, dtype=np.float32) for _ in range(B)]
    steps = []
    for c in range(1, T - 1):
        score, tok = select_candidates(rng, docs, c, W, T)
        for b, d in enumerate(docs):
            cands = [(score[b, w, k], w, int(tok[b, w, k])) for w in range(W) if d.cum[w] > -np.inf
                     for k in range(2 * W)]
            d.select(cands, c, SEL_END, pen, alpha)
        steps.append((score, tok, [(d.cum.copy(), d.ids.copy(), d.anc.copy(), list(d.pool_score), list(d.pool_logp),
                                    list(d.pool_len), [r.copy() for r in d.pool_ids], d.done,
                                    list(d.history[-1]) if len(d.history) == c else None) for d in docs]))
    return docs, steps, pen


SEL_SEEDS = {1: 0, 3: 27, 8: 27}       # chosen on the CPU so that every rule below fires (the test asserts it)


@pytest.mark.parametrize('W', [1, 3, 8])
def test_beam_select_and_finalize_exact(W):
    B, T, alpha = SEL_B, SEL_T, SEL_ALPHA[W]
    docs, steps, pen = select_reference(W, SEL_SEEDS[W])
    ev = sum((d.events for d in docs), start=__import__('collections').Counter())
    # the scenario covers the rules (checked on the reference, so a change of the generator cannot hollow the test)
    assert ev['end_in'] > 0 and any(n == T - 2 and row[T - 2] == SEL_END
                                    for d in docs for n, row in zip(d.pool_len, d.pool_ids))
    done_at = [next((c + 1 for c, s in enumerate(steps) if s[2][b][7]), None) for b in range(B)]
    if W > 1:
        assert ev['end_drop'] > 0 and ev['replace'] > 0 and ev['reject'] > 0 and ev['tie'] > 0, ev
        assert any(c is not None and c < T - 2 for c in done_at) and any(c is None for c in done_at), done_at
    st = BeamState(B, W, T, 1, SEL_END, alpha, 'cuda', history=True)
    st.len_pen.copy_(dev(pen))
    Rr = B * W
    for c, (score, tok, snap) in enumerate(steps, start=1):
        K.beam_select(dev(score.reshape(Rr, 2 * W)), dev(tok.reshape(Rr, 2 * W)), st)
        K.dec_advance(st.cur)
        torch.cuda.synchronize()
        cum, ids, anc = st.cum.cpu().numpy(), st.ids.cpu().numpy().reshape(B, W, T), st.anc.cpu().numpy().reshape(B, W, T)
        pn, dn = st.pool_n.cpu().numpy(), st.done.cpu().numpy()
        ps, pl, pln = st.pool_score.cpu().numpy(), st.pool_logp.cpu().numpy(), st.pool_len.cpu().numpy()
        pids = st.pool_ids.cpu().numpy()
        hp, ht, hs = (t[c].cpu().numpy().reshape(B, W) for t in (st.hist_parent, st.hist_token, st.hist_score))
        for b, (rcum, rids, ranc, rps, rpl, rpln, rpids, rdone, rhist) in enumerate(snap):
            tag = (W, c, b)
            assert np.array_equal(cum[b].view(np.int32), rcum.astype(np.float32).view(np.int32)), tag
            assert np.array_equal(ids[b], rids) and np.array_equal(anc[b], ranc), tag
            assert pn[b] == len(rps) and bool(dn[b]) == rdone, tag
            n = len(rps)
            assert np.array_equal(ps[b, :n], np.asarray(rps, np.float32)), tag
            assert np.array_equal(pl[b, :n], np.asarray(rpl, np.float32)) and pln[b, :n].tolist() == rpln, tag
            assert all(np.array_equal(pids[b, i], rpids[i]) for i in range(n)), tag
            if rhist is None:                      # done before this step: nothing written
                assert (hp[b] == -1).all() and (ht[b] == -1).all() and np.isneginf(hs[b]).all(), tag
            else:
                assert hp[b].tolist() == [h[0] for h in rhist] and ht[b].tolist() == [h[1] for h in rhist], tag
                assert np.array_equal(hs[b], np.asarray([h[2] for h in rhist], np.float32)), tag
        assert int(st.not_done.item()) == sum(not s[7] for s in snap)
        assert int(st.cur.item()) == c + 1
    for n in sorted({1, W}):
        ids, scores, logp, lengths = (t.cpu().numpy() for t in K.beam_finalize(st, n))
        pools = [d.finalize(pen)[0] for d in docs]
        rids, rs, rl, rlen = BR.result_arrays(pools, n, T)
        assert np.array_equal(ids, rids) and np.array_equal(lengths, rlen)
        assert np.array_equal(scores, rs.astype(np.float32)) and np.array_equal(logp, rl.astype(np.float32))


# ============================================================================================== the kernel chain
CH_V, CH_B, CH_T, CH_END = 1000, 5, 48, 17
# A peaked model (logit scale 16) keeps the candidates of a step apart; the end column is raised by 40. The seeds were
# chosen on the CPU so that the reference leaves no document out. Smallest margin / accumulated bound over the five
# documents, for alpha = 0, 0.6, 1 (a document counts from 2 on):
#   W 1, seed 0: 2249, 2249, 2249  (margins 1.7e-1 .. 8.0e-2, bounds 7.6e-5)
#   W 3, seed 0: 56.5, 19.6, 2.51  (margins 3.0e-3, 3.0e-3, 4.7e-4; bounds 7.4e-5, 1.5e-4, 2.0e-4)
#   W 8, seed 1: 84.4, 4.75, 3.92  (margins 2.9e-3, 7.8e-4, 7.7e-4; bounds 7.8e-5, 1.8e-4, 2.1e-4)
CH_SCALE, CH_BOOST = 16.0, 40.0
CH_SEED = {1: 0, 3: 0, 8: 1}


@functools.lru_cache(maxsize=None)
def chain_table(seed):
    """f32 [V, V] logits; the end token's column is raised so that most hypotheses finish within ~10 steps."""
    rng = np.random.default_rng(seed)
    t = (CH_SCALE * rng.standard_normal((CH_V, CH_V))).astype(np.float32)
    t[:, CH_END] += np.float32(CH_BOOST)
    return t


@functools.lru_cache(maxsize=None)
def chain_reference(W, alpha):
    table = chain_table(CH_SEED[W])
    start = 100 + 7 * np.arange(CH_B)
    return BR.beam_search64(BR.markov_logp_fn(table, bound=True), CH_B, W, CH_T, CH_END, alpha, W, start=start), start


@pytest.mark.parametrize('alpha', [0.0, 0.6, 1.0])
@pytest.mark.parametrize('W', [1, 3, 8])
def test_kernel_chain_on_a_markov_model(W, alpha):
    """beam_topk -> beam_select per step, then beam_finalize, with logits[r] = table[previous token of r]; against
    beam_search64 over the same table. A document counts only if the reference's smallest decision margin is at
    least twice its accumulated error bound (beam_ref: margins of the pool's normalised scores are scaled back by
    their divisor first). The smallest margins of the seeds in use are recorded at CH_SEED above: no document is
    left out."""
    B, T, V = CH_B, CH_T, CH_V
    ref, start = chain_reference(W, alpha)
    clear = ref['margin'] >= 2 * ref['err']
    print(f'chain W {W} alpha {alpha}: margins {ref["margin"]}, bounds {ref["err"]}, lengths {ref["lengths"][:, 0]}')
    assert clear.sum() >= B - B // 5
    table = dev(chain_table(CH_SEED[W]))
    st = BeamState(B, W, T, 1, CH_END, alpha, 'cuda')
    st.ids[:, 0] = dev(np.repeat(start, W))
    Rr = B * W
    for c in range(1, T - 1):
        logits = table[st.ids[:, c - 1]]
        K.beam_topk(logits, V, Rr, W, st.cum, st.done, st.cand_score, st.cand_tok)
        K.beam_select(st.cand_score, st.cand_tok, st)
        K.dec_advance(st.cur)
    ids, scores, logp, lengths = (t.cpu().numpy() for t in K.beam_finalize(st, W))
    worst = 0.0
    for b in np.flatnonzero(clear):
        assert np.array_equal(ids[b], ref['ids'][b]) and np.array_equal(lengths[b], ref['lengths'][b]), b
        tol_lp = ref['err'][b]
        tol_sc = ref['err'][b] + 2 * BR.EPS24 * np.abs(ref['scores'][b])
        assert (np.abs(logp[b] - ref['log_probs'][b]) <= tol_lp).all(), b
        assert (np.abs(scores[b] - ref['scores'][b]) <= tol_sc).all(), b
        worst = max(worst, float((np.abs(logp[b] - ref['log_probs'][b]) / tol_lp).max()))
    print(f'chain W {W} alpha {alpha}: worst log-prob err / bound {worst:.3f}')
    # most documents finished early: the done flag, not the step limit, ended them
    assert (ref['lengths'][:, 0] < T - 2).sum() >= 3
