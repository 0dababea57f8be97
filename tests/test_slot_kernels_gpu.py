"""The per-slot decode kernels (svae_slot_*, csrc/decode.hip), each called directly.

They share their kernel bodies with the svae_dec_* kernels, which tests/test_decode_gpu.py pins to the float64
restatements; so every comparison here is exact (torch.equal) against the dec_* twin:

1. every pos[s] = c and key[s] = s reproduces the twin at cur = c;
2. a batch whose rows sit at different positions equals, row by row, the equal-position calls;
3. idle slots (pos == 0) leave outputs, caches, ids and the result buffer untouched;
4. slot_sample's draws follow the sample number (key), not the slot;
5. slot_sample's bookkeeping (advance, finish on the end token, finish at position T - 2, the int16 result row);
6. slot_refill (sample numbers in slot order, idle when none remain, the initial fill).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from sparse_vae import kernels as K
    from sparse_vae._native import EPI_ROTARY_BF16
    from sparse_vae.engine import rotary_table

f32 = torch.float32
POISON = 0x7FC0BEEF          # a quiet NaN with a payload: untouched cells are recognised bit for bit


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == f32 else t


def same(a, b):
    return torch.equal(bits(a), bits(b))


def poisoned(*shape):
    return torch.full(shape, POISON, dtype=torch.int32, device='cuda').view(f32)


def randn(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).cuda()


def i32(v):
    return torch.as_tensor(v, dtype=torch.int32).reshape(-1).cuda()


POSITIONS = (1, 2, 37, 100)


def mixed_pos(S, seed, choices=POSITIONS):
    g = torch.Generator().manual_seed(seed)
    return torch.tensor(choices)[torch.randint(0, len(choices), (S,), generator=g)].to(torch.int32).cuda()


# ============================================================================================== slot_linear
def linear_case(M, d, split):
    N, Kd = 3 * d, d
    X, W, b = randn(M, Kd, seed=M + d), randn(N, Kd, seed=M + d + 1), randn(N, seed=M + d + 2)
    rot = rotary_table(128, d).cuda()
    part = (lambda: torch.full((16 * M * 4 * d,), float('nan'), device='cuda')) if split else (lambda: None)

    def dec(c):
        Y = poisoned(M, N)
        K.dec_linear(X, W, Y, M, N, Kd, bias=b, epi=EPI_ROTARY_BF16, rot=rot, rot_cols=2 * d, rot_d=d, cur=i32([c]),
                     part=part())
        return Y

    def slot(pos, Y=None):
        Y = poisoned(M, N) if Y is None else Y
        K.slot_linear(X, W, Y, M, N, Kd, bias=b, rot=rot, rot_cols=2 * d, rot_d=d, pos=pos, part=part())
        return Y
    return dec, slot


@pytest.mark.parametrize('split', [False, True], ids=['unsplit', 'workspace'])
@pytest.mark.parametrize('d', [128, 512])
@pytest.mark.parametrize('M', [15, 64, 70])
def test_slot_linear_equals_dec_linear(M, d, split):
    """d 128 never splits (K / 2 < 256); d 512 with the workspace runs 2 splits and the finalize kernel."""
    dec, slot = linear_case(M, d, split)
    for c in (1, 2, 100):
        assert same(slot(i32([c] * M)), dec(c)), c
    # mixed positions, and idle rows that keep their sentinel
    pos = mixed_pos(M, M + d)
    pos[::5] = 0
    Y = slot(pos)
    for c in POSITIONS:
        rows = pos == c
        assert same(Y[rows], dec(c)[rows]), c
    assert (bits(Y[pos == 0]) == POISON).all()


# ============================================================================================== slot_attn
def visible(p, window):
    if window == 0:
        return list(range(p + 1))
    lo2 = max(32, (p // 32 - (window - 1)) * 32)
    return list(range(min(p + 1, 32))) + list(range(lo2, p + 1))


ATTN_T = 140
ATTN_H = {16: 5, 64: 3, 96: 2}


def attn_run(fn, qkv, kc, vc, S, H, hd, posarg, window):
    kc, vc, O = kc.clone(), vc.clone(), poisoned(S, H * hd)
    fn(qkv, kc, vc, O, S, H, hd, ATTN_T, posarg, window)
    return O, kc, vc


@pytest.mark.parametrize('window', [0, 2], ids=['dense', 'window2'])
@pytest.mark.parametrize('hd', [16, 64, 96])
def test_slot_attn_equals_dec_attn(hd, window):
    S, H, T = 3, ATTN_H[hd], ATTN_T
    qkv = randn(S, 3 * H * hd, seed=hd)
    kc, vc = randn(S, H, T, hd, seed=hd + 1), randn(S, H, T, hd, seed=hd + 2)
    for c in (1, 2, 33, 97, T - 1):
        got = attn_run(K.slot_attn, qkv, kc, vc, S, H, hd, i32([c] * S), window)
        want = attn_run(K.dec_attn, qkv, kc, vc, S, H, hd, i32([c]), window)
        for g, w in zip(got, want):
            assert same(g, w), c


@pytest.mark.parametrize('window', [0, 2], ids=['dense', 'window2'])
@pytest.mark.parametrize('hd', [16, 64])
def test_slot_attn_mixed_positions_on_poisoned_caches(hd, window):
    """Each slot's cache row holds numbers only at the keys visible from its own position, NaN everywhere else:
    a read of any other key shows in O. The kernel writes position pos - 1 of the slot's row and nothing else;
    an idle slot's row and output stay as they were."""
    H, T = ATTN_H[hd], ATTN_T
    cs = [1, 2, 33, 97, T - 1, 0, 64, 0]
    S = len(cs)
    qkv = randn(S, 3 * H * hd, seed=hd + 7)
    kc, vc = poisoned(S, H, T, hd), poisoned(S, H, T, hd)
    fill_k, fill_v = randn(S, H, T, hd, seed=hd + 8), randn(S, H, T, hd, seed=hd + 9)
    for s, c in enumerate(cs):
        vis = [j for j in visible(c - 1, window) if j != c - 1] if c else []
        if vis:
            kc[s, :, vis], vc[s, :, vis] = fill_k[s, :, vis], fill_v[s, :, vis]
    O, kc2, vc2 = attn_run(K.slot_attn, qkv, kc, vc, S, H, hd, i32(cs), window)
    d = H * hd
    for s, c in enumerate(cs):
        if c == 0:
            assert same(kc2[s], kc[s]) and same(vc2[s], vc[s]) and (bits(O[s]) == POISON).all()
            continue
        want, _, _ = attn_run(K.dec_attn, qkv, kc, vc, S, H, hd, i32([c]), window)
        assert torch.isfinite(O[s]).all() and same(O[s], want[s]), (s, c)
        others = [j for j in range(T) if j != c - 1]
        assert same(kc2[s, :, others], kc[s, :, others]) and same(vc2[s, :, others], vc[s, :, others])
        assert same(kc2[s, :, c - 1].reshape(-1), qkv[s, d:2 * d]) and same(vc2[s, :, c - 1].reshape(-1), qkv[s, 2 * d:])


# ============================================================================================== embed / splice / penalty
EP_T, EP_V = 700, 1000


def ids_table(S, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, EP_V, (S, EP_T), generator=g).cuda()


def test_slot_embed_equals_dec_embed():
    S, D = 9, 136
    ids, table = ids_table(S, 3), randn(EP_V, D, seed=4)
    ref = {}
    for c in (1, 5, 600):
        ref[c] = poisoned(S, D)
        K.dec_embed(ids, EP_T, i32([c]), table, ref[c], S, D)
        x = poisoned(S, D)
        K.slot_embed(ids, EP_T, i32([c] * S), table, x, S, D)
        assert same(x, ref[c]), c
    pos = i32([1, 5, 600, 0, 5, 1, 0, 600, 600])
    x = poisoned(S, D)
    K.slot_embed(ids, EP_T, pos, table, x, S, D)
    for s, c in enumerate(pos.tolist()):
        assert (bits(x[s]) == POISON).all() if c == 0 else same(x[s], ref[c][s])


def test_slot_splice_takes_zp_at_position_one_only():
    S, D = 9, 136
    x0, zp = randn(S, D, seed=5), randn(S, D, seed=6)
    pos = i32([1, 2, 0, 1, 37, 1, 0, 3, 1])
    x = x0.clone()
    K.slot_splice(x, zp, pos, S, D)
    first = (pos == 1)
    assert same(x[first], zp[first]) and same(x[~first], x0[~first])
    # zp as a column block of a wider buffer (all layers' projections side by side)
    wide = randn(S, 3 * D, seed=7)
    x = x0.clone()
    K.slot_splice(x, wide[:, D:], pos, S, D, ldz=3 * D)
    assert same(x[first], wide[first, D:2 * D]) and same(x[~first], x0[~first])


def test_slot_penalty_equals_dec_penalty():
    """T 700 with c = 600: the window [c - 512, c) has moved off the start of the row."""
    S = 6
    ids, logits = ids_table(S, 8), randn(S, EP_V, seed=9)
    ref = {}
    for c in (1, 5, 600):
        ref[c] = logits.clone()
        K.dec_penalty(ref[c], S, None, ids, EP_T, i32([c]), None, 1.2)
        got = logits.clone()
        K.slot_penalty(got, S, ids, EP_T, i32([c] * S), 1.2)
        assert same(got, ref[c]), c
        assert not same(got, logits)
    pos = i32([600, 0, 5, 1, 0, 600])
    got = logits.clone()
    K.slot_penalty(got, S, ids, EP_T, pos, 1.2)
    for s, c in enumerate(pos.tolist()):
        assert same(got[s], logits[s] if c == 0 else ref[c][s])


# ============================================================================================== slot_sample
MODES = {'greedy': dict(temperature=0.0, top_k=0, top_p=0.9),
         'temperature': dict(temperature=0.8, top_k=0, top_p=1.0),
         'topk40': dict(temperature=1.0, top_k=40, top_p=1.0),
         'nucleus': dict(temperature=1.0, top_k=0, top_p=0.9),
         'topk40+nucleus': dict(temperature=1.0, top_k=40, top_p=0.9)}
SEED = 20231


def slot_sample(logits, pos, key, T, N, end=-1, ids=None, out=None, **mode):
    S, V = logits.shape
    ids = torch.full((S, T), -7, dtype=torch.int64, device='cuda') if ids is None else ids
    out = torch.full((N, T - 1), -7, dtype=torch.int16, device='cuda') if out is None else out
    pos = pos.clone()
    K.slot_sample(logits, V, S, ids, T, pos, key, out, N, end, mode['temperature'], mode['top_k'], mode['top_p'], SEED)
    return ids, out, pos


def dec_sample(logits, c, T, end=-1, **mode):
    S, V = logits.shape
    ids = torch.full((S, T), -7, dtype=torch.int64, device='cuda')
    K.dec_sample(logits, V, S, None, ids, T, i32([c]), None, end, mode['temperature'], mode['top_k'], mode['top_p'], SEED)
    return ids


@pytest.mark.parametrize('V', [1000, 32768])
@pytest.mark.parametrize('mode', list(MODES))
def test_slot_sample_equals_dec_sample(mode, V):
    S, T = 8, 9
    logits = randn(S, V, seed=V) * 3
    key = torch.arange(S, dtype=torch.int32, device='cuda')
    want = {c: dec_sample(logits, c, T, **MODES[mode]) for c in (1, 3, 6)}
    for c in (1, 3):
        ids, out, pos = slot_sample(logits, i32([c] * S), key, T, S, **MODES[mode])
        assert torch.equal(ids, want[c]), c
        assert torch.equal(out[:, c - 1].long(), want[c][:, c]) and pos.tolist() == [c + 1] * S
    # mixed positions and idle slots
    mixed = i32([1, 3, 6, 0, 3, 1, 0, 6])
    ids, out, pos = slot_sample(logits, mixed, key, T, S, **MODES[mode])
    for s, c in enumerate(mixed.tolist()):
        if c == 0:
            assert (ids[s] == -7).all() and (out[s] == -7).all() and pos[s] == 0
        else:
            assert torch.equal(ids[s], want[c][s]) and out[s, c - 1] == want[c][s, c]
            assert (out[s, [j for j in range(T - 1) if j != c - 1]] == -7).all()
    if mode != 'greedy':
        assert len({int(want[1][s, 1]) for s in range(S)}) > 1


def test_slot_sample_draws_follow_the_key_not_the_slot():
    """64 samples in nucleus mode at V 1000: the same (logits row, pos, key) triples in another slot order give
    the same token per sample; and the key matters (the same row under another key draws differently somewhere)."""
    S, V, T = 64, 1000, 8
    g = torch.Generator().manual_seed(5)
    logits = randn(S, V, seed=6)
    pos = torch.randint(1, 6, (S,), generator=g).to(torch.int32).cuda()
    key = torch.randperm(S, generator=g).to(torch.int32).cuda()
    perm = torch.randperm(S, generator=g).cuda()
    ids_a, out_a, _ = slot_sample(logits, pos, key, T, S, **MODES['nucleus'])
    ids_b, out_b, _ = slot_sample(logits[perm].contiguous(), pos[perm].contiguous(), key[perm].contiguous(), T, S,
                                  **MODES['nucleus'])
    assert torch.equal(ids_b, ids_a[perm]) and torch.equal(out_a, out_b)
    _, out_c, _ = slot_sample(logits, pos, ((key + 1) % S).contiguous(), T, S, **MODES['nucleus'])
    tok_a = out_a[key.long(), (pos - 1).long()]
    tok_c = out_c[((key + 1) % S).long(), (pos - 1).long()]
    assert (tok_a != tok_c).any()


def test_slot_sample_bookkeeping():
    """Planted logits, greedy: slot 1 emits the end token and finishes; slot 3 writes position T - 2 and finishes;
    the others advance by one; idle slot 4 is skipped. out[key][pos - 1] holds the token as int16 and nothing
    else in out changes."""
    S, T, V, end, N = 6, 6, 1000, 17, 40
    toks = (3, end, 5, 8, 9, 700)
    logits = torch.full((S, V), -5.0)
    for r, tok in enumerate(toks):
        logits[r, tok] = 4.0
    pos = i32([2, 2, 1, T - 2, 0, T - 3])
    key = i32([30, 7, 0, 39, 12, 21])
    ids, out, new = slot_sample(logits.cuda(), pos, key, T, N, end=end, **MODES['greedy'])
    assert new.tolist() == [3, -1, 2, -1, 0, T - 2]
    want_out = torch.full((N, T - 1), -7, dtype=torch.int16)
    want_ids = torch.full((S, T), -7, dtype=torch.int64)
    for s, (c, k, tok) in enumerate(zip(pos.tolist(), key.tolist(), toks)):
        if c:
            want_out[k, c - 1] = tok
            want_ids[s, c] = tok
    assert out.dtype == torch.int16 and torch.equal(out.cpu(), want_out) and torch.equal(ids.cpu(), want_ids)
    assert (out[:, T - 2] == -7).all()          # the last column of a full-length row is never written


# ============================================================================================== slot_refill
def refill_state(S, T, Z, pos, key, counter, done, N):
    st = dict(pos=i32(pos), key=i32(key), ids=torch.full((S, T), -7, dtype=torch.int64, device='cuda'),
              z_slot=poisoned(S, Z), next=i32([counter]), completed=i32([done]))
    z_all = randn(max(N, 1), Z, seed=N)
    K.slot_refill(st['pos'], st['key'], st['ids'], T, S, 1, z_all, st['z_slot'], N, st['next'], st['completed'])
    return st, z_all


def test_slot_refill_hands_out_sample_numbers_in_slot_order():
    S, T, Z = 8, 6, 20
    pos, key = [3, -1, 2, 4, -1, 1, -1, 5], [2, 3, 4, 5, 6, 7, 8, 9]
    st, z_all = refill_state(S, T, Z, pos, key, 10, 5, 12)
    assert st['pos'].tolist() == [3, 1, 2, 4, 1, 1, 0, 5]
    assert st['key'].tolist() == [2, 10, 4, 5, 11, 7, 8, 9]
    assert st['next'].item() == 12 and st['completed'].item() == 8
    assert st['ids'][[1, 4], 0].tolist() == [1, 1] and (st['ids'][:, 1:] == -7).all()
    assert (st['ids'][[0, 2, 3, 5, 6, 7], 0] == -7).all()
    assert same(st['z_slot'][1], z_all[10]) and same(st['z_slot'][4], z_all[11])
    assert (bits(st['z_slot'][[0, 2, 3, 5, 6, 7]]) == POISON).all()


def test_slot_refill_with_nothing_left_idles_every_finished_slot():
    S, T, Z = 8, 6, 20
    st, _ = refill_state(S, T, Z, [3, -1, 2, 4, -1, 0, -1, 5], list(range(8)), 12, 0, 12)
    assert st['pos'].tolist() == [3, 0, 2, 4, 0, 0, 0, 5] and st['key'].tolist() == list(range(8))
    assert st['next'].item() == 12 and st['completed'].item() == 3
    assert (st['ids'] == -7).all() and (bits(st['z_slot']) == POISON).all()


def test_slot_refill_initial_fill():
    """All slots finished without a sample (key -1): nothing is counted as completed."""
    S, T, Z = 8, 6, 20
    st, z_all = refill_state(S, T, Z, [-1] * S, [-1] * S, 0, 0, 3)
    assert st['pos'].tolist() == [1, 1, 1, 0, 0, 0, 0, 0] and st['key'].tolist() == [0, 1, 2] + [-1] * 5
    assert st['next'].item() == 3 and st['completed'].item() == 0
    assert same(st['z_slot'][:3], z_all) and (bits(st['z_slot'][3:]) == POISON).all()


def test_slot_refill_more_slots_than_one_pass():
    """600 slots (three passes of the 256-slot scan), every third finished: the numbering runs on across passes."""
    S, T, Z = 600, 4, 8
    pos = [-1 if s % 3 == 0 else 2 for s in range(S)]
    st, z_all = refill_state(S, T, Z, pos, list(range(S)), 100, 0, 250)
    fin = [s for s in range(S) if s % 3 == 0]
    got_key, got_pos = st['key'].tolist(), st['pos'].tolist()
    for r, s in enumerate(fin):
        if 100 + r < 250:
            assert got_key[s] == 100 + r and got_pos[s] == 1 and same(st['z_slot'][s], z_all[100 + r])
        else:
            assert got_pos[s] == 0
    assert st['next'].item() == 250 and st['completed'].item() == len(fin)
