"""Reconstruction scoring on one MI355X: svae_ngram_overlap and svae_edit_distance against what a user would write in
torch on the same device, in the same process on the same tensors.

    python scripts/bench_textscore.py [--pairs 4096] [--widths 128 512 2048] [--reps 20] [--json PATH]

The references are seeded rows of W / 2 .. W tokens from the full vocabulary; a candidate is its reference with 10 %
of its tokens edited (substitutions, deletions and insertions in equal parts), cut to W. Both baselines are batched
over all pairs (a per-pair loop, which is what the reference's reconstruction_bleu is, pays some forty launches per
pair and is not timed):
  n-grams  per order n the keys of n packed 15-bit ids, one torch.sort per side over [P, W], then three batched
           torch.searchsorted: a candidate key counts when its rank inside its run of equal keys is below the run's
           length on the reference side, which sums to the clipped matches. 4 orders x (2 sorts + 3 searches).
  edit     the anti-diagonal wavefront over [P, W + 1] int32 tensors, 2 W diagonals of nine elementwise launches.
Each figure is the median of --reps runs between two HIP events after 3 warm-ups (the torch edit distance at W = 2048
takes a second per run and gets 3 reps), with the smallest and largest run beside it; the kernel and its baseline are
timed alternately. The counts of the two routes are compared on every pair and must be equal. No speed is asserted."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'sparse-vae_amd'))
import numpy as np  # noqa: E402
import torch  # noqa: E402

VOCAB = 32768
RATE = 0.10


def make_pairs(P, W, seed=1):
    """(cand, ref int16 [P, W], cand_len, ref_len int32 [P]) on the host."""
    rng = np.random.default_rng(seed)
    cand, ref = np.zeros((P, W), dtype=np.int16), np.zeros((P, W), dtype=np.int16)
    Lc, Lr = np.zeros(P, dtype=np.int32), rng.integers(W // 2, W + 1, P).astype(np.int32)
    third = RATE / 3
    for p in range(P):
        r = rng.integers(0, VOCAB, Lr[p])
        u = rng.random(Lr[p])
        kept = np.where(u < third, rng.integers(0, VOCAB, Lr[p]), r)          # substitutions
        emit = (u >= 2 * third) | (u < third)                                  # deletions drop the rest
        ins = rng.random(Lr[p]) < third
        out = np.stack([np.where(emit, kept, -1), np.where(ins, rng.integers(0, VOCAB, Lr[p]), -1)], axis=1).ravel()
        out = out[out >= 0][:W]
        ref[p, :Lr[p]], cand[p, :len(out)], Lc[p] = r, out, len(out)
    return cand, ref, Lc, Lr


def torch_ngram(cand, ref, Lc, Lr):
    """[P, 4] clipped matches, batched: see the module docstring."""
    P, big = cand.shape[0], torch.iinfo(torch.int64).max
    out = torch.empty(P, 4, dtype=torch.int64, device=cand.device)
    c64, r64 = cand.long(), ref.long()
    for n in range(1, 5):
        def keys(t, L, filler):
            W = t.shape[1]
            k = t[:, :W - n + 1].clone()
            for m in range(1, n):
                k = (k << 15) | t[:, m:W - n + 1 + m]
            valid = torch.arange(W - n + 1, device=t.device)[None, :] + n <= L[:, None]
            return torch.where(valid, k, torch.full_like(k, filler)).sort(dim=1).values
        if cand.shape[1] < n or ref.shape[1] < n:
            out[:, n - 1] = 0
            continue
        A, B = keys(c64, Lc, big), keys(r64, Lr, big - 1)
        rank = torch.arange(A.shape[1], device=A.device)[None, :] - torch.searchsorted(A, A)
        count = torch.searchsorted(B, A, right=True) - torch.searchsorted(B, A)
        out[:, n - 1] = ((A < big - 1) & (rank < count)).sum(dim=1)
    return out


def torch_edit(cand, ref, Lc, Lr):
    """[P] Levenshtein distances: D[i][d - i] along the anti-diagonals d, indexed by the candidate position i."""
    P, Wc = cand.shape
    Wr, dev = ref.shape[1], cand.device
    i = torch.arange(Wc + 1, device=dev, dtype=torch.int32)[None, :].expand(P, Wc + 1)
    cpad = torch.cat([torch.full((P, 1), -1, device=dev, dtype=torch.int32), cand.int()], dim=1)      # c[i - 1] at i
    # r[d - i - 1] at i: a window of the reversed, padded reference
    rrev = torch.cat([torch.full((P, Wc + 1), -2, device=dev, dtype=torch.int32), ref.int().flip(1),
                      torch.full((P, Wc + 1), -2, device=dev, dtype=torch.int32)], dim=1)
    inf = Wc + Wr + 1
    prev2 = torch.where(i == 0, 0, inf).int()                                  # d = 0
    prev1 = torch.where(i <= 1, 1, inf).int()                                  # d = 1: D[0][1], D[1][0]
    target, rows = (Lc + Lr).long(), torch.arange(P, device=dev)
    at = Lc.long().clamp(max=Wc)
    res = torch.where(target == 0, 0, torch.where(target == 1, 1, 0)).int()
    for d in range(2, Wc + Wr + 1):
        start = Wc + 1 + Wr - d                                                # rrev[start + i] = r[d - i - 1]
        sub = prev2[:, :-1] + (cpad[:, 1:] != rrev[:, start + 1:start + Wc + 1]).int()
        inner = torch.minimum(torch.minimum(prev1[:, :-1], prev1[:, 1:]) + 1, sub)
        cur = torch.cat([torch.full((P, 1), d, device=dev, dtype=torch.int32), inner], dim=1)
        cur = torch.where((i == d), d, torch.where((i > d) | (d - i > Wr), inf, cur))
        res = torch.where(target == d, cur[rows, at], res)
        prev2, prev1 = prev1, cur
    return res


def timed_pair(f, g, reps_f, reps_g, warmup=3):
    """Median (and min, max) milliseconds of f and g, run alternately."""
    def once(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)
    for _ in range(warmup):
        f()
    g()
    torch.cuda.synchronize()
    tf, tg = [], []
    for k in range(max(reps_f, reps_g)):
        if k < reps_f:
            tf.append(once(f))
        if k < reps_g:
            tg.append(once(g))
    stat = lambda t: (statistics.median(t), min(t), max(t))      # noqa: E731
    return stat(tf), stat(tg)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=4096)
    ap.add_argument('--widths', type=int, nargs='+', default=[128, 512, 2048])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--json', default=None)
    a = ap.parse_args(argv)
    assert torch.cuda.is_available(), 'bench_textscore needs a GPU (no CPU fallback)'
    from sparse_vae import kernels as K
    dev = torch.device('cuda', 0)
    results = []
    print(f'{"pairs":>6s} {"width":>6s} {"ngram ms":>22s} {"torch ms":>26s} {"speed-up":>9s} {"edit ms":>22s} '
          f'{"torch ms":>28s} {"speed-up":>9s} {"Gcell/s":>8s} {"equal":>6s}', flush=True)
    for W in a.widths:
        cand, ref, Lc, Lr = (torch.from_numpy(t).to(dev) for t in make_pairs(a.pairs, W))
        out5 = torch.empty(a.pairs, 5, dtype=torch.int32, device=dev)
        out1 = torch.empty(a.pairs, dtype=torch.int32, device=dev)
        slow = 3 if W >= 1024 else a.reps
        tn, tn_t = timed_pair(lambda: K.ngram_overlap(cand, ref, Lc, Lr, out=out5),
                              lambda: torch_ngram(cand, ref, Lc, Lr), a.reps, a.reps)
        te, te_t = timed_pair(lambda: K.edit_distance(cand, ref, Lc, Lr, out=out1),
                              lambda: torch_edit(cand, ref, Lc, Lr), a.reps, slow)
        equal = bool(torch.equal(out5[:, :4].long(), torch_ngram(cand, ref, Lc, Lr)) and
                     torch.equal(out1, torch_edit(cand, ref, Lc, Lr)))
        cells = float((Lc.double() * Lr.double()).sum())
        r = {'pairs': a.pairs, 'width': W, 'mean_cand_len': round(float(Lc.float().mean()), 1),
             'mean_ref_len': round(float(Lr.float().mean()), 1),
             'ngram_ms': round(tn[0], 4), 'ngram_ms_min_max': [round(tn[1], 4), round(tn[2], 4)],
             'torch_ngram_ms': round(tn_t[0], 4), 'torch_ngram_ms_min_max': [round(tn_t[1], 4), round(tn_t[2], 4)],
             'ngram_speedup_vs_torch': round(tn_t[0] / tn[0], 2),
             'edit_ms': round(te[0], 4), 'edit_ms_min_max': [round(te[1], 4), round(te[2], 4)],
             'torch_edit_ms': round(te_t[0], 4), 'torch_edit_ms_min_max': [round(te_t[1], 4), round(te_t[2], 4)],
             'torch_edit_reps': slow, 'edit_speedup_vs_torch': round(te_t[0] / te[0], 2),
             'edit_gcells_per_s': round(cells / (te[0] * 1e-3) / 1e9, 2), 'counts_equal': equal}
        results.append(r)
        fmt = lambda t: f'{t[0]:9.4f} [{t[1]:.3f}, {t[2]:.3f}]'      # noqa: E731
        print(f'{a.pairs:6d} {W:6d} {fmt(tn):>22s} {fmt(tn_t):>26s} {tn_t[0] / tn[0]:8.2f}x {fmt(te):>22s} '
              f'{fmt(te_t):>28s} {te_t[0] / te[0]:8.2f}x {r["edit_gcells_per_s"]:8.2f} {str(equal):>6s}', flush=True)
        del cand, ref
        torch.cuda.empty_cache()
    print(json.dumps({'bench': 'textscore', 'results': results}), flush=True)
    if a.json:
        with open(a.json, 'w') as f:
            json.dump(results, f, indent=1)
    assert all(r['counts_equal'] for r in results), 'the kernels and the torch baselines disagree on a count'


if __name__ == '__main__':
    main()
