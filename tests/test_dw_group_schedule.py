"""kernels.group_schedule (CPU): the fixed schedule of the grouped weight-gradient pass at the C2 / C4 / tiny shapes."""
from sparse_vae import kernels as K


def _model(d, T, R, layers, enc_mid):
    """The deferred dW GEMMs of a backward in launch order, (n_out, n_in, rows): decoder layers over T token rows; the
    encoder's layers over R = batch x latents rows, their key / value projections over the T token rows."""
    dec = [(d, 4 * d, T), (4 * d, d, T), (d, d, T), (3 * d, d, T)] * layers
    mid = [(d, 4 * d, R), (4 * d, d, R), (d, d, R), (d, d, R), (2 * d, d, T), (d, d, R), (3 * d, d, R)] * enc_mid
    first = [(d, 4 * d, R), (4 * d, d, R), (d, d, R), (2 * d, d, T)]
    return dec + mid + first


def _tiles(s):
    return -(-s[0] // 256) * -(-s[1] // 256)


def _check(shapes, ncu=256):
    calls = K.group_schedule(shapes, ncu)
    seen = sorted(i for idx, _, _ in calls for i in idx)
    assert seen == list(range(len(shapes)))                      # every GEMM exactly once
    for idx, splits, slab in calls:
        assert sum(_tiles(shapes[i]) for i, sb in zip(idx, slab) if not sb) <= ncu   # one round of whole-K tiles
        for i, s, sb in zip(idx, splits, slab):
            assert s >= 1 and (sb or s == 1)
            kchunk = -(-(-(-shapes[i][2] // s)) // 64) * 64
            assert (s - 1) * kchunk < shapes[i][2]               # no empty slice
    return calls


def test_c2_one_full_round_and_one_round_of_slices():
    shapes = _model(512, 32768, 4096, 6, 1)
    calls = _check(shapes)
    assert len(calls) == 1
    idx, splits, slab = calls[0]
    whole = [i for i, sb in zip(idx, slab) if not sb]
    assert sum(_tiles(shapes[i]) for i in whole) == 256 and all(shapes[i][2] == 32768 for i in whole)
    units = sum(_tiles(shapes[i]) * s for i, s, sb in zip(idx, splits, slab) if sb)
    assert 192 <= units <= 256                                   # the slices fill the chip once


def test_c4_full_rounds_only():
    shapes = _model(768, 65536, 4096, 12, 4)
    calls = _check(shapes)
    assert len(calls) == 5                                       # 1296 decoder tiles: five rounds of 252
    for idx, _, slab in calls:
        assert sum(_tiles(shapes[i]) for i, sb in zip(idx, slab) if not sb) == 252


def test_tiny_and_odd_chips():
    assert len(_check(_model(128, 512, 256, 4, 0))) == 1         # nothing fills a round: slices only
    _check(_model(512, 32768, 4096, 6, 1), ncu=304)
    _check(_model(768, 65536, 2048, 12, 4), ncu=64)
