"""CPU side of streaming bulk sampling: the batch_generate_samples port and trim_samples on host tensors, the
argument validation of every svae_slot_* entry point (before any launch), and sample.py's parser."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
END = 3


def rows():
    """10 rows of width 7: ends at various places, one row without an end token, one with two."""
    g = torch.Generator().manual_seed(0)
    ids = torch.randint(4, 30000, (10, 7), generator=g)
    for r, e in enumerate((0, 6, 2, None, 4, 1, 5, 3, None, 2)):
        if e is not None:
            ids[r, e] = END
    ids[4, 6] = END                 # a second end token after the first
    ids[2, 5] = END
    return ids


def expected(ids):
    out = []
    for r in ids.tolist():
        out.append(torch.tensor(r[:r.index(END) + 1] if END in r else r, dtype=torch.int16))
    return out


def test_batch_generate_samples_truncates_the_last_batch_and_trims():
    from sparse_vae import batch_generate_samples
    ids = rows()
    calls = []

    def sample_func():                                   # batches of 4: 4 + 4 + 2 of the third batch's 4
        i = len(calls) * 4
        calls.append(i)
        return torch.cat([ids, ids])[i:i + 4].clone()

    got = batch_generate_samples(sample_func, 10, 8, END)     # max_length 8: sample() returns max_length - 1 columns
    want = expected(ids)
    assert len(calls) == 3 and len(got) == 10
    for g, w in zip(got, want):
        assert g.dtype == torch.int16 and g.dim() == 1 and torch.equal(g, w)
    assert len(got[3]) == 7 and len(got[8]) == 7             # no end token: the full width
    assert got[4].tolist().count(END) == 1 and len(got[4]) == 5   # two end tokens: cut at the first
    assert len(got[0]) == 1 and len(got[1]) == 7             # end token in the first / the last column


def test_batch_generate_samples_zero_samples_calls_nothing():
    from sparse_vae import batch_generate_samples
    assert batch_generate_samples(lambda: 1 / 0, 0, 8, END) == []


def test_trim_samples_matches_batch_generate_samples():
    from sparse_vae import batch_generate_samples, trim_samples
    ids = rows()
    a = trim_samples(ids.to(torch.int16), END)
    b = batch_generate_samples(lambda: ids, 10, 8, END)
    assert len(a) == len(b) == 10
    for x, y, w in zip(a, b, expected(ids)):
        assert x.dtype == torch.int16 and torch.equal(x, y) and torch.equal(x, w)
    assert [len(r) for r in trim_samples(ids, None)] == [7] * 10
    assert trim_samples(torch.zeros(0, 7, dtype=torch.int16), END) == []


def test_slot_entry_points_reject_bad_arguments_without_launch():
    """Validation happens before any launch, so it is testable without a GPU. 16 and 64 stand for aligned non-null
    pointers that are never dereferenced; 24 is misaligned."""
    from sparse_vae._native import lib
    p, q, bad = 64, 128, 24
    ok_lin = dict(X=p, ldx=128, W=p, ldw=128, bias=None, Y=p, ldy=384, resid=None, ldr=384, S=8, N=384, K=128, rot=p,
                  rot_cols=256, rot_d=128, pos=p, part=None, part_elems=0)

    def linear(**kw):
        return lib.svae_slot_linear(*{**ok_lin, **kw}.values(), None)
    for kw in (dict(X=None), dict(W=None), dict(Y=None), dict(pos=None), dict(rot=None), dict(S=0), dict(S=-3),
               dict(K=126), dict(ldx=130), dict(X=bad), dict(W=bad), dict(rot_d=127), dict(rot_cols=255)):
        assert linear(**kw) == 1, kw

    ok_attn = dict(qkv=p, ldq=384, kc=p, vc=q, S=8, H=8, hd=16, T=64, pos=p, window=0, scale=0.25, O=p, ldo=128)

    def attn(**kw):
        return lib.svae_slot_attn(*{**ok_attn, **kw}.values(), None)
    for kw in (dict(qkv=None), dict(kc=None), dict(vc=None), dict(pos=None), dict(O=None), dict(S=0), dict(T=32769),
               dict(T=0), dict(hd=132), dict(hd=18), dict(kc=bad), dict(vc=bad), dict(ldq=386), dict(window=-1)):
        assert attn(**kw) == 1, kw

    ok_embed = dict(ids=p, T=64, pos=p, table=p, x=p, S=8, D=128)

    def embed(**kw):
        return lib.svae_slot_embed(*{**ok_embed, **kw}.values(), None)
    for kw in (dict(ids=None), dict(pos=None), dict(table=None), dict(x=None), dict(S=0), dict(D=126), dict(T=32769),
               dict(table=bad), dict(x=bad)):
        assert embed(**kw) == 1, kw

    ok_splice = dict(x=p, zp=q, ldz=128, pos=p, S=8, D=128)

    def splice(**kw):
        return lib.svae_slot_splice(*{**ok_splice, **kw}.values(), None)
    for kw in (dict(x=None), dict(zp=None), dict(pos=None), dict(S=0), dict(D=126), dict(x=bad), dict(zp=bad), dict(ldz=124),
               dict(ldz=130)):
        assert splice(**kw) == 1, kw

    ok_pen = dict(logits=p, ldl=1000, S=8, ids=p, T=64, pos=p, penalty=1.2)

    def penalty(**kw):
        return lib.svae_slot_penalty(*{**ok_pen, **kw}.values(), None)
    for kw in (dict(logits=None), dict(ids=None), dict(pos=None), dict(S=0), dict(T=32769), dict(T=0)):
        assert penalty(**kw) == 1, kw

    ok_sample = dict(logits=p, ldl=1000, V=1000, S=8, ids=p, T=64, pos=p, key=p, out=p, N=100, end=2, temp=1.0,
                     top_k=0, top_p=0.9, seed=1)

    def sample(**kw):
        return lib.svae_slot_sample(*{**ok_sample, **kw}.values(), None)
    for kw in (dict(logits=None), dict(ids=None), dict(pos=None), dict(key=None), dict(out=None), dict(S=0),
               dict(V=32769), dict(V=0), dict(T=32769), dict(T=1), dict(N=-1)):
        assert sample(**kw) == 1, kw

    ok_refill = dict(pos=p, key=p, ids=p, T=64, S=8, start=1, z_all=p, z_slot=p, Z=64, N=100, next=p, completed=p)

    def refill(**kw):
        return lib.svae_slot_refill(*{**ok_refill, **kw}.values(), None)
    for kw in (dict(pos=None), dict(key=None), dict(ids=None), dict(z_all=None), dict(z_slot=None), dict(next=None),
               dict(completed=None), dict(S=0), dict(S=-1), dict(Z=0), dict(T=32769), dict(T=1), dict(N=-1)):
        assert refill(**kw) == 1, kw


def test_sample_py_parser_defaults():
    sys.path.insert(0, ROOT)
    try:
        import sample as tool
    finally:
        sys.path.remove(ROOT)
    a = tool.build_parser().parse_args([])
    assert (a.num_samples, a.max_length, a.slots, a.out) == (700_000, 512, 1000, 'samples.npz')
    assert (a.top_k, a.top_p, a.temperature, a.repetition_penalty) == (0, 0.9, 1.0, 1.2)
    assert a.preset is None and a.weights is None and a.device is None and not a.loop and a.overrides == []
    b = tool.build_parser().parse_args(['--preset', 'tiny', '--loop', '--num-samples', '40', 'model.d_model=256'])
    assert b.preset == 'tiny' and b.loop and b.num_samples == 40 and b.overrides == ['model.d_model=256']
