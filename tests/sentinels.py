"""Sentinel-filled output buffers for the one-kernel-at-a-time GPU tests (test_head_kernels_gpu.py,
test_attn_kernels_gpu.py, test_ln_kernels_gpu.py, test_gemm_kernels_gpu.py): a kernel's output is a view into a larger buffer whose remainder holds SENTINEL, and
intact() checks after the launch that nothing outside the view was written. report() / ratio() print each measured
figure beside its bound before asserting it."""
import torch

dev = 'cuda'
GUARD = 64                        # sentinel elements after a flat output
XROWS = 3                         # sentinel rows below a matrix output
SENTINEL = -7777.0
f32 = torch.float32


def g(t):
    return t.to(dev)


def flat(n, dtype=f32, fill=SENTINEL):
    """-> (buffer, view of its first n elements); the GUARD elements after them hold the sentinel."""
    full = torch.full((n + GUARD,), SENTINEL, dtype=dtype, device=dev)
    full[:n] = fill
    return full, full[:n]


def matrix(rows, cols, ld, dtype, fill=SENTINEL):
    """-> (buffer [rows + XROWS, ld], view [rows, cols]); everything outside the view holds the sentinel."""
    full = torch.full((rows + XROWS, ld), SENTINEL, dtype=dtype, device=dev)
    full[:rows, :cols] = fill
    return full, full[:rows, :cols]


def intact(full, rows=None, cols=None):
    """The sentinels of flat() / matrix() survived."""
    s = torch.tensor(SENTINEL, dtype=full.dtype)
    if full.dim() == 1:
        return bool((full[-GUARD:] == s).all().item())
    return bool((full[rows:] == s).all().item() and (full[:, cols:] == s).all().item())


def report(what, got, limit):
    print(f'{what}: {got:.3e} (bound {limit:.3e})')
    assert got <= limit, (what, got, limit)


def ratio(what, got):
    print(f'{what}: {got:.3f} of its allowance')
    assert got <= 1.0, (what, got)
