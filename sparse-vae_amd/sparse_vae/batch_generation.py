"""Mass sampling helpers (sparse_vae/batch_generation.py in the reference).

`batch_generate_samples` is the reference's batch-synchronous loop: call `sample_func()` until `num_samples` rows
are gathered in one host buffer, then cut every row after its first end token. Two deviations, both because the
reference's version cannot run as written: its buffer is `max_length` wide while `sample` returns
`max_length - 1` columns (the copy fails on the shape), and its last batch overruns the buffer whenever
`num_samples` is not a multiple of the batch size. Here the width is taken from what `sample_func` returns and
the last batch is truncated. The buffer is pinned only where CUDA is available, so the helper also runs on CPU
tensors. `max_length` stays in the signature for compatibility; it only bounds the width.

`trim_samples` does the same cut on the result of `TransformerVAE.sample_stream`, which needs no loop.
"""
from typing import Callable, List, Optional

import torch


def trim_samples(ids: torch.Tensor, end_token: Optional[int]) -> List[torch.Tensor]:
    """ids [N, W] -> a list of N 1-D int16 host tensors, each cut after its first `end_token` (a row without one
    keeps its full width)."""
    ids = ids.to(device='cpu', dtype=torch.int16)
    n, width = ids.shape
    lengths = torch.full((n,), width, dtype=torch.long)
    if end_token is not None and width > 0:
        hit = ids.eq(end_token)
        first = hit.to(torch.uint8).argmax(dim=1)                 # first end token of the rows that have one
        lengths = torch.where(hit.any(dim=1), first + 1, lengths)
    return [row[:k] for row, k in zip(ids, lengths.tolist())]


@torch.no_grad()
def batch_generate_samples(sample_func: Callable[[], torch.Tensor], num_samples: int, max_length: int,
                           end_token: Optional[int]) -> List[torch.Tensor]:
    """Gather `num_samples` rows from repeated `sample_func()` calls (each a [batch, width] id tensor) and trim them."""
    buffer, filled = None, 0
    while filled < num_samples:
        batch = sample_func()
        if batch is None or batch.shape[0] == 0:
            raise RuntimeError('batch_generate_samples: sample_func returned no samples')
        batch = batch.to(torch.int16)
        if buffer is None:
            width = min(batch.shape[1], max_length)
            buffer = torch.zeros(num_samples, width, dtype=torch.int16, pin_memory=torch.cuda.is_available())
        take = min(batch.shape[0], num_samples - filled)
        buffer[filled:filled + take].copy_(batch[:take, :buffer.shape[1]], non_blocking=True)
        filled += take
    if buffer is None:
        return []
    if torch.cuda.is_available():
        torch.cuda.synchronize()
    return trim_samples(buffer, end_token)
