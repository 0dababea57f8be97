"""Reconstruction scoring: how much of a document comes back out of its latent.

`score_reconstructions` runs the two scoring kernels (svae_ngram_overlap, svae_edit_distance: csrc/textscore.hip) over a
batch of (candidate, reference) id rows on the device and returns their integer counts as a `ReconstructionScores`,
whose methods turn the integers into BLEU (sentence and corpus form), token accuracy and the translation edit rate on
the host in float64. The quantity is the textbook BLEU of Papineni et al. (2002) over token ids with a brevity
penalty; the reference's `reconstruction_bleu` (math_utils.py:9-38) is not reproduced (DESIGN section 7 says why).
`corpus_bleu(2)` is the setting of the reference's `train_bleu` callback (weights 1/2, 1/2), over token ids where
the callback counts whitespace words.

`reference_rows` puts a data-module batch into the frame of the decoder's output, `interpolate_latents` gives the
latents between two documents; `TransformerVAE.autoencode` produces the candidates.
"""
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch

from . import kernels as K
from ._native import TEXT_MAX_LEN
from .core.padded_tensor import PaddedTensor

VOCAB = 2 ** 15


def _host(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


@dataclass
class ReconstructionScores:
    """Integer counts of P scored pairs (tensors or arrays, int32 / int64): matches [P, 4] (clipped n-gram matches of
    orders 1..4), totals [P, 4] (the candidate's n-grams, max(Lc - n + 1, 0)), exact [P] (equal positions), edit [P]
    (Levenshtein distance) or None, cand_len [P], ref_len [P]."""
    matches: torch.Tensor
    totals: torch.Tensor
    exact: torch.Tensor
    edit: Optional[torch.Tensor]
    cand_len: torch.Tensor
    ref_len: torch.Tensor

    def __len__(self):
        return int(self.cand_len.shape[0])

    @classmethod
    def cat(cls, parts):
        """The scores of several batches as one (on the host)."""
        parts = list(parts)
        join = lambda name: np.concatenate([_host(getattr(p, name)) for p in parts])  # noqa: E731
        edit = None if any(p.edit is None for p in parts) else join('edit')
        return cls(join('matches'), join('totals'), join('exact'), edit, join('cand_len'), join('ref_len'))

    def _f64(self, name):
        return _host(getattr(self, name)).astype(np.float64)

    def bleu(self, max_n: int = 4, smooth: bool = False):
        """Per-pair BLEU, float64 [P]: BP * exp(mean_n log p_n), p_n = m_n / total_n, BP = 1 if Lc > Lr else
        exp(1 - Lr / Lc); 0 when any p_n is 0 or Lc is 0. smooth: (m_n + 1) / (total_n + 1) for n >= 2."""
        if not 1 <= max_n <= 4:
            raise ValueError(f'bleu: max_n in 1..4, got {max_n}')
        m, tot = self._f64('matches')[:, :max_n].copy(), self._f64('totals')[:, :max_n].copy()
        lc, lr = self._f64('cand_len'), self._f64('ref_len')
        if smooth:
            m[:, 1:] += 1.0
            tot[:, 1:] += 1.0
        ok = (m > 0).all(axis=1) & (tot > 0).all(axis=1) & (lc > 0)
        out = np.zeros(len(lc), dtype=np.float64)
        if ok.any():
            logs = np.log(m[ok] / tot[ok]).sum(axis=1) / max_n
            bp = np.where(lc[ok] > lr[ok], 1.0, np.exp(1.0 - lr[ok] / lc[ok]))
            out[ok] = bp * np.exp(logs)
        return out

    def corpus_bleu(self, max_n: int = 4) -> float:
        """Papineni's corpus form: matches, totals and lengths summed over the pairs before the ratio."""
        if not 1 <= max_n <= 4:
            raise ValueError(f'corpus_bleu: max_n in 1..4, got {max_n}')
        m = _host(self.matches).astype(np.int64).sum(axis=0)[:max_n].astype(np.float64)
        tot = _host(self.totals).astype(np.int64).sum(axis=0)[:max_n].astype(np.float64)
        lc, lr = float(_host(self.cand_len).astype(np.int64).sum()), float(_host(self.ref_len).astype(np.int64).sum())
        if lc <= 0 or (m <= 0).any() or (tot <= 0).any():
            return 0.0
        bp = 1.0 if lc > lr else float(np.exp(1.0 - lr / lc))
        return bp * float(np.exp(np.log(m / tot).sum() / max_n))

    def token_accuracy(self) -> float:
        """sum exact / sum Lr: the share of reference positions the candidate reproduces in place."""
        return float(_host(self.exact).astype(np.int64).sum()) / float(_host(self.ref_len).astype(np.int64).sum())

    def ter(self) -> float:
        """sum edit / sum Lr: edits per reference token."""
        if self.edit is None:
            raise ValueError('ter: the scores were computed with edit=False')
        return float(_host(self.edit).astype(np.int64).sum()) / float(_host(self.ref_len).astype(np.int64).sum())

    def summary(self) -> dict:
        out = dict(pairs=len(self), corpus_bleu=self.corpus_bleu(4), bleu2=self.corpus_bleu(2),
                   sentence_bleu=float(self.bleu(4, smooth=True).mean()) if len(self) else 0.0,
                   token_accuracy=self.token_accuracy(), mean_cand_len=float(self._f64('cand_len').mean()),
                   mean_ref_len=float(self._f64('ref_len').mean()))
        if self.edit is not None:
            out['ter'] = self.ter()
        return out


def _ids16(t, name):
    """A device id matrix as contiguous int16 [P, W], refusing ids outside 0..32767."""
    if isinstance(t, PaddedTensor):
        t = t.as_raw()
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.dtype not in (torch.int16, torch.int32, torch.int64):
        raise ValueError(f'score_reconstructions: {name} must be an int16 / int32 / int64 tensor [P, W]')
    if not t.is_cuda:
        raise RuntimeError('libsvae kernels need device tensors (no CPU fallback)')
    if not 1 <= t.shape[1] <= TEXT_MAX_LEN:
        raise ValueError(f'score_reconstructions: {name} are {t.shape[1]} wide; rows of 1..{TEXT_MAX_LEN} tokens '
                         f'(SVAE_TEXT_MAX_LEN) are scored')
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= VOCAB):
        raise ValueError(f'score_reconstructions: {name} hold ids outside 0..{VOCAB - 1}')
    return t.to(torch.int16).contiguous()


def _first_end(ids, end_token):
    """(has an end token [P] bool, tokens up to and including the first one [P] int64), on the device."""
    hit = ids.eq(end_token)
    return hit.any(dim=1), hit.to(torch.uint8).argmax(dim=1) + 1


def default_lengths(ids, end_token=2, zero_pad=False):
    """trim_samples' rule on the device: tokens up to and including the first end token, the full width where there
    is none (zero_pad: the number of leading non-zero ids there). int32 [P]."""
    P, W = ids.shape
    has, upto = _first_end(ids, end_token)
    if zero_pad:
        zero = ids.eq(0)
        other = torch.where(zero.any(dim=1), zero.to(torch.uint8).argmax(dim=1), torch.full_like(upto, W))
    else:
        other = torch.full_like(upto, W)
    return torch.where(has, upto, other).to(torch.int32)


def _lengths(t, P, name):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    if t.dim() != 1 or t.shape[0] != P or t.dtype not in (torch.int16, torch.int32, torch.int64):
        raise ValueError(f'score_reconstructions: {name} must be an integer tensor [{P}]')
    return t


@torch.no_grad()
def score_reconstructions(candidates, references, cand_lengths=None, ref_lengths=None, end_token=2, edit=True):
    """Score P reconstructions against their originals: device id matrices [P, W] (int16 / int32 / int64, ids
    0..32767, at most SVAE_TEXT_MAX_LEN wide) -> ReconstructionScores (device tensors). Lengths default to the tokens
    up to and including the first end_token; a candidate without one counts its full width, a reference without one its
    leading non-zero ids. Given lengths are clamped into [0, width]."""
    cand, ref = _ids16(candidates, 'candidates'), _ids16(references, 'references')
    P = cand.shape[0]
    if ref.shape[0] != P or P < 1:
        raise ValueError(f'score_reconstructions: {P} candidates against {ref.shape[0]} references')
    dev = cand.device
    if cand_lengths is None:
        lc = default_lengths(cand, end_token)
    else:
        lc = _lengths(cand_lengths, P, 'cand_lengths').to(dev).clamp(0, cand.shape[1]).to(torch.int32)
    if ref_lengths is None:
        lr = default_lengths(ref, end_token, zero_pad=True)
    else:
        lr = _lengths(ref_lengths, P, 'ref_lengths').to(dev).clamp(0, ref.shape[1]).to(torch.int32)
    lc, lr = lc.contiguous(), lr.contiguous()
    counts = K.ngram_overlap(cand, ref, lc, lr)
    dist = K.edit_distance(cand, ref, lc, lr) if edit else None
    n = torch.arange(4, device=dev, dtype=torch.int32)
    totals = (lc[:, None] - n[None, :]).clamp_min(0)
    return ReconstructionScores(counts[:, :4], totals, counts[:, 4], dist, lc, lr)


def reference_rows(batch):
    """A data-module batch in the frame of the decoder's output: (ids [B, W - 1], lengths int32 [B]). A collated row
    is [CLS] tokens [SEP] and zeros, with num_tokens counting both special tokens (RobertaProcessing in
    text_data_module.py:243, the collate at 194-210); final_output drops the start token, so the row loses its first
    column and its length, up to and including the end token, is num_tokens - 1."""
    ids = batch['token_ids']
    ids = ids.as_raw() if isinstance(ids, PaddedTensor) else ids
    lengths = (torch.as_tensor(batch['num_tokens']).to(ids.device) - 1).clamp(0, ids.shape[1] - 1).to(torch.int32)
    return ids[:, 1:], lengths


def interpolate_latents(a, b, steps, mode='linear'):
    """`steps` latents from a to b, endpoints included: [steps, 1, Z]. linear: (1 - t) a + t b; slerp: along the great
    circle between the directions of a and b with the norm interpolated linearly (linear where they are parallel or opposite)."""
    if steps < 2:
        raise ValueError(f'interpolate_latents: at least the two endpoints, got steps={steps}')
    if mode not in ('linear', 'slerp'):
        raise ValueError(f"interpolate_latents: mode 'linear' or 'slerp', got {mode!r}")
    a, b = a.reshape(-1), b.reshape(-1)
    if a.shape != b.shape:
        raise ValueError('interpolate_latents: the two latents differ in size')
    t = torch.linspace(0.0, 1.0, steps, device=a.device, dtype=torch.float64)[:, None]
    a64, b64 = a.double()[None, :], b.double()[None, :]
    out = (1.0 - t) * a64 + t * b64
    if mode == 'slerp':
        na, nb = a64.norm(), b64.norm()
        cos = ((a64 * b64).sum() / (na * nb).clamp_min(1e-300)).clamp(-1.0, 1.0)
        omega = torch.acos(cos)
        if 1e-6 < float(omega) < 3.141592 and float(na) > 0 and float(nb) > 0:
            so = torch.sin(omega)
            direction = (torch.sin((1.0 - t) * omega) / so) * (a64 / na) + (torch.sin(t * omega) / so) * (b64 / nb)
            out = ((1.0 - t) * na + t * nb) * direction
    out[0], out[-1] = a64[0], b64[0]
    return out.to(a.dtype)[:, None, :]
