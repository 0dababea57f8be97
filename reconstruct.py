"""python reconstruct.py --weights model.pt --out recon.npz [--preset NAME] [section.key=value ...]

Reconstruction at corpus scale (the reference's reconstruct.py answers one typed title at a time): every batch of the
data module's test (or train) loader is encoded, decoded again from its posterior mean (TransformerVAE.autoencode:
encode, then sample_stream(z=...)) and scored against the original on the device (sparse_vae.score_reconstructions:
clipped n-gram matches of orders 1..4, equal positions and the token edit distance per document). Printed: corpus
BLEU-4, BLEU-2 (the training callback's train_bleu setting, over token ids), the mean smoothed sentence BLEU-4, token
accuracy, the edit rate (TER), mean lengths, the number of documents and how many originals were longer than
--max-length - 1 tokens and were cut to that window. --json prints the same as one JSON line. The .npz holds
    ids      int16 [N, max_length - 1], the reconstructions, zero after each one's end,
    lengths  int32 [N], tokens up to and including the first end token (the full width where there is none),
    matches, totals int32 [N, 4], exact, edit, ref_len int32 [N]: the integer counts every figure above is made of,
    titles   where the batches carry them,
    hparams  the model's hyperparameters and the generation settings, as a JSON string.
--beams N [--length-penalty A] decodes by beam search instead (TransformerVAE.beam_search: the most probable
continuation under p(x|z), no seed, scores comparable between latents), in the corpus mode and under --interpolate. The
.npz then also holds beam_scores and beam_log_probs f32 [N] (log p / length ** A, and log p); the sampling flags
(--top-k, --top-p, --temperature, --slots) are ignored, with a note on stderr.
Originals and reconstructions are at most SVAE_TEXT_MAX_LEN = 2048 tokens, so --max-length is at most 2049.

--interpolate A B [--steps 9] [--interp-mode linear|slerp] decodes along the line between the posterior means of two
documents, given by title, or by row number when the batches have no titles, and prints one row of ids per step (text
when the data module has a tokenizer): the interpolation mode the reference's prompt announces.

Model and data are configured as for train.py, gather_latents.py and sample.py: an OmegaConf-style dotlist and a named
preset merged after it. Without --weights the model keeps its initial weights (useful only to try the pipeline); the
synthetic data mode works as it does for training:
    python reconstruct.py --preset tiny --max-batches 2 --max-length 48 --out /tmp/recon.npz
    python reconstruct.py --preset tiny --max-batches 1 --max-length 48 --interpolate 0 3 --steps 5
"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, 'sparse-vae_amd')):     # train.py (build_config) and the package
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser():
    ap = argparse.ArgumentParser(description='Reconstruct a corpus through its latents and score the result')
    ap.add_argument('--preset', default=None, help='named preset of hparam_presets.py (merged after the dotlist)')
    ap.add_argument('--weights', default=None, help='state_dict .pt of the trained TransformerVAE')
    ap.add_argument('--out', default='recon.npz', help='.npz to write')
    ap.add_argument('--split', choices=('test', 'train'), default='test', help='which loader to reconstruct')
    ap.add_argument('--max-batches', type=int, default=None, help='stop after this many batches')
    ap.add_argument('--max-length', type=int, default=512, help='decoded tokens + 1, at most SVAE_TEXT_MAX_LEN + 1')
    ap.add_argument('--slots', type=int, default=None, help='decoder rows (default: the batch, at most 1000)')
    ap.add_argument('--top-k', type=int, default=0)
    ap.add_argument('--top-p', type=float, default=0.9)
    ap.add_argument('--temperature', type=float, default=0.7)
    ap.add_argument('--repetition-penalty', type=float, default=1.2)
    ap.add_argument('--beams', type=int, default=None, help='decode by beam search with this many beams (1..16)')
    ap.add_argument('--length-penalty', type=float, default=1.0, help='with --beams: score = log p / length ** A')
    ap.add_argument('--start-token', type=int, default=None, help='default: the model\'s ([CLS] = 1)')
    ap.add_argument('--end-token', type=int, default=None, help='default: the model\'s ([SEP] = 2)')
    ap.add_argument('--sample-posterior', action='store_true', help='decode from a posterior draw, not the mean')
    ap.add_argument('--seed', type=int, default=0, help='torch.manual_seed before decoding; keys the posterior draws')
    ap.add_argument('--json', action='store_true', help='print the figures as one JSON line')
    ap.add_argument('--interpolate', nargs=2, metavar=('A', 'B'), default=None,
                    help='two documents (titles, or row numbers) to decode between instead of scoring')
    ap.add_argument('--steps', type=int, default=9, help='latents along the line, endpoints included')
    ap.add_argument('--interp-mode', choices=('linear', 'slerp'), default='linear')
    ap.add_argument('--device', default=None, help="torch device (default: 'cuda')")
    ap.add_argument('overrides', nargs='*', help='model.key=value / data.key=value, as for train.py')
    return ap


def _titles(batch):
    titles = batch.get('title') if hasattr(batch, 'get') else None
    if titles is None:
        return None
    return [t if isinstance(t, str) else ''.join(t) for t in titles]


def interpolate(model, data, loader, args, gen, end):
    """Decode --steps latents between the posterior means of documents A and B; returns the ids [steps, T - 1]."""
    import torch
    from sparse_vae import interpolate_latents, trim_samples
    want, found, row0 = list(args.interpolate), {}, 0
    for batch in loader:
        titles = _titles(batch)
        n = batch['num_tokens'].shape[0]
        names = titles if titles is not None else [str(row0 + i) for i in range(n)]
        hits = {w: names.index(w) for w in want if w not in found and w in names}
        if hits:
            loc = model.encode(batch).loc
            for w, i in hits.items():
                found[w] = loc[i, 0].clone()
        row0 += n
        if len(found) == len(set(want)):
            break
    missing = [w for w in want if w not in found]
    if missing:
        raise SystemExit(f'no document named {missing} in the {row0} documents read (titles, or row numbers where the '
                         f'batches have no titles)')
    z = interpolate_latents(found[want[0]], found[want[1]], args.steps, mode=args.interp_mode)
    if args.beams is not None:
        res = model.beam_search(args.max_length, z, num_beams=args.beams, length_penalty=args.length_penalty,
                                repetition_penalty=args.repetition_penalty)
        out, scores = res.ids[:, 0].to(torch.int16), res.scores[:, 0].tolist()
    else:
        out, scores = model.sample_stream(args.max_length, args.steps, slots=args.slots, z=z, **gen), None
    if out is None:
        raise SystemExit('the model does not sample below kl_weight 1')
    for i, row in enumerate(trim_samples(out, end)):
        text = data.tokenizer.decode(row.tolist()) if not data.synthetic else ' '.join(str(t) for t in row.tolist())
        print(f'[{i / (args.steps - 1):.3f}] {text}' + (f'  ({scores[i]:.4f})' if scores is not None else ''))
    return out.cpu().numpy()


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch
    from train import build_config
    from sparse_vae import (ReconstructionScores, TextDataModule, TransformerVAE, TransformerVAEHparams, reference_rows,
                            score_reconstructions)
    from sparse_vae._native import TEXT_MAX_LEN
    T = args.max_length
    if not 3 <= T <= TEXT_MAX_LEN + 1:
        raise SystemExit(f'--max-length {T}: 3..{TEXT_MAX_LEN + 1} (rows of at most SVAE_TEXT_MAX_LEN = {TEXT_MAX_LEN} '
                         f'tokens are scored)')
    config = build_config(list(args.overrides) + ([f'preset={args.preset}'] if args.preset else []))
    model = TransformerVAE(TransformerVAEHparams(**config['model']), device=args.device)
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location='cpu'))
    model.eval()
    if args.start_token is not None:
        model.start_token = args.start_token
    if args.end_token is not None:
        model.end_token = args.end_token
    end = model.end_token if model.end_token is not None else 2
    gen = dict(top_k=args.top_k, top_p=args.top_p, temperature=args.temperature,
               repetition_penalty=args.repetition_penalty)
    beam = {}
    if args.beams is not None:
        if not 1 <= args.beams <= 16:
            raise SystemExit(f'--beams {args.beams}: 1..16')
        beam = dict(num_beams=args.beams, length_penalty=args.length_penalty)
        print('--beams: beam search decoding; --top-k, --top-p, --temperature and --slots are ignored',
              file=sys.stderr)
    data = TextDataModule(**config.get('data', {}))
    data.prepare_data()
    data.setup('predict')
    loader = data.test_dataloader() if args.split == 'test' else data.train_dataloader()
    if args.max_batches is not None:
        loader = itertools.islice(loader, args.max_batches)
    torch.manual_seed(args.seed)
    if args.interpolate is not None:
        if args.steps < 2:
            raise SystemExit('--steps: at least the two endpoints')
        return interpolate(model, data, loader, args, gen, end)

    window = T - 1
    parts, ids_out, titles, truncated, beam_scores, beam_logp = [], [], [], 0, [], []
    for k, batch in enumerate(loader):
        ref, ref_len = reference_rows(batch)
        ref, ref_len = ref.to(model.device), ref_len.to(model.device)
        truncated += int((ref_len > window).sum())
        ref, ref_len = ref[:, :window], ref_len.clamp(max=window)
        ids, _ = model.autoencode(batch, max_length=T, sample_posterior=args.sample_posterior, slots=args.slots,
                                  seed=args.seed + k, **beam, **gen)
        if beam:
            beam_scores.append(model.last_beam_result.scores[:, 0].cpu().numpy())
            beam_logp.append(model.last_beam_result.log_probs[:, 0].cpu().numpy())
        parts.append(score_reconstructions(ids, ref, ref_lengths=ref_len, end_token=end))
        ids_out.append(ids.cpu().numpy())
        t = _titles(batch)
        if t is not None:
            titles += t
    if not parts:
        raise SystemExit('the loader gave no batches')
    scores = ReconstructionScores.cat(parts)
    figures = dict(scores.summary(), documents=len(scores), truncated=truncated)
    hparams = dict(model=dict(config['model']),
                   generation=dict(gen, max_length=T, slots=args.slots, end_token=end, seed=args.seed,
                                   sample_posterior=bool(args.sample_posterior), **beam))
    i32 = lambda a: np.asarray(a).astype(np.int32)                    # noqa: E731
    saved = dict(ids=np.concatenate(ids_out).astype(np.int16), lengths=i32(scores.cand_len),
                 matches=i32(scores.matches), totals=i32(scores.totals), exact=i32(scores.exact),
                 edit=i32(scores.edit), ref_len=i32(scores.ref_len), hparams=json.dumps(hparams, default=str))
    if beam:
        saved['beam_scores'] = np.concatenate(beam_scores).astype(np.float32)
        saved['beam_log_probs'] = np.concatenate(beam_logp).astype(np.float32)
    if titles:
        saved['titles'] = np.array(titles)
    np.savez(args.out, **saved)
    if args.json:
        print(json.dumps(figures))
    else:
        print(f'{figures["documents"]} documents ({truncated} cut to {window} tokens) -> {args.out}\n'
              f'corpus BLEU-4 {figures["corpus_bleu"]:.4f}  BLEU-2 {figures["bleu2"]:.4f}  '
              f'mean sentence BLEU-4 (smoothed) {figures["sentence_bleu"]:.4f}\n'
              f'token accuracy {figures["token_accuracy"]:.4f}  TER {figures["ter"]:.4f}  '
              f'mean length {figures["mean_cand_len"]:.1f} (originals {figures["mean_ref_len"]:.1f})')
    return figures


if __name__ == '__main__':
    main()
