"""python sample.py --weights model.pt --num-samples 700000 --out samples.npz [--preset NAME] [section.key=value ...]

Mass unconditional sampling (the reference's sample.py): draw --num-samples texts of up to --max-length tokens from
the prior and save them as one .npz with
    ids      int16 [N, max_length - 1], zero after each sample's end,
    lengths  int32 [N], tokens up to and including the first end token (the full width where there is none),
    hparams  the model's hyperparameters and the generation settings, as a JSON string.
The default path is TransformerVAE.sample_stream: --slots decoder rows, each refilled on the device with the next
sample as soon as its current one ends. --loop runs the reference's batch-synchronous loop instead
(batch_generate_samples over model.sample at batch size --slots), for comparison.

--prior prior.npz (written by fit_prior.py) draws z from that Gaussian mixture instead of N(0, I) and passes it as z=
to sample_stream, or to model.sample under --loop; the component draw and the normals are seeded from --seed. The .npz
then also holds `components` int32 [N], the mixture component behind each sample, and the prior's path among the
generation settings. Without --prior nothing changes, the .npz's keys included.

Model configuration is as for train.py and gather_latents.py: an OmegaConf-style dotlist (model.*) and a named preset
merged after it. Without --weights the model keeps its initial weights (useful only to try the pipeline):
    python sample.py --preset tiny --num-samples 40 --slots 8 --max-length 32 --out /tmp/samples.npz
"""
import argparse
import json
import os
import sys
from functools import partial

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, 'sparse-vae_amd')):     # train.py (build_config) and the package
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser():
    ap = argparse.ArgumentParser(description='Draw samples from the prior of a TransformerVAE into an .npz')
    ap.add_argument('--preset', default=None, help='named preset of hparam_presets.py (merged after the dotlist)')
    ap.add_argument('--weights', default=None, help='state_dict .pt of the trained TransformerVAE')
    ap.add_argument('--out', default='samples.npz', help='.npz to write')
    ap.add_argument('--num-samples', type=int, default=700_000)
    ap.add_argument('--max-length', type=int, default=512)
    ap.add_argument('--slots', type=int, default=1000, help='decoder rows (the batch size of --loop)')
    ap.add_argument('--top-k', type=int, default=0)
    ap.add_argument('--top-p', type=float, default=0.9)
    ap.add_argument('--temperature', type=float, default=1.0)
    ap.add_argument('--repetition-penalty', type=float, default=1.2)
    ap.add_argument('--start-token', type=int, default=None, help='default: the model\'s ([CLS] = 1)')
    ap.add_argument('--end-token', type=int, default=None, help='default: the model\'s ([SEP] = 2)')
    ap.add_argument('--seed', type=int, default=None, help='torch.manual_seed before sampling')
    ap.add_argument('--prior', default=None, help='mixture .npz of fit_prior.py: draw z from it instead of N(0, I)')
    ap.add_argument('--loop', action='store_true', help='the batch-synchronous loop over model.sample')
    ap.add_argument('--device', default=None, help="torch device (default: 'cuda')")
    ap.add_argument('overrides', nargs='*', help='model.key=value, as for train.py')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import numpy as np
    import torch
    from train import build_config
    from sparse_vae import TransformerVAE, TransformerVAEHparams, batch_generate_samples, trim_samples
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
    if args.seed is not None:
        torch.manual_seed(args.seed)
    N, T = args.num_samples, args.max_length
    comp = None
    if args.prior:
        from sparse_vae import GaussianMixture
        prior = GaussianMixture.load(args.prior, model.device)
        if prior.means_.shape[1] != model.hparams.latent_depth:
            raise SystemExit(f'{args.prior} has rows of {prior.means_.shape[1]}, the model a latent depth of '
                             f'{model.hparams.latent_depth}')
        z, comp = prior.sample(N, seed=args.seed or 0)
    if args.prior and args.loop:
        bs, start = min(args.slots, max(N, 1)), [0]

        def next_batch():                            # the last batch may be short: the helper truncates anyway
            zb = z[start[0]:start[0] + bs]
            start[0] += bs
            return model.sample(T, zb.shape[0], z=zb, **gen)
        rows = batch_generate_samples(next_batch, N, T, end)
    elif args.prior:
        out = model.sample_stream(T, N, slots=min(args.slots, max(N, 1)), z=z, **gen)
        if out is None:
            raise SystemExit('the model does not sample below kl_weight 1')
        rows = trim_samples(out, end)
    elif args.loop:
        rows = batch_generate_samples(partial(model.sample, T, min(args.slots, max(N, 1)), **gen), N, T, end)
    else:
        out = model.sample_stream(T, N, slots=min(args.slots, max(N, 1)), **gen)
        if out is None:
            raise SystemExit('the model does not sample below kl_weight 1')
        rows = trim_samples(out, end)
    ids = np.zeros((N, T - 1), dtype=np.int16)
    for i, r in enumerate(rows):
        ids[i, :len(r)] = r.numpy()
    lengths = np.array([len(r) for r in rows], dtype=np.int32)
    hparams = dict(model=dict(config['model']), generation=dict(gen, max_length=T, slots=args.slots, end_token=end,
                                                                seed=args.seed, loop=bool(args.loop)))
    extra = {}
    if args.prior:
        hparams['generation']['prior'] = args.prior
        extra['components'] = comp.cpu().numpy().astype(np.int32)
    np.savez(args.out, ids=ids, lengths=lengths, hparams=json.dumps(hparams, default=str), **extra)
    print(f'{N} samples (mean length {lengths.mean() if N else 0:.1f}) -> {args.out}')
    return ids, lengths


if __name__ == '__main__':
    main()
