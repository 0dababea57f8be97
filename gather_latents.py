"""python gather_latents.py --weights model.pt --out latents.npz [--preset NAME] [section.key=value ...]

Encode a corpus to its posterior latents: every batch of the data module's test (or train) loader goes through
TransformerVAE.encode (encoder only) and the (mean, scale) rows, with the documents' titles where the batches carry
them, are saved as one .npz that knn.py and sparse_vae.LatentIndex.load read back.

Model and data are configured as for train.py: an OmegaConf-style dotlist (model.*, data.*) and a named preset
merged after it. --weights is a state_dict saved with torch.save(model.state_dict(), path); without it the model keeps
its initial weights (useful only to try the pipeline). The synthetic data mode works as it does for training:
    python gather_latents.py --preset tiny --out /tmp/latents.npz --max-batches 4
"""
import argparse
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.abspath(__file__))
for _p in (ROOT, os.path.join(ROOT, 'sparse-vae_amd')):     # train.py (build_config) and the package
    if _p not in sys.path:
        sys.path.insert(0, _p)


def build_parser():
    ap = argparse.ArgumentParser(description='Gather the posterior latents of a corpus into a LatentIndex .npz')
    ap.add_argument('--preset', default=None, help='named preset of hparam_presets.py (merged after the dotlist)')
    ap.add_argument('--weights', default=None, help='state_dict .pt of the trained TransformerVAE')
    ap.add_argument('--out', required=True, help='index .npz to write')
    ap.add_argument('--split', choices=('test', 'train'), default='test', help='which loader to encode')
    ap.add_argument('--max-batches', type=int, default=None, help='stop after this many batches')
    ap.add_argument('--device', default=None, help="torch device (default: 'cuda')")
    ap.add_argument('overrides', nargs='*', help='model.key=value / data.key=value, as for train.py')
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from train import build_config
    from sparse_vae import TransformerVAE, TransformerVAEHparams, TextDataModule, gather_latents
    config = build_config(list(args.overrides) + ([f'preset={args.preset}'] if args.preset else []))
    model = TransformerVAE(TransformerVAEHparams(**config['model']), device=args.device)
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location='cpu'))
    model.eval()
    data = TextDataModule(**config.get('data', {}))
    data.prepare_data()
    data.setup('predict')
    loader = data.test_dataloader() if args.split == 'test' else data.train_dataloader()
    if args.max_batches is not None:
        loader = itertools.islice(loader, args.max_batches)
    index = gather_latents(model, loader)
    index.save(args.out)
    print(f'{len(index)} posteriors (latent depth {index.latent_depth}) -> {args.out}')
    return index


if __name__ == '__main__':
    main()
