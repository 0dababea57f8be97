"""sparse-vae on MI355X: the TransformerVAE training hot path of norabelrose/sparse-vae on hand-written gfx950
kernels (libsvae.so, C ABI in include/svae.h), behind the reference's Python surface."""
from .core import *  # noqa: F401,F403
from .core import PaddedTensor, RAdam, marginal_kl, pairwise_gaussian_kl  # noqa: F401
from .core import analytic_gaussian_rbf_mmd_sq, custom_gaussian_rbf_mmd_sq, gaussian_imq_mmd_sq  # noqa: F401
from .transformer_vae import TransformerVAE, TransformerVAEHparams  # noqa: F401
from .decoding import BeamDecoder, BeamResult  # noqa: F401
from .latent_index import LatentIndex, gather_latents  # noqa: F401
from .tsne import TSNE  # noqa: F401
from .kmeans import KMeans  # noqa: F401
from .mixture import GaussianMixture  # noqa: F401
from .surgery import ElboSurgery  # noqa: F401
from .reconstruction import (ReconstructionScores, interpolate_latents, reference_rows,  # noqa: F401
                             score_reconstructions)
from .batch_generation import batch_generate_samples, trim_samples  # noqa: F401
from .text_data_module import TextDataModule  # noqa: F401
from .trainer import Trainer, seed_everything  # noqa: F401
from .core.auto_select_gpu import select_best_gpu  # noqa: F401
