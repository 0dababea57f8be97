"""ctypes binding of libsvae.so (the C ABI declared in include/svae.h).

There is deliberately no fallback: if the HIP library is missing or fails to load, importing the model
raises. Every wrapper validates shapes/dtypes/devices on the host before the call and raises
RuntimeError on a non-zero status.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('SVAE_LIB') or os.path.join(_HERE, 'libsvae.so')   # SVAE_LIB: A/B builds

c_void_p, c_int32, c_int64, c_float, c_uint64 = (ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64,
                                                  ctypes.c_float, ctypes.c_uint64)
c_fptr = ctypes.c_void_p

EPI_BF16, EPI_F32, EPI_F32_ACC, EPI_F32_ATOMIC, EPI_GELU, EPI_GELU_BWD, EPI_DROPOUT_RESID, \
    EPI_ROTARY_BF16, EPI_CE_STATS, EPI_CE_PROB, EPI_ROWSCALE_GATHER = range(11)

LATENT_L2, LATENT_COSINE, LATENT_KL = range(3)      # enum svae_latent_metric
LATENT_METRICS = {'l2': LATENT_L2, 'cosine': LATENT_COSINE, 'kl': LATENT_KL}
LATENT_MAX_BLOCKS = 1024                             # SVAE_LATENT_MAX_BLOCKS
TSNE_ROWS_PER_BLOCK, TSNE_TILE_COLS = 512, 256       # SVAE_TSNE_ROWS_PER_BLOCK, SVAE_TSNE_TILE_COLS
PAIR_RBF, PAIR_IMQ = range(2)                        # SVAE_PAIR_RBF, SVAE_PAIR_IMQ
PAIR_KINDS = {'rbf': PAIR_RBF, 'imq': PAIR_IMQ}
PAIRSUM_TILE_COLS, PAIRSUM_MAX_P, MMD_REDUCE_BLOCKS = 32, 8, 256   # SVAE_PAIRSUM_TILE_COLS, _MAX_P, SVAE_MMD_REDUCE_BLOCKS
# SVAE_KMEANS_MAX_K, _TILE_CENTROIDS, _SORT_BLOCKS, _SEED_BLOCK_ROWS
KMEANS_MAX_K, KMEANS_TILE_CENTROIDS, KMEANS_SORT_BLOCKS, KMEANS_SEED_BLOCK_ROWS = 1024, 32, 256, 256
# SVAE_GMM_MAX_K, _TILE_COMPONENTS, _ROWS_PER_BLOCK
GMM_MAX_K, GMM_TILE_COMPONENTS, GMM_ROWS_PER_BLOCK = 256, 16, 256
# SVAE_AGGPOST_POINTS_PER_BLOCK, _TILE_ROWS, _PASS_DIMS
AGGPOST_POINTS_PER_BLOCK, AGGPOST_TILE_ROWS, AGGPOST_PASS_DIMS = 256, 16, 16
TEXT_MAX_LEN = 2048                                  # SVAE_TEXT_MAX_LEN
BEAM_MAX_W = 16                                      # SVAE_BEAM_MAX_W


class GemmDesc(ctypes.Structure):
    _fields_ = [
        ('A', c_void_p), ('B', c_void_p),
        ('lda', c_int64), ('ldb', c_int64), ('batch_stride_a', c_int64), ('batch_stride_b', c_int64),
        ('M', c_int32), ('N', c_int32), ('K', c_int32),
        ('batch', c_int32), ('splits', c_int32),
        ('a_t', c_int32), ('b_t', c_int32),
        ('epi', c_int32),
        ('C', c_void_p),
        ('ldc', c_int64), ('batch_stride_c', c_int64),
        ('bias', c_void_p), ('resid', c_void_p), ('ldr', c_int64),
        ('aux', c_void_p), ('ldaux', c_int64),
        ('alpha', c_float), ('drop_p', c_float), ('seed', c_uint64),
        ('rot_tab', c_void_p), ('rot_cols', c_int32), ('rot_d', c_int32), ('rot_seq', c_int32),
        ('labels', c_void_p), ('label_logit', c_void_p),
        ('a_rowsum', c_void_p),
        ('k_weight', c_void_p), ('row_a', c_void_p), ('row_b', c_void_p), ('gather', c_void_p), ('ldg', c_int64),
        ('delta', c_void_p), ('delta_o32', c_void_p), ('ld_o32', c_int64), ('delta_hd', c_int32), ('delta_seq', c_int32),
    ]


class AttnDesc(ctypes.Structure):
    _fields_ = [
        ('q', c_void_p), ('k', c_void_p), ('v', c_void_p), ('o', c_void_p),
        ('sq', c_int64), ('sk', c_int64), ('sv', c_int64), ('so', c_int64),
        ('bq', c_int64), ('bk', c_int64), ('bv', c_int64), ('bo', c_int64),
        ('key_pad', c_void_p), ('lse', c_void_p),
        ('B', c_int32), ('H', c_int32), ('Lq', c_int32), ('Lk', c_int32), ('hd', c_int32), ('causal', c_int32),
        ('scale', c_float),
        ('dout', c_void_p), ('sdo', c_int64), ('bdo', c_int64),
        ('delta', c_void_p), ('dq', c_void_p), ('bdq', c_int64),
        ('dk', c_void_p), ('dv', c_void_p),
        ('sdk', c_int64), ('sdv', c_int64), ('bdk', c_int64), ('bdv', c_int64),
        ('rot_tab', c_void_p), ('rot_d', c_int32),
        ('o32', c_void_p), ('so32', c_int64), ('bo32', c_int64),
        ('dq_part', c_void_p), ('dq_bf', c_void_p), ('ldq_bf', c_int64),
        ('window', c_int32),
        ('delta_ready', c_int32),
        ('o_lo', c_void_p), ('so_lo', c_int64), ('bo_lo', c_int64),
        ('fwd_ws', c_void_p), ('fwd_ws_elems', c_int64),
    ]


GROUP_MAX = 256         # SVAE_GROUP_MAX
COLSUM_MAX = 8
LN_MULTI_MAX = 4        # SVAE_LN_MULTI_MAX


ZPROJ_MAX = 32


class ZprojSeg(ctypes.Structure):
    """svae_zproj_seg (include/svae.h)."""
    _fields_ = [('g', c_void_p), ('W', c_void_p), ('dW', c_void_p), ('db', c_void_p)]


class ZprojFwdSeg(ctypes.Structure):
    """svae_zproj_fwd_seg (include/svae.h)."""
    _fields_ = [('W', c_void_p), ('bias', c_void_p), ('out', c_void_p)]


class ColsumSeg(ctypes.Structure):
    """svae_colsum_seg (include/svae.h)."""
    _fields_ = [('inp', c_void_p), ('out', c_void_p), ('ld', c_int64), ('rows', c_int32), ('cols', c_int32)]


_SIGS = {
    'svae_gemm': [ctypes.POINTER(GemmDesc), c_void_p],
    'svae_gemm_pair': [ctypes.POINTER(GemmDesc), ctypes.POINTER(GemmDesc), c_void_p],
    'svae_gemm_group_table_bytes': [c_int32],
    'svae_gemm_group': [ctypes.POINTER(GemmDesc), c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p],
    'svae_resid_ln_fwd': [c_void_p, c_void_p, c_int32, c_int64, c_float, c_uint64, c_void_p, c_int32, c_void_p,
                          c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_layernorm_fwd': [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                           c_void_p],
    'svae_layernorm_bwd': [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p],
    'svae_layernorm_bwd_drop': [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_float, c_uint64, c_int32,
                                c_void_p, c_void_p, c_void_p],
    'svae_layernorm_bwd_gelu': [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                c_void_p, c_int32, c_int32, c_int32, c_void_p],
    'svae_layernorm_nblk': [c_int32],
    'svae_colsum': [c_void_p, c_int32, c_int32, c_int32, c_int64, c_void_p, c_int32, c_void_p],
    'svae_colsum_multi': [c_void_p, c_int32, c_void_p],
    'svae_attn_fwd': [ctypes.POINTER(AttnDesc), c_void_p],
    'svae_attn_bwd': [ctypes.POINTER(AttnDesc), c_void_p],
    'svae_attn_dq_part_elems': [c_int32, c_int32, c_int32, c_int32, c_int32],
    'svae_attn_dq_part_elems_w': [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32],
    'svae_attn_fwd_ws_elems': [c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32],
    'svae_transpose_blocks': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_dq_finalize': [c_void_p, c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p],
    'svae_embedding_fwd': [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_embedding_fwd_dual': [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_embedding_bwd': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_reparam_kl_fwd': [c_void_p, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                            c_void_p, c_int32, c_int32, c_void_p],
    'svae_reparam_kl_bwd': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_ce_finalize': [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_ce_weighted_nll': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                             c_void_p],
    'svae_ce_red_ws_elems': [c_int32],
    'svae_clip_grad': [c_void_p, c_int64, c_void_p, c_int32, c_float, c_void_p, c_void_p],
    'svae_ce_label_logit': [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                            c_void_p],
    'svae_ce_prob_finalize': [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                              c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_ce_prob_finalize_fix': [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p,
                                  c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p,
                                  c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p],
    'svae_ce_prob_bwd_prep': [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                              c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_embedding_bwd_ce': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p],
    'svae_ce_grad': [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32,
                     c_int32, c_int32, c_void_p],
    'svae_dropout_bwd_cast': [c_void_p, c_void_p, c_float, c_uint64, c_int64, c_int32, c_int64, c_void_p],
    'svae_gelu_bwd': [c_void_p, c_void_p, c_void_p, c_int64, c_void_p],
    'svae_prep_tokens': [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p],
    'svae_step_scalars': [c_void_p, c_void_p, c_void_p, c_float, c_void_p, c_void_p, c_void_p],
    'svae_zproj_bwd_multi': [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    'svae_zproj_fwd_multi': [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    'svae_layernorm_fwd_multi': [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                                 c_void_p],
    'svae_layernorm_bwd_multi': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p,
                                 c_int32, c_int32, c_int32, c_int32, c_void_p],
    'svae_layernorm_fwd_z': [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32,
                             c_int32, c_void_p],
    'svae_cast_bf16': [c_void_p, c_void_p, c_int64, c_void_p],
    'svae_extract_rows': [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p],
    'svae_zproj_bwd': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    'svae_sumsq': [c_void_p, c_int64, c_void_p, c_int32, c_void_p],
    'svae_radam': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_void_p,
                   c_void_p, c_void_p],
    'svae_gemm_f32': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int64, c_int64, c_int64, c_void_p,
                      c_void_p, c_int64, c_int32, c_void_p, c_int32, c_int32, c_int32, c_void_p],
    'svae_attn_fwd_f32': [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int64, c_int64, c_int64, c_int64,
                          c_int64, c_int64, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32, c_int32,
                          c_float, c_void_p],
    'svae_layernorm_fwd_f32': [c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_ce_seq_logprob': [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    'svae_dec_linear': [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32,
                        c_int32, c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p],
    'svae_dec_attn': [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                      c_float, c_void_p, c_int64, c_void_p],
    'svae_dec_embed': [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_dec_penalty': [c_void_p, c_int64, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_float,
                         c_void_p],
    'svae_dec_sample': [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_int32,
                        c_float, c_int32, c_float, c_uint64, c_void_p, c_void_p],
    'svae_dec_advance': [c_void_p, c_void_p],
    'svae_slot_linear': [c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int32,
                         c_int32, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_int64, c_void_p],
    'svae_slot_attn': [c_void_p, c_int64, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32,
                       c_float, c_void_p, c_int64, c_void_p],
    'svae_slot_embed': [c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_slot_splice': [c_void_p, c_void_p, c_int64, c_void_p, c_int32, c_int32, c_void_p],
    'svae_slot_penalty': [c_void_p, c_int64, c_int32, c_void_p, c_int32, c_void_p, c_float, c_void_p],
    'svae_slot_sample': [c_void_p, c_int64, c_int32, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32,
                         c_int32, c_float, c_int32, c_float, c_uint64, c_void_p],
    'svae_slot_refill': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_int32, c_int32,
                         c_void_p, c_void_p, c_void_p],
    'svae_beam_attn': [c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_int32, c_int32, c_int32,
                       c_void_p, c_int32, c_float, c_void_p, c_int64, c_void_p],
    'svae_beam_topk': [c_void_p, c_int64, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_beam_select': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32,
                         c_int32, c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_beam_finalize': [c_void_p, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_mutual_info': [c_void_p, c_void_p, c_uint64, c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p,
                         c_void_p],
    'svae_latent_prepare': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p],
    'svae_latent_scores': [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    'svae_latent_topk_ws_bytes': [c_int32, c_int32],
    'svae_latent_topk': [c_int32, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p,
                         c_void_p, c_int32, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p],
    'svae_tsne_affinities': [c_void_p, c_int32, c_int32, c_float, c_void_p, c_void_p, c_void_p],
    'svae_tsne_repulse_slice_cols': [c_int32],
    'svae_tsne_repulse_ws_bytes': [c_int32],
    'svae_tsne_repulse': [c_void_p, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p],
    'svae_tsne_attract': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p],
    'svae_tsne_update': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_float, c_float,
                         c_float, c_void_p],
    'svae_pairsum_geometry': [c_int32, c_int32, c_int32, c_int32, c_void_p],
    'svae_pairsum_ws_bytes': [c_int32, c_int32, c_int32, c_int32],
    'svae_pairsum': [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_int32, c_int32, c_void_p, c_int32, c_void_p,
                     c_void_p, c_int64, c_void_p, c_void_p],
    'svae_mmd_rowterm_ws_bytes': [c_int32],
    'svae_mmd_rowterm': [c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p],
    'svae_latent_colstats_ws_bytes': [c_int32, c_int32],
    'svae_latent_colstats': [c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_int64, c_void_p, c_void_p, c_void_p,
                             c_void_p],
    'svae_latent_draw': [c_void_p, c_void_p, c_void_p, c_uint64, c_int32, c_int32, c_void_p, c_void_p],
    'svae_kmeans_geometry': [c_int32, c_int32, c_int32, c_void_p],
    'svae_kmeans_assign_ws_bytes': [c_int32, c_int32, c_int32],
    'svae_kmeans_assign': [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                           c_void_p, c_int64, c_void_p],
    'svae_kmeans_update_ws_bytes': [c_int32, c_int32, c_int32],
    'svae_kmeans_update': [c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_int64,
                           c_void_p],
    'svae_kmeans_seed_ws_bytes': [c_int32, c_int32, c_int32],
    'svae_kmeans_seed': [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_uint64, c_void_p, c_void_p, c_void_p,
                         c_int64, c_void_p],
    'svae_gmm_params_floats': [c_int32, c_int32],
    'svae_gmm_geometry': [c_int32, c_int32, c_int32, c_int32, c_void_p],
    'svae_gmm_prepare': [c_void_p, c_int32, c_int32, c_void_p],
    'svae_gmm_estep_ws_bytes': [c_int32, c_int32, c_int32],
    'svae_gmm_estep': [c_void_p, c_void_p, c_int32, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p, c_void_p,
                       c_void_p, c_int64, c_void_p],
    'svae_gmm_mstep_ws_bytes': [c_int32, c_int32, c_int32],
    'svae_gmm_mstep': [c_void_p, c_void_p, c_int32, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_float, c_void_p,
                       c_void_p, c_int64, c_void_p],
    'svae_gmm_sample': [c_void_p, c_int32, c_int32, c_int32, c_void_p, c_void_p, c_uint64, c_void_p, c_void_p,
                        c_void_p],
    'svae_aggpost_geometry': [c_int32, c_int32, c_int32, c_int32, c_void_p],
    'svae_aggpost_ws_bytes': [c_int32, c_int32, c_int32, c_int32],
    'svae_aggpost_logq': [c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_int32, c_void_p, c_void_p, c_void_p,
                          c_void_p, c_int64, c_void_p],
    'svae_aggpost_decompose_ws_bytes': [c_int32, c_int32],
    'svae_aggpost_decompose': [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_int32, c_void_p,
                               c_int64, c_void_p, c_void_p],
    'svae_ngram_overlap': [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    'svae_edit_distance': [c_void_p, c_int32, c_void_p, c_int32, c_void_p, c_void_p, c_int32, c_void_p, c_void_p],
    'svae_version': [],
}


def _load():
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f'libsvae.so not found at {LIB_PATH}: build it with `make -C sparse-vae_amd` '
                           f'(or __graft_entry__.build()). There is no CPU fallback.')
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in _SIGS.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = {'svae_version': ctypes.c_char_p, 'svae_attn_dq_part_elems': c_int64,
                      'svae_attn_dq_part_elems_w': c_int64, 'svae_attn_fwd_ws_elems': c_int64,
                      'svae_latent_topk_ws_bytes': c_int64,
                      'svae_tsne_repulse_slice_cols': c_int64, 'svae_tsne_repulse_ws_bytes': c_int64,
                      'svae_pairsum_ws_bytes': c_int64, 'svae_mmd_rowterm_ws_bytes': c_int64,
                      'svae_latent_colstats_ws_bytes': c_int64,
                      'svae_kmeans_assign_ws_bytes': c_int64, 'svae_kmeans_update_ws_bytes': c_int64,
                      'svae_kmeans_seed_ws_bytes': c_int64,
                      'svae_gmm_params_floats': c_int64, 'svae_gmm_estep_ws_bytes': c_int64,
                      'svae_gmm_mstep_ws_bytes': c_int64,
                      'svae_aggpost_ws_bytes': c_int64, 'svae_aggpost_decompose_ws_bytes': c_int64,
                      'svae_gemm_group_table_bytes': c_int64}.get(name, ctypes.c_int)
    return lib


lib = _load()
EXPORTED = tuple(_SIGS)


def check(status, name):
    if status != 0:
        raise RuntimeError(f'{name} failed with status {status}')


def ptr(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream
