/*
 * svae.h — C ABI of libsvae.so, the MI355X (gfx950) kernels behind the sparse-vae TransformerVAE
 * training step.
 *
 * The reference (norabelrose/sparse-vae) has NO native layer: its hot path is PyTorch ATen ops called
 * from nn.Modules. Each entry point below replaces the ATen op sequence of one
 * reference call site (cited per function); the Python host package (sparse-vae_amd/sparse_vae) keeps
 * the reference's nn.Module / LightningModule surface and calls these through ctypes.
 *
 * Conventions (all entry points):
 *   - device pointers are plain addresses of memory owned by the caller (PyTorch's caching allocator);
 *     the library never allocates, frees or synchronises;
 *   - element types: bf16 = 16-bit bfloat16 storage, f32 = IEEE float;
 *   - `stream` is a hipStream_t; work is enqueued asynchronously on it;
 *   - return 0 on success, SVAE_EINVAL (1) on a bad argument (nothing launched), SVAE_ELAUNCH (2) if
 *     the launch failed. The Python layer raises RuntimeError on any non-zero status.
 */
#ifndef SVAE_H
#define SVAE_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef void* svae_stream_t; /* hipStream_t */

/* ---- GEMM: C[M,N] = epi(alpha * A[M,K] . B[K,N]) ------------------------------------------------
 * Replaces nn.Linear forward (addmm) and its autograd backward (mm for dX and dW) at every Linear of
 * the path: attention.py:33-38,60,67,103; transformer_layer.py:17-21; transformer_language_model.py:55-63;
 * conditional_gaussian.py:18; transformer_vae.py:37-40,89.
 * a_t = 0: A stored [M][K] (lda >= K); a_t = 1: A stored [K][M] (lda >= M).
 * b_t = 0: B stored [N][K] (nn.Linear weight layout); b_t = 1: B stored [K][N].
 * Requirements: K % 8 == 0 unless a_t && b_t; for a_t: M % 8 == 0; for b_t: N % 8 == 0; lda, ldb % 8 == 0;
 * A, B 16-byte aligned; N, ldc (and ldr, ldaux) % 4 == 0 and C 8-byte aligned (vectorised epilogue). */
enum svae_epi {
  SVAE_EPI_BF16 = 0,          /* C bf16 = alpha*acc + bias                                            */
  SVAE_EPI_F32 = 1,           /* C f32  = alpha*acc + bias (+ resid); with aux != NULL (batch 1, ldaux %
                                 8 == 0) also aux bf16 = bf16(keep(seed, m*N+n) * C / (1 - p)) -- what
                                 svae_dropout_bwd_cast makes of C (drop_p 0: bf16(C))                  */
  SVAE_EPI_F32_ACC = 2,       /* C f32 += alpha*acc                                                   */
  SVAE_EPI_F32_ATOMIC = 3,    /* atomicAdd(C f32, alpha*acc)   (split-K / shared destinations); with
                                 splits > 1 and aux != NULL: each split stores its partial tile into the
                                 f32 workspace aux [splits][M][N] and a reduce pass adds them into C     */
  SVAE_EPI_GELU = 4,          /* C bf16 = gelu(acc + bias);  aux bf16 = gelu'(acc + bias)              */
  SVAE_EPI_GELU_BWD = 5,      /* C bf16 = acc * aux  (aux = the gelu' saved by SVAE_EPI_GELU)          */
  SVAE_EPI_DROPOUT_RESID = 6, /* C f32 = resid + keep(seed, m*N+n) * acc / (1 - p); with aux != NULL
                                 (batch 1, ldaux % 8 == 0) also aux bf16 = bf16(C)                    */
  SVAE_EPI_ROTARY_BF16 = 7,   /* C bf16 = rotary(acc + bias) on cols < rot_cols (attention.py:194-208) */
  SVAE_EPI_CE_STATS = 8,      /* C bf16 = acc + bias; per (row, 128-col tile) online (max, sumexp) to
                                 aux f32 [M][ceil(N/128)][2]; label logit (f32) to resid-as-out [M]   */
  SVAE_EPI_CE_PROB = 9,       /* vocab head, training: C bf16 = exp(acc + bias - row_a[m]) for rows with
                                 labels[m] != 0, else 0 (exponent clamped at 2^127); aux f32
                                 [ceil(N/128)][M] (tile-major) = per (128-col tile, row) sums of them  */
  SVAE_EPI_ROWSCALE_GATHER = 10 /* C bf16 = alpha * row_a[m] * acc - row_b[m] * gather[labels[m]][n]
                                 (the gather term is skipped where labels[m] == 0); N % 8 == 0 (the
                                 gather row is read 8 columns at a time), else SVAE_EINVAL            */
};

typedef struct svae_gemm_desc {
  const void* A;
  const void* B;
  int64_t lda, ldb, batch_stride_a, batch_stride_b;
  int32_t M, N, K;
  int32_t batch, splits;
  int32_t a_t, b_t;
  int32_t epi;
  void* C;
  int64_t ldc, batch_stride_c;
  const float* bias;        /* [N] f32 or NULL */
  const float* resid;       /* f32 [M][ldr] or NULL (DROPOUT_RESID / F32); may alias C */
  int64_t ldr;
  void* aux;                /* see svae_epi */
  int64_t ldaux;
  float alpha;
  float drop_p;
  uint64_t seed;
  const float* rot_tab;     /* [rot_seq][rot_d/2] x (cos, sin) f32 */
  int32_t rot_cols, rot_d, rot_seq;
  const int32_t* labels;    /* CE_STATS: [M] target column per row (0 = ignored) */
  float* label_logit;       /* CE_STATS: [M] f32 out */
  float* a_rowsum;          /* a_t only, optional: a_rowsum[m] += sum_k A[m][k] (bias grad of a dW GEMM) */
  /* optional with a_rowsum (a_t && b_t; splits 1 with F32_ACC, or split-K slab mode: F32_ATOMIC with aux):  */
  /* a_rowsum[m] += sum_k A[m][k] * k_weight[k]                                                            */
  const float* k_weight;
  const float* row_a;       /* CE_PROB / ROWSCALE_GATHER: [M] f32 (see svae_epi)                        */
  const float* row_b;       /* ROWSCALE_GATHER: [M] f32                                                  */
  const void* gather;       /* ROWSCALE_GATHER: bf16 rows [*][ldg], row labels[m] gathered; 16-B aligned */
  int64_t ldg;
  /* optional with SVAE_EPI_BF16 (the attention output projection's dO GEMM under autograd, attention.py:51-105):
   * also write the attention backward's row constants delta[(b * (N / delta_hd) + h) * delta_seq + q] = sum over
   * the head's delta_hd columns of bf16(C)[m][h * delta_hd + c] * delta_o32[m * ld_o32 + h * delta_hd + c], m = b *
   * delta_seq + q (delta_o32: the forward's f32 copy of O). delta is overwritten; svae_attn_bwd with delta_ready = 1
   * then skips its own delta pass. splits 1, batch 1, a_t 0; N % delta_hd == 0, delta_hd % 16 == 0, M % delta_seq == 0. */
  float* delta;
  const float* delta_o32;
  int64_t ld_o32;
  int32_t delta_hd, delta_seq;
} svae_gemm_desc;

int svae_gemm(const svae_gemm_desc* d, svae_stream_t stream);

/* Two weight-gradient GEMMs in one launch (engine.layer_bwd pairs the two dW GEMMs of the FFN, and the output
 * projection's with the QKV / K-V projection's: the nn.Linear weight gradients of transformer_layer.py:56-61 and
 * attention.py:51-105 under loss.backward()). Each desc as for svae_gemm with a_t = b_t = 1, epi
 * SVAE_EPI_F32_ATOMIC, splits >= 2 and a slab workspace in aux (aux[split][M][N] f32, then C += the sum of the
 * splits); the results equal two svae_gemm calls with the same descs. */
int svae_gemm_pair(const svae_gemm_desc* d0, const svae_gemm_desc* d1, svae_stream_t stream);

/* n weight-gradient GEMMs as one grouped pass (engine.backward defers every layer's nn.Linear weight gradients,
 * transformer_layer.py:56-61 and attention.py:51-105 under loss.backward(), to one call: the chip is filled across
 * layers instead of across K). d[0..n): each as for svae_gemm with a_t = b_t = 1, batch 1, and either splits == 1
 * with epi SVAE_EPI_F32_ACC (C += the product, one accumulation chain over K) or splits >= 1 with epi
 * SVAE_EPI_F32_ATOMIC and a slab workspace of its own in aux (as for svae_gemm_pair); a_rowsum as for svae_gemm. The
 * unsplit GEMMs run as one launch of 256 x 256 tiles, the split ones as a second, and one launch adds every slab
 * into its C in split order; the results equal n svae_gemm calls with the same descs.
 *   max_blocks: 0 = one block per compute unit; then the unsplit GEMMs together must not have more tiles than that
 *     (a second round of whole-K tiles would cost a full tile time: SVAE_EINVAL -- give the rest a split count).
 *     > 0 (<= SVAE_GROUP_MAX_BLOCKS): at most that many blocks per launch, which then walk several tiles each.
 *   table / table_host: the parameter table the kernels read, in device memory (16-byte aligned), and the caller's
 *     host copy of it, both of table_bytes >= svae_gemm_group_table_bytes(n) bytes and owned by the caller;
 *     table_host zeroed before its first use. The device table is written (a copy on `stream`, waited for) only
 *     when its contents differ from table_host, i.e. not in a step that repeats the previous step's addresses. */
#define SVAE_GROUP_MAX 256
#define SVAE_GROUP_MAX_BLOCKS 1024
int64_t svae_gemm_group_table_bytes(int32_t n);
int svae_gemm_group(const svae_gemm_desc* d, int32_t n, int32_t max_blocks, void* table, void* table_host,
                    int64_t table_bytes, svae_stream_t stream);

/* ---- LayerNorm ---------------------------------------------------------------------------------
 * nn.LayerNorm(d, eps=1e-5) forward/backward: transformer_layer.py:23-24,39-40,47,52,56;
 * transformer_language_model.py:59. x_dtype: 0 = f32 input, 1 = bf16 input. y is bf16.
 * Backward: dx = dres + LN'(dy) (dres may be NULL), written f32 to dx and (optionally) bf16 to dx_bf;
 * per-block partial (dw, db) sums go to part[nblk][2][D] (reduce with svae_colsum). Rows with
 * (row % zero_mod == 0) get dx = 0 when zero_mod > 0 (position-0 overwrite, transformer_vae.py:89-90). */
/* Residual add + dropout + LayerNorm forward (transformer_layer.py:49-50, :58-61 and the following LayerNorm, :47 / :56),
 * one pass: v = x[r] + dropout(y[r]) (x f32 [rows][D] or NULL; y bf16 [rows][ldy] -- the projection's output -- or
 * NULL; y_dtype 0 = f32, 1 = bf16; dropout with the counter RNG of SVAE_EPI_DROPOUT_RESID: seed, index (r * D + c) / 4),
 * or v = zrows[r / zmod]
 * where zrows != NULL and r % zmod == 0 (the z splice, transformer_vae.py:89-90); xo f32 = v (may be NULL);
 * h bf16 = LayerNorm(v) * w + b with mean / rstd, or h = bf16(v) when w == b == NULL. D % 8 == 0, D <= 1024. */
int svae_resid_ln_fwd(const float* x, const void* y, int32_t y_dtype, int64_t ldy, float drop_p, uint64_t seed,
                      const float* zrows, int32_t zmod, const float* w, const float* b, float* xo, void* h, float* mean,
                      float* rstd, int32_t rows, int32_t D, svae_stream_t stream);
int svae_layernorm_fwd(const void* x, int32_t x_dtype, const float* w, const float* b, void* y,
                       float* mean, float* rstd, int32_t rows, int32_t D, svae_stream_t stream);
int svae_layernorm_bwd(const void* dy, const void* x, int32_t x_dtype, const float* w, const float* mean,
                       const float* rstd, const float* dres, float* dx, void* dx_bf, float* part,
                       int32_t nblk, int32_t rows, int32_t D, int32_t zero_mod, svae_stream_t stream);
/* svae_layernorm_bwd for the last LayerNorm of a decoder layer's backward, with the two passes that followed it
 * fused in: (1) the bf16 copy dx_bf carries the NEXT layer's dropout backward (replaces svae_dropout_bwd_cast of
 * dx): dx_bf = bf16(keep(bf_seed, (row*D + c)/4) * dx / (1 - bf_drop_p)), the mask of the forward's
 * SVAE_EPI_DROPOUT_RESID epilogue with the same seed (transformer_layer.py:61, nn.Dropout), and dx_bf = 0 on rows
 * with row % bf_zero_mod == 0 (bf_zero_mod > 0); bf_drop_p in [0, 1). (2) with zero_mod > 0, the rows it zeroes in
 * dx are first written to zrow[row / zero_mod] (f32) and zrow_bf (bf16), either may be NULL: the gradient of the
 * position-0 z splice (transformer_vae.py:89-90; replaces svae_extract_rows + svae_cast_bf16). */
int svae_layernorm_bwd_drop(const void* dy, const void* x, int32_t x_dtype, const float* w, const float* mean,
                            const float* rstd, const float* dres, float* dx, void* dx_bf, float* part, int32_t nblk,
                            int32_t rows, int32_t D, int32_t zero_mod, float bf_drop_p, uint64_t bf_seed,
                            int32_t bf_zero_mod, float* zrow, void* zrow_bf, svae_stream_t stream);
/* svae_layernorm_bwd of the vocabulary head's LayerNorm (transformer_vae.py output_layer[2]) fused with the GELU
 * backward of the linear before it (output_layer[0..1]): out_bf = bf16(LN'(dy) * gp), gp the bf16 GELU' the forward's
 * SVAE_EPI_GELU epilogue saved; no f32 dx is written (replaces svae_layernorm_bwd + svae_gelu_bwd). part as above. */
int svae_layernorm_bwd_gelu(const void* dy, const void* x, int32_t x_dtype, const float* w, const float* mean,
                            const float* rstd, const void* gp, void* out_bf, float* part, int32_t nblk, int32_t rows,
                            int32_t D, svae_stream_t stream);
/* svae_layernorm_fwd (f32 x, D % 8 == 0, 16-B aligned x / zrows) with the z splice of transformer_vae.py:89-90: rows
 * r % zmod == 0 are taken from zrows[r / zmod] (f32 [rows / zmod][D]) and also written into x (the residual stream). */
int svae_layernorm_fwd_z(float* x, const float* zrows, int32_t zmod, const float* w, const float* b, void* y,
                         float* mean, float* rstd, int32_t rows, int32_t D, svae_stream_t stream);
int svae_layernorm_nblk(int32_t rows);
/* n <= SVAE_LN_MULTI_MAX LayerNorms of ONE input with their own affines: the encoder middle layers'
 * context_layer_norm(context) over the same x_emb (transformer_layer.py:52, one per middle layer, perceiver.py:43-46).
 * svae_layernorm_fwd_multi: one pass over f32 x writes y[j] = bf16(LN(x) * w[j] + b[j]) (bit-identical to n
 * svae_layernorm_fwd calls) and the shared mean / rstd. svae_layernorm_bwd_multi: the n backwards in one pass,
 * dx = dres + sum_j LN'_j(dy[j]) (dres may alias dx), the affine-gradient partials of LayerNorm j into part[j]
 * ([nblk][2][D] each, as svae_layernorm_bwd's part). f32 x, D % 4 == 0, D <= 1024. */
#define SVAE_LN_MULTI_MAX 4
int svae_layernorm_fwd_multi(const float* x, const float* const* w, const float* const* b, void* const* y, int32_t n,
                             float* mean, float* rstd, int32_t rows, int32_t D, svae_stream_t stream);
int svae_layernorm_bwd_multi(const void* const* dy, const float* x, const float* const* w, const float* mean,
                             const float* rstd, const float* dres, float* dx, float* const* part, int32_t nblk,
                             int32_t n, int32_t rows, int32_t D, svae_stream_t stream);

/* ---- column sums: out[j] (+)= sum_i in[i*ld + j] (bias grads, LN affine grads, batch sums) ----------
 * in_dtype 0 = f32, 1 = bf16. accumulate: 0 = overwrite, 1 = add into out. */
int svae_colsum(const void* in, int32_t in_dtype, int32_t rows, int32_t cols, int64_t ld, float* out,
                int32_t accumulate, svae_stream_t stream);

/* Up to SVAE_COLSUM_MAX f32 column sums in one launch, each added into its own out (the LayerNorm-affine gradients
 * of one layer's LayerNorm backwards). in / out 16-B aligned, cols and ld multiples of 4. */
#define SVAE_COLSUM_MAX 8
typedef struct svae_colsum_seg {
  const float* in;
  float* out;
  int64_t ld;
  int32_t rows, cols;
} svae_colsum_seg;
int svae_colsum_multi(const svae_colsum_seg* segs, int32_t n, svae_stream_t stream);

/* ---- Flash attention (dense path of Attention.forward, attention.py:51-105) ------------------------
 * q/k/v/o: bf16 rows of H*hd (token-major, head-interleaved, exactly the nn.Linear output layout),
 * row strides sq/sk/sv/so elements, batch strides bq/bk/bv/bo elements (bq = 0 for learned queries).
 * key_pad: uint8 [B][Lk] (1 = masked, padded_tensor.py:16) or NULL. causal: mask key > query
 * (attention.py:85-95). lse: f32 [B][H][Lq]. scale = hd^-0.5 (attention.py:83). hd: any multiple of 8 up to 128 (the
 * kernels are built for 64, 96 and 128 dims; another size runs the next one up with its loads and stores cut at hd).
 * A query with no visible key (every key of its batch entry padded) gets O = 0 and lse = -inf, and the backward
 * gives it and its entry's keys zero gradients. */
typedef struct svae_attn_desc {
  const void* q; const void* k; const void* v; void* o;
  int64_t sq, sk, sv, so, bq, bk, bv, bo;
  const uint8_t* key_pad;
  float* lse;
  int32_t B, H, Lq, Lk, hd, causal;
  float scale;
  /* backward only */
  const void* dout; int64_t sdo, bdo;
  float* delta;             /* [B][H][Lq] f32 workspace */
  float* dq;                /* f32 [B][Lq][H*hd] output (written), batch stride bdq; used when dq_bf is NULL */
  int64_t bdq;
  void* dk; void* dv;       /* bf16 outputs, row stride sdk/sdv, batch stride bdk/bdv */
  int64_t sdk, sdv, bdk, bdv;
  const float* rot_tab;     /* inverse rotary applied to dk when non-NULL ([Lk][d/2] (cos, sin)) */
  int32_t rot_d;
  /* optional f32 copy of O (forward writes it, backward's delta = rowsum(dO . O) reads it): keeps delta
     free of the bf16 rounding of O, which otherwise cancels badly when the keys are nearly alike */
  float* o32;
  int64_t so32, bo32;
  /* dQ is summed over key blocks without atomics: the backward writes one f32 partial per 128-key block
     into dq_part ([svae_attn_dq_part_elems] floats), then a second kernel sums them (times scale) into dq_bf
     (bf16, row stride ldq_bf, inverse rotary with rot_tab at pos = query row when rot_tab is set) or, when
     dq_bf is NULL, into dq (f32, no rotary). */
  float* dq_part;
  void* dq_bf;
  int64_t ldq_bf;
  /* > 0 (causal only): block-sparse sliding window of SparseAttention (sparse_attention.py:39-60 with
     block_size 32, include_cls): query q sees key k <= q iff k < 32 or k / 32 >= q / 32 - (window - 1).
     0 = dense. */
  int32_t window;
  /* backward: 1 = delta already holds rowsum(dO . O) (svae_gemm's delta epilogue on the dO GEMM): the delta pass is
     skipped */
  int32_t delta_ready;
  /* optional bf16 residual of O (the alternative to o32, 2 B per element instead of 4): the forward writes
     o_lo = bf16(O - bf16(O)) (row stride so_lo, batch stride bo_lo), the backward's delta pass reads dO . (o + o_lo):
     O to ~16 significant bits, where the f32-accumulated O itself carries ~19 */
  void* o_lo;
  int64_t so_lo, bo_lo;
  /* forward, few queries over many keys (<= 128 queries, non-causal, >= 2048 keys, < 128 query tiles in all): optional
     f32 workspace of svae_attn_fwd_ws_elems floats (16-B aligned); when given, the keys are cut into slices (one launch,
     the slice a grid dimension) whose partial O / lse are combined (split-KV), so a long key sequence fills the chip.
     NULL: one pass. */
  float* fwd_ws;
  int64_t fwd_ws_elems;
} svae_attn_desc;

int svae_attn_fwd(const svae_attn_desc* d, svae_stream_t stream);
/* floats of the split-KV forward's workspace for a shape (0: that shape runs in one pass) */
int64_t svae_attn_fwd_ws_elems(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t causal, int32_t window);
int svae_attn_bwd(const svae_attn_desc* d, svae_stream_t stream);
/* floats of the dq_part workspace: ceil(Lk / 128) * B * Lq * H * hd (+ the sliding window's [CLS] slabs) -- enough for
   every mode */
int64_t svae_attn_dq_part_elems(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd);
/* the same for a given sliding window (0 = dense): in window mode the 8-wave backward keeps dQ planes >= 1 to their
   band's rows, O(Lq) floats instead of O(Lq^2 / 512) (2 x 16384 tokens at hd 64: 36 MB instead of 8.6 GB) */
int64_t svae_attn_dq_part_elems_w(int32_t B, int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t window);
/* dq f32 [rows][H*hd] -> bf16 out (row stride ldo) with optional inverse rotary (pos = row % seq). */
int svae_dq_finalize(const float* dq, void* out, int64_t ldo, int32_t rows, int32_t D, const float* rot_tab,
                     int32_t seq, svae_stream_t stream);

/* ---- embedding (transformer_language_model.py:40-48): gather rows / scatter-add grads ------------- */
int svae_embedding_fwd(const int32_t* ids, const void* table_bf, float* out, void* out_bf, int32_t rows,
                       int32_t D, svae_stream_t stream);
/* the same gather into two f32 destinations (the encoder's input and the decoder's, whose position-0 rows the z
 * splice overwrites): replaces a device copy of the [rows, D] result */
int svae_embedding_fwd_dual(const int32_t* ids, const void* table, float* out, float* out2, int32_t rows, int32_t D,
                            svae_stream_t stream);
int svae_embedding_bwd(const int32_t* ids, const float* dout, float* dtable, int32_t rows, int32_t D,
                       svae_stream_t stream);

/* ---- reparameterise + KL (conditional_gaussian.py:18-28, continuous_autoencoder.py:42-52) -----------
 * stats: f32 [B][2*Z] (mu | logvar). eps: f32 [B][Z] or NULL (then drawn from (seed) in-kernel).
 * z out bf16 [B][Z] and f32 copy; raw_kl f32 [B]; kl_out f32[2] = {mean(raw_kl / ntok), mean(raw_kl)}.
 * Backward: dstats from dz (bf16 or f32) and the scalar kl gradient weight. */
int svae_reparam_kl_fwd(const float* stats, const float* eps, uint64_t seed, const int64_t* ntok,
                        float* z, void* z_bf, float* eps_out, float* raw_kl, float* kl_out, int32_t B,
                        int32_t Z, svae_stream_t stream);
int svae_reparam_kl_bwd(const float* stats, const float* eps, const float* dz, const int64_t* ntok,
                        const float* gkl, float* dstats, int32_t B, int32_t Z, svae_stream_t stream);

/* ---- cross entropy over materialised bf16 logits (robust_cross_entropy, language_model.py:161-170) --
 * part: f32 [rows][ntile][2] (max, sumexp) from SVAE_EPI_CE_STATS; label_logit f32 [rows].
 * Row r is position (r % seq) of its sequence (rows % seq == 0); label 0 = ignore_index. The sequence
 * positions are cut into nchunks chunks of chunk_len (torch.chunk along the sequence dim, :168; the last
 * chunk runs to the end of the sequence) and nll = mean over chunks of the per-chunk mean loss (a single
 * F.cross_entropy when nchunks == 1, :164-165). 1 <= nchunks <= 1024, (nchunks - 1) * chunk_len < seq.
 * finalize: lse[rows], row_loss[rows] (lse - label logit, 0 for ignored rows), chunk_w[nchunks]
 * (= 1 / (count_c * nchunks)), nll_out[1]; red_ws: f32 workspace of svae_ce_red_ws_elems(nchunks) floats
 * (per-block chunk partials, added in a fixed order: deterministic).
 * weighted_nll: the same chunked mean with F.cross_entropy's class weights (the val_bpb metric,
 * language_model.py:106-110): per chunk sum tok_w[y] * row_loss / sum tok_w[y]; tok_w f32 [V].
 * grad: in place, logits -> gscale[0] * chunk_w[c] * (softmax - onehot) in bf16 (0 for ignored rows);
 * dbias (optional, f32 [V]) += column sums of dlogits (output-bias gradient). */
int svae_ce_finalize(const float* part, int32_t ntile, const float* label_logit, const int32_t* labels,
                     int32_t rows, int32_t seq, int32_t nchunks, int32_t chunk_len, float* lse, float* row_loss,
                     float* chunk_w, float* nll_out, float* red_ws, svae_stream_t stream);
int svae_ce_weighted_nll(const float* row_loss, const int32_t* labels, const float* tok_w, int32_t rows,
                         int32_t seq, int32_t nchunks, int32_t chunk_len, float* out, float* red_ws,
                         svae_stream_t stream);
int32_t svae_ce_red_ws_elems(int32_t nchunks);
int svae_ce_grad(void* logits, int64_t ld, const float* lse, const float* chunk_w, const int32_t* labels,
                 const float* gscale, float* dbias, int32_t rows, int32_t V, int32_t seq, int32_t nchunks,
                 int32_t chunk_len, svae_stream_t stream);

/* ---- P-head cross entropy (training path of the tied vocabulary head + robust_cross_entropy) -----------
 * The head GEMM (SVAE_EPI_CE_PROB, row_a = c) stores P = exp(logit - c), c = the row's label logit, instead of
 * the logits; the backward then needs neither an exponential nor a dlogits pass:
 *   dlogits = r (x) P - q (x) onehot(label),  q = gscale * chunk_w[chunk] (0 for ignored rows),
 *   r = q * exp(c - lse);  dX = r . (P W) - q W[label] (SVAE_EPI_ROWSCALE_GATHER);
 *   dW = P^T (r . hh) (+ the one-hot part, svae_embedding_bwd_ce); d bias = sum_t r_t P[t] (k_weight row sums
 *   of the dW GEMM) - q scattered to the labels (bwd_prep).
 * ce_label_logit: out[r] = hh[r] . W[labels[r]] + bias[labels[r]] (f32 dot of bf16 rows; 0 where labels[r] = 0).
 * ce_prob_finalize: part f32 [ntile][rows] (the per-tile sums of P) -> lse = c + log sum, row_loss = lse - c,
 *   chunk_w, nll_out: the chunked mean of means of svae_ce_finalize.
 * ce_prob_bwd_prep: r_out, q_out [rows]; hh_out bf16 [rows][D] = r * hh; dbias[label] -= q (atomics; may be NULL).
 * The GEMM's exponent overflows to +inf for a logit more than 88 nats above the label logit; ce_prob_finalize_fix
 * finds every labelled row whose sum of P reaches 2^100 (or is not finite), lists it in sat_ws (int32 [1 + rows]:
 * count, then rows; the count stays readable after the call) and recomputes it exactly: the row's logits from hh, W
 * and bias, P[row] = exp(logit - max) (bf16, into P with leading dimension ldp), lse = max + log sum, row_loss =
 * lse - c, and row_off[row] = max -- so the backward (which reads P, row_off and lse) stays consistent. Every flagged
 * row is recomputed, however many there are (64 blocks stride over the list, ~0.3 ms per round at V = 32768, D = 512):
 * an overflowed P left in place would feed inf / NaN gradients to the clip and the optimiser, where the reference's
 * log-softmax stays finite.
 * ce_prob_finalize = ce_prob_finalize_fix without the check (sat_ws = NULL). */
int svae_ce_label_logit(const void* hh, int64_t ldh, const void* W, int64_t ldw, const float* bias,
                        const int32_t* labels, int32_t rows, int32_t D, float* out, svae_stream_t stream);
int svae_ce_prob_finalize(const float* part, int32_t ntile, const float* row_off, const int32_t* labels,
                          int32_t rows, int32_t seq, int32_t nchunks, int32_t chunk_len, float* lse, float* row_loss,
                          float* chunk_w, float* nll_out, float* red_ws, svae_stream_t stream);
int svae_ce_prob_finalize_fix(const float* part, int32_t ntile, float* row_off, const int32_t* labels, int32_t rows,
                              int32_t seq, int32_t nchunks, int32_t chunk_len, float* lse, float* row_loss,
                              float* chunk_w, float* nll_out, float* red_ws, const void* hh, int64_t ldh, const void* W,
                              int64_t ldw, const float* bias, void* P, int64_t ldp, int32_t V, int32_t D,
                              int32_t* sat_ws, svae_stream_t stream);
int svae_ce_prob_bwd_prep(const void* hh, int64_t ldh, const float* lse, const float* row_off, const float* chunk_w,
                          const int32_t* labels, const float* gscale, int32_t rows, int32_t seq, int32_t nchunks,
                          int32_t chunk_len, int32_t D, void* hh_out, float* r_out, float* q_out, float* dbias,
                          svae_stream_t stream);
/* Embedding backward fused with the one-hot part of the P-head's dW: dtable[ids[t]] += dout[t] - q[t-1] * hh[t-1]
 * (the second term where t % seq != 0; valid because labels[t-1] = ids[t] inside a sequence). */
int svae_embedding_bwd_ce(const int32_t* ids, const float* dout, float* dtable, int32_t rows, int32_t D, int32_t seq,
                          const void* hh, const float* q, svae_stream_t stream);

/* ---- elementwise helpers ------------------------------------------------------------------------ */
/* dropout backward + cast: out bf16 = keep(seed, idx) * g / (1-p) (p = 0: plain cast). */
int svae_dropout_bwd_cast(const float* g, void* out, float p, uint64_t seed, int64_t n, int32_t cols,
                          int64_t ld_in, svae_stream_t stream);
/* GELU backward (transformer_language_model.py:57 head GELU): out bf16 = dx * gp, gp = gelu' saved by the
   forward's SVAE_EPI_GELU epilogue. */
int svae_gelu_bwd(const float* dx, const void* gp, void* out, int64_t n, svae_stream_t stream);
/* The training step's token inputs (transformer_vae.py:42-55 / language_model.py's next-token targets), one pass:
 * ids32[t] = int32(ids[t]), labels[t] = ids[t + 1] inside a sequence of L and 0 at its last position, padm[t]
 * (uint8) = (ids[t] == 0) for pad_mode 1 or pad[t] (bool bytes) for pad_mode 2 (pad_mode 0: no mask), and
 * ntok_out[b] = ntok[b] for b < B when both are given. ids int64 [B][L] contiguous. */
int svae_prep_tokens(const int64_t* ids, const void* pad, int32_t pad_mode, int32_t B, int32_t L, int32_t* ids32,
                     int32_t* labels, void* padm, const int64_t* ntok, int64_t* ntok_out, svae_stream_t stream);
/* The step's scalars (transformer_vae.py:55 and its autograd backward): loss[0] = nll[0] + kl_weight * kl[0] when
 * loss != NULL; gs[0] = gloss[0], gs[1] = gloss[0] * kl_weight when gs != NULL (f32, each op rounded separately). */
int svae_step_scalars(const float* nll, const float* kl, const float* gloss, float kl_weight, float* loss, float* gs,
                      svae_stream_t stream);
/* cast f32 -> bf16 (n elements). */
int svae_cast_bf16(const float* in, void* out, int64_t n, svae_stream_t stream);
/* Transposed bf16 weight shadows (the K-contiguous B operand of the dX GEMMs): for each of nblocks
 * blocks, table[4b..4b+3] = (element offset, rows, cols, first tile) on the device, rows and cols % 8 == 0,
 * dst[offset + c * rows + r] = src[offset + r * cols + c]; one workgroup per 64 x 64 tile. */
int svae_transpose_blocks(const void* src, void* dst, const int64_t* table, int32_t nblocks, int32_t total_tiles,
                          svae_stream_t stream);
/* rows of x (f32 [rows][D], stride ld) whose (row % mod == 0) are copied to out [rows/mod][D] and zeroed
 * (the position-0 gradient of the z-projection splice, transformer_vae.py:89-90). */
int svae_extract_rows(float* x, int64_t ld, int32_t rows, int32_t mod, int32_t D, float* out,
                      svae_stream_t stream);
/* z_projections[i] backward (transformer_vae.py:89-90, x[:, 0] = nn.Linear(Z, d)(z)) from the position-0 gradient
 * g f32 [B][d]: dW f32 [d][Z] += g^T z, db f32 [d] += sum_b g[b], dz f32 [B][Z] += g W, with z bf16 [B][Z] and
 * W bf16 [d][Z] the forward's operands; f32 accumulation in a fixed order (deterministic), one launch (replaces the
 * dW GEMM with fused bias row sums and the split-K dz GEMM of a decoder layer). */
int svae_zproj_bwd(const float* g, const void* z, const void* W, float* dW, float* db, float* dz, int32_t B,
                   int32_t d, int32_t Z, svae_stream_t stream);
/* n (<= SVAE_ZPROJ_MAX) z-projection backwards sharing z and dz in one launch: for each segment, dW += g^T z and
 * db += sum_b g as svae_zproj_bwd; dz += g_0 W_0, then += g_1 W_1, ... in list order -- the same f32 results as n
 * svae_zproj_bwd calls in that order. */
#define SVAE_ZPROJ_MAX 32
typedef struct svae_zproj_seg {
  const float* g;   /* [B][d] f32 */
  const void* W;    /* [d][Z] bf16 */
  float* dW;        /* [d][Z] f32 */
  float* db;        /* [d] f32 */
} svae_zproj_seg;
int svae_zproj_bwd_multi(const svae_zproj_seg* segs, int32_t n, const void* z, float* dz, int32_t B, int32_t d,
                         int32_t Z, svae_stream_t stream);
/* The forward of n (<= SVAE_ZPROJ_MAX) z projections in one launch (transformer_vae.py:89, z_projections[i](z)):
 * out_i [B][d] f32 = z W_i^T + bias_i, z bf16 [B][Z] (Z <= 1024), W_i bf16 [d][Z]; f32 FMAs over k in order. */
typedef struct svae_zproj_fwd_seg {
  const void* W;       /* [d][Z] bf16 */
  const float* bias;   /* [d] f32 */
  float* out;          /* [B][d] f32 */
} svae_zproj_fwd_seg;
int svae_zproj_fwd_multi(const svae_zproj_fwd_seg* segs, int32_t n, const void* z, int32_t B, int32_t d, int32_t Z,
                         svae_stream_t stream);

/* ---- optimiser (RAdam, rectified_adam.py:16-88; clip_grad_norm_, language_model.py:120-122) -------
 * sumsq: partial sums of g^2 over n elements into part[nblk]; radam: reads part to form the global
 * norm, clips, updates m, v, p (f32) and the bf16 shadow pbf in one pass. scal: {lr_eff, bcm, bcv,
 * rho_ok, beta1, beta2, eps, wd_lr, max_norm}. norm_out[0] = total grad norm (pre-clip). */
int svae_sumsq(const float* g, int64_t n, float* part, int32_t nblk, svae_stream_t stream);
int svae_radam(float* p, void* pbf, const float* g, float* m, float* v, int64_t n, const float* part,
               int32_t nblk, const float* scal, float* norm_out, svae_stream_t stream);
/* In-place clip_grad_norm_ of a micro-step that no optimiser step follows (gradient accumulation): g *=
 * min(1, max_norm / (norm + 1e-6)) with norm from the sumsq partials; norm_out[0] = norm (may be NULL).
 * n % 4 == 0, g 16-byte aligned. */
int svae_clip_grad(float* g, int64_t n, const float* part, int32_t nblk, float max_norm, float* norm_out,
                   svae_stream_t stream);

/* ---- fp32 kernel mode (argmax-reconstruction parity; TransformerVAE.reconstruct in exact f32) ---------
 * svae_gemm_f32: C[M,N] = epi(A[M,K] . W[N,K]^T) on f32-input MFMA; epi in {SVAE_EPI_F32 (+bias, +resid),
 * SVAE_EPI_ROTARY_BF16 (rotary on cols < rot_cols, f32 out), SVAE_EPI_GELU (f32 out)}: these three and no other
 * (SVAE_EINVAL otherwise). bias and resid (added after the epilogue's function) are optional with each. Any M, N,
 * K >= 1 and any leading dimensions in elements; no alignment is required. The rotary epilogue needs rot_tab,
 * rot_d > 0, rot_seq > 0 and an even rot_cols (pairs of adjacent columns rotate together); row m takes table row
 * m % rot_seq.
 * svae_attn_fwd_f32: attention forward in f32 (same strides / masks / window as svae_attn_desc). Lk <= 32768 (a
 * query's scores for every key are held in LDS); window > 0 requires causal (the block-sparse band is causal).
 * SVAE_EINVAL otherwise. Any hd >= 1.
 * svae_layernorm_fwd_f32: LayerNorm with f32 output. */
int svae_gemm_f32(const float* A, const float* W, float* C, int32_t M, int32_t N, int32_t K, int64_t lda, int64_t ldw,
                  int64_t ldc, const float* bias, const float* resid, int64_t ldr, int32_t epi, const float* rot_tab,
                  int32_t rot_cols, int32_t rot_d, int32_t rot_seq, svae_stream_t stream);
int svae_attn_fwd_f32(const float* q, const float* k, const float* v, float* o, int64_t sq, int64_t sk, int64_t sv,
                      int64_t so, int64_t bq, int64_t bk, int64_t bv, int64_t bo, const uint8_t* key_pad, int32_t B,
                      int32_t H, int32_t Lq, int32_t Lk, int32_t hd, int32_t causal, int32_t window, float scale,
                      svae_stream_t stream);
int svae_layernorm_fwd_f32(const float* x, const float* w, const float* b, float* y, int32_t rows, int32_t D,
                           svae_stream_t stream);

/* ---- mutual-information log (transformer_vae.py:59-61, math_utils.py:51-58) ---------------------------
 * out[0] = kl[0] - marginal_kl(q), q = N(mu, exp(logvar)) from stats [B][2Z] (mu | logvar), with S posterior
 * samples per sequence: eps f32 [S][B][Z] or NULL (counter-based normals from seed). ws: f32 workspace of
 * >= 2 * S * B floats (on return ws[s*B + i] = the marginal log density of sample s of sequence i, ws[S*B + s*B + i]
 * = the sample's sum of squares). Z <= 4096 (SVAE_EINVAL beyond). Log-only diagnostic (not in the loss). */
int svae_mutual_info(const float* stats, const float* eps, uint64_t seed, const float* kl, int32_t B, int32_t Z,
                     int32_t S, float* ws, float* out, svae_stream_t stream);

/* ---- evaluation: log p(x|z) per sequence (continuous_autoencoder.py:82-88) ---------------------------
 * From the SVAE_EPI_CE_STATS partials of the head GEMM (which may run with C = NULL: no logits stored):
 * out[s] = sum over the rows r of sequence s (rows s*seq .. s*seq+seq-1) with labels[r] != 0 of
 * (label_logit[r] - logsumexp_r); labels 0 add 0 (the reference zeroes log_softmax column 0). part: f32
 * [rows][ntile][2] = (max, sum exp(x - max)) per 128-column tile, (-inf, 0) for a tile without a finite entry.
 * rows % seq == 0 (SVAE_EINVAL otherwise); out has rows / seq entries. */
int svae_ce_seq_logprob(const float* part, int32_t ntile, const float* label_logit, const int32_t* labels,
                        int32_t rows, int32_t seq, float* out, svae_stream_t stream);

/* ---- autoregressive decoding (TransformerVAE.sample, transformer_vae.py:95-128; the KV cache of
 * attention.py:107-168; GenerationState, generation.py). All f32. `cur` is a device int32 holding
 * GenerationState.current_index: kernels read it at run time, so a captured step graph replays for every
 * position. out_ids: int64 [B][T] (GenerationState.output_ids); live: uint8 [B].
 * dec_linear: Y[M,N] = epi(X[M,K] . W[N,K]^T + bias) + resid; epi SVAE_EPI_F32 / SVAE_EPI_GELU /
 *   SVAE_EPI_ROTARY_BF16 (rotary of rot_tab row cur-1 on columns < rot_cols, pairs within rot_d; f32 out).
 *   K % 4 == 0, X and W 16-byte aligned. part_ws (f32, part_elems floats, may be NULL): split-K partials for
 *   narrow N (the library picks the split count that fits; NULL = no split).
 * dec_attn: qkv f32 [B][ldq] = q | k | v (rotary applied); appends k, v at position cur-1 to the caches
 *   [B][H][T][hd] and writes O[b][h*hd ..] = softmax(q k^T * scale) v over the visible keys: 0..cur-1, or with
 *   window > 0 the sliding-window cache's set ([CLS] block, window-1 previous 32-blocks, current block).
 * dec_embed: x[b] = table[out_ids[b][cur-1]].
 * dec_penalty: repetition penalty on logits rows (row r is sequence row_map[r], or r): the ids
 *   out_ids[b][max(cur-512,0) .. cur-1] get logit * penalty if < 0 else logit / penalty (generation.py:35-41).
 * dec_sample: per live row: greedy (temperature <= 0 or top_k == 1) or temperature / top-k / nucleus top-p +
 *   multinomial from (seed, cur, b); writes out_ids[b][cur]; clears live[b] (and decrements *live_count)
 *   when the token is end_token or cur + 1 >= T (generation.py:43-77). V <= 32768.
 * dec_advance: *cur += 1. */
int svae_dec_linear(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y, int64_t ldy,
                    const float* resid, int64_t ldr, int32_t M, int32_t N, int32_t K, int32_t epi, const float* rot_tab,
                    int32_t rot_cols, int32_t rot_d, const int32_t* cur, float* part_ws, int64_t part_elems,
                    svae_stream_t stream);
int svae_dec_attn(const float* qkv, int64_t ldq, float* kcache, float* vcache, int32_t B, int32_t H, int32_t hd,
                  int32_t T, const int32_t* cur, int32_t window, float scale, float* O, int64_t ldo,
                  svae_stream_t stream);
int svae_dec_embed(const int64_t* out_ids, int32_t T, const int32_t* cur, const float* table, float* x, int32_t B,
                   int32_t D, svae_stream_t stream);
int svae_dec_penalty(float* logits, int64_t ldl, int32_t rows, const int32_t* row_map, const int64_t* out_ids,
                     int32_t T, const int32_t* cur, const uint8_t* live, float penalty, svae_stream_t stream);
int svae_dec_sample(const float* logits, int64_t ldl, int32_t V, int32_t rows, const int32_t* row_map,
                    int64_t* out_ids, int32_t T, const int32_t* cur, uint8_t* live, int32_t end_token,
                    float temperature, int32_t top_k, float top_p, uint64_t seed, int32_t* live_count,
                    svae_stream_t stream);
int svae_dec_advance(int32_t* cur, svae_stream_t stream);

/* ---- streaming bulk sampling: the decode kernels with one position per row ("slot"), StreamDecoder's step.
 * Same kernel bodies and arithmetic as the dec_* forms: with every pos[s] = c and key[s] = s the results equal
 * the dec_* forms' at cur = c bit for bit. pos: device int32 [S], the slot's current_index (>= 1); 0 = idle slot,
 * which every kernel skips without touching the slot's outputs; < 0 = finished, waiting for slot_refill. ids:
 * int64 [S][T], a slot's own output_ids row. T <= 32768.
 * slot_linear: dec_linear with the rotary epilogue at position pos[m]-1 of each row (same K-slicing, split rule,
 *   reduction order and finalize; the other epilogues take no position: use svae_dec_linear).
 * slot_attn: dec_attn with p = pos[s]-1 per slot: appends k, v at p, attends over the keys visible from p.
 * slot_embed: x[s] = table[ids[s][pos[s]-1]].
 * slot_splice: x[s] = zp[s] for the slots with pos[s] == 1 (the layer input of a sample's first step is
 *   z_projections[layer](z), transformer_vae.py:117-121); x f32 [S][D], zp f32 [S][ldz] (ldz >= D: one layer's
 *   columns of all layers' projections side by side), D % 4 == 0, ldz % 4 == 0, 16-byte aligned.
 * slot_penalty: dec_penalty over the slot's own ids[s][max(pos-512,0) .. pos-1].
 * slot_sample: dec_sample per slot; the multinomial draw is keyed by (seed, pos[s], key[s]) where key[s] is the
 *   number of the sample in the slot, so a sample's draws do not depend on the slot it ran in. Writes the token to
 *   ids[s][pos[s]] and as int16 to out[key[s]][pos[s]-1] (out: int16 [num_samples][T-1], zeroed by the caller),
 *   then pos[s] += 1, or pos[s] = -1 when the sample ended: the token is end_token, or position T-2 was written
 *   (KVDecoder.run's bound: the last column of a full-length row stays 0). V <= 32768.
 * slot_refill: one workgroup, no atomics. Every finished slot (pos < 0), in slot order, counts into *completed if
 *   it held a sample (key >= 0) and takes the next sample number j = (*next)++: if j < num_samples then key[s] = j,
 *   pos[s] = 1, ids[s][0] = start_token, z_slot[s] = z_all[j] (f32 rows of Z); else pos[s] = 0. *next never passes
 *   num_samples. The initial fill is this call on pos = -1, key = -1, *next = 0. */
int svae_slot_linear(const float* X, int64_t ldx, const float* W, int64_t ldw, const float* bias, float* Y, int64_t ldy,
                     const float* resid, int64_t ldr, int32_t S, int32_t N, int32_t K, const float* rot_tab,
                     int32_t rot_cols, int32_t rot_d, const int32_t* pos, float* part_ws, int64_t part_elems,
                     svae_stream_t stream);
int svae_slot_attn(const float* qkv, int64_t ldq, float* kcache, float* vcache, int32_t S, int32_t H, int32_t hd,
                   int32_t T, const int32_t* pos, int32_t window, float scale, float* O, int64_t ldo,
                   svae_stream_t stream);
int svae_slot_embed(const int64_t* ids, int32_t T, const int32_t* pos, const float* table, float* x, int32_t S,
                    int32_t D, svae_stream_t stream);
int svae_slot_splice(float* x, const float* zp, int64_t ldz, const int32_t* pos, int32_t S, int32_t D,
                     svae_stream_t stream);
int svae_slot_penalty(float* logits, int64_t ldl, int32_t S, const int64_t* ids, int32_t T, const int32_t* pos,
                      float penalty, svae_stream_t stream);
int svae_slot_sample(const float* logits, int64_t ldl, int32_t V, int32_t S, int64_t* ids, int32_t T, int32_t* pos,
                     const int32_t* key, int16_t* out, int32_t num_samples, int32_t end_token, float temperature,
                     int32_t top_k, float top_p, uint64_t seed, svae_stream_t stream);
int svae_slot_refill(int32_t* pos, int32_t* key, int64_t* ids, int32_t T, int32_t S, int32_t start_token,
                     const float* z_all, float* z_slot, int32_t Z, int32_t num_samples, int32_t* next,
                     int32_t* completed, svae_stream_t stream);

/* ---- beam search decoding. R = B * W decoder rows, row r = b * W + w is hypothesis w of document b;
 * 1 <= W <= 16 (SVAE_BEAM_MAX_W), 3 <= T <= 32768, R <= 65535. `cur` is the device int32 of the dec_* kernels: the
 * index c of the token this step generates (1 .. T-2). All pointers are static over a decode, so one captured step
 * graph replays. Per row: cum f32 [R] (cumulative log-probability, -inf = dead row), ids int64 [R][T] (ids[r][0] =
 * start token), anc uint8 [R][T]: anc[r][j] = the beam of the same document whose cache row holds this hypothesis's
 * key at position j. Per document: a pool of up to W finished hypotheses, pool_score / pool_logp f32 [B][W],
 * pool_len int32 [B][W], pool_ids int64 [B][W][T], pool_n int32 [B]; done uint8 [B]. len_pen f32 [T]: len_pen[l] =
 * l^alpha, computed by the caller (entry 0 unused); alpha_pos = (alpha > 0).
 * beam_attn: svae_dec_attn over rows r with p = cur-1: appends k, v at p to row r's own cache row and reads the
 *   visible key j < p from cache row (r / W) * W + anc[r][j]. Same visible set, body and summation order as
 *   dec_attn: with anc[r][j] = r % W the outputs are equal bit for bit.
 * beam_topk: per row with cum[r] > -inf whose document is not done (done may be NULL): lse = max + logf(sum
 *   expf(x - max)), the C = 2W largest logits by (value descending, id ascending), cand_score[r][k] = cum[r] +
 *   ((x - max) - logf(sum)), cand_tok[r][k] = id. Other rows' outputs are not written. 2W <= V <= 32768; R need not
 *   be a multiple of W here (done then has ceil(R / W) entries).
 * beam_select: per document not done, at c = *cur in 1 .. T-2 (nothing is written otherwise): the W * C candidates of
 *   its live rows ordered by (score descending, beam ascending, then the row's own candidate order, which beam_topk
 *   emits by logit descending, token ascending: for equal scores of one beam that is token ascending, and it stays
 *   the order of the exact sums where cum + logp rounds two candidates together), the best C walked in that order:
 *   an end_token candidate of rank < W enters the pool with score s / len_pen[c], length c (a free slot, else it
 *   replaces the worst entry -- lowest score, the later slot among equals -- if strictly better); one of rank >= W is
 *   dropped; any other becomes the next live hypothesis, in order, until W are live. Writes cum (-inf for rows left
 *   without a hypothesis), for each new row ids = parent's ids[0..c-1] + token and anc = parent's anc[0..c-2] +
 *   parent at c-1, the pool rows that arrived (prefix, end token, zeros), done[b] = pool full and
 *   best live cum / len_pen[alpha_pos ? T-2 : c] <= worst pool score, stamp[b] = c, and, when the three history
 *   pointers are given (int32, int32, f32 [T][R]), parent / token / score of each new row at [c][r] (-1, -1, -inf
 *   for a row left dead). The new id and ancestry rows are written to ids_next / anc_next (a row's parent may be
 *   another row of the document) and copied back by a second launch, which also writes *not_done = the number of
 *   documents with done == 0. No atomics.
 * beam_finalize: per document: if not done, its live rows (cum > -inf, in beam order) enter the pool as unfinished
 *   with score cum / len_pen[T-2] and length T-2 under the same rule; the pool is sorted by score descending
 *   (stable in slot order) and the best n <= W written: out_ids int64 [B][n][T-1] (start token excluded, zero from
 *   the entry's length on), out_scores, out_logp f32 [B][n], out_len int32 [B][n]. Missing entries: -inf, 0. The
 *   pool and the rows themselves are not modified. */
#define SVAE_BEAM_MAX_W 16
int svae_beam_attn(const float* qkv, int64_t ldq, float* kcache, float* vcache, const uint8_t* anc, int32_t R,
                   int32_t W, int32_t H, int32_t hd, int32_t T, const int32_t* cur, int32_t window, float scale,
                   float* O, int64_t ldo, svae_stream_t stream);
int svae_beam_topk(const float* logits, int64_t ldl, int32_t V, int32_t R, int32_t W, const float* cum,
                   const uint8_t* done, float* cand_score, int32_t* cand_tok, svae_stream_t stream);
int svae_beam_select(const float* cand_score, const int32_t* cand_tok, float* cum, int64_t* ids, uint8_t* anc,
                     int64_t* ids_next, uint8_t* anc_next, int32_t B, int32_t W, int32_t T, const int32_t* cur,
                     int32_t end_token, const float* len_pen, int32_t alpha_pos, float* pool_score, float* pool_logp,
                     int32_t* pool_len, int64_t* pool_ids, int32_t* pool_n, uint8_t* done, int32_t* not_done,
                     int32_t* stamp, int32_t* hist_parent, int32_t* hist_token, float* hist_score,
                     svae_stream_t stream);
int svae_beam_finalize(const float* cum, const int64_t* ids, int32_t B, int32_t W, int32_t T, const float* len_pen,
                       const float* pool_score, const float* pool_logp, const int32_t* pool_len,
                       const int64_t* pool_ids, const int32_t* pool_n, const uint8_t* done, int32_t n,
                       int64_t* out_ids, float* out_scores, float* out_logp, int32_t* out_len, svae_stream_t stream);

/* ---- latent index: posterior gathering and k-NN search (gather_latents.py:26-31, knn.py:28-50,
 * math_utils.py:90-101) -------------------------------------------------------------------------------
 * A corpus is N posteriors q(z|x) = N(mu, scale^2), f32 [N][Z]; Z % 4 == 0, 4 <= Z <= 256, N >= 1 (int32); mu,
 * scale and inv_var 16-byte aligned. Scores of query q against row i, summed over j:
 *   L2      sum (mu_q - mu_i)^2                                              smallest first
 *   COSINE  (mu_q . mu_i) * inv_norm_q * inv_norm_i                          largest first
 *   KL      KL(N_q || N_i) = (logdet_i - logdet_q)
 *           + 1/2 sum (scale_q^2 + (mu_q - mu_i)^2) * inv_var_i - Z / 2      smallest first
 * latent_prepare: the per-row quantities, once: inv_var [N][Z] = 1 / scale^2, logdet [N] = sum log scale,
 *   inv_norm [N] = 1 / max(|mu|_2, 1e-8) (precise logf, division, sqrtf). Queries are prepared the same way.
 * latent_scores: out f32 [Q][N]. A metric reads only its own operands (L2: the two mu; COSINE: + the inv_norms; KL:
 *   q_scale, q_logdet, inv_var, logdet); the others may be NULL.
 * latent_topk: the best k rows per query (1 <= k <= 64, k <= N), best first: scores f32 [Q][k], indices int32
 *   [Q][k]. A score is bit-identical to latent_scores' for the same pair; ties go to the lower row index; a NaN
 *   score ranks after every number. Two launches: a persistent grid (<= SVAE_LATENT_MAX_BLOCKS workgroups, each
 *   over a contiguous run of rows, queries in tiles of 8 per corpus pass) leaves its best k candidates per query in
 *   ws, then one workgroup per query merges them. ws: caller-owned, 8-byte aligned, >=
 *   svae_latent_topk_ws_bytes(Q, k) = Q * SVAE_LATENT_MAX_BLOCKS * k * 8 bytes; its contents need not survive. */
enum svae_latent_metric { SVAE_LATENT_L2 = 0, SVAE_LATENT_COSINE = 1, SVAE_LATENT_KL = 2 };
#define SVAE_LATENT_MAX_BLOCKS 1024
int svae_latent_prepare(const float* mu, const float* scale, float* inv_var, float* logdet, float* inv_norm, int32_t N,
                        int32_t Z, svae_stream_t stream);
int svae_latent_scores(int32_t metric, const float* q_mu, const float* q_scale, const float* q_logdet,
                       const float* q_inv_norm, int32_t Q, const float* mu, const float* inv_var, const float* logdet,
                       const float* inv_norm, int32_t N, int32_t Z, float* out, svae_stream_t stream);
int64_t svae_latent_topk_ws_bytes(int32_t Q, int32_t k);
int svae_latent_topk(int32_t metric, const float* q_mu, const float* q_scale, const float* q_logdet,
                     const float* q_inv_norm, int32_t Q, const float* mu, const float* inv_var, const float* logdet,
                     const float* inv_norm, int32_t N, int32_t Z, int32_t k, void* ws, int64_t ws_bytes, float* scores,
                     int32_t* indices, svae_stream_t stream);

/* ---- t-SNE of the latent index: exact, two output dimensions (tsne.py:16-30, where the embedding is tsnecuda's or
 * sklearn's) --------------------------------------------------------------------------------------------
 * The k-NN graph is dist f32 [N][k], nbr int32 [N][k] (LatentIndex.knn_graph); 1 <= k <= 64, N * k < 2^31. y, rep,
 * attr, vel, gains are f32 [N][2], 8-byte aligned; N >= 2 (tsne_affinities, a per-row operation, takes N >= 1);
 * tsne_repulse, its two companions (which return 0) and tsne_update also reject N > 2^24.
 * Nothing below uses an atomic: every sum has a fixed order and two calls on one input agree bit for bit.
 * tsne_affinities: per row the conditional p_j = exp(-beta (d_j - d_min)) / sum, beta found by bisection (start 1,
 *   doubled / halved while one bracket is open, at most 100 steps) until the entropy is within 1e-5 of
 *   log(perplexity); 1 < perplexity < k. p f32 [N][k] (each row sums to 1), beta f32 [N]. Precise expf / logf; the
 *   exponent carries the rounding errors of d_j - d_min and of the product, so a p is accurate relative to itself.
 *   Rows of equal distances come out uniform; rows with more tied minima than the perplexity share 1 among the ties.
 * tsne_repulse: with q_ij = 1 / (1 + |y_i - y_j|^2): rep_i = sum_{j != i} q_ij^2 (y_i - y_j), zrow_i =
 *   sum_{j != i} q_ij, zsum = sum_i zrow_i. j = i is excluded by index (duplicate points are legal: q = 1, no
 *   force). Three launches: a (row block, column slice) grid of workgroups, each over SVAE_TSNE_ROWS_PER_BLOCK rows
 *   (two per lane) and the slice's columns in LDS tiles of SVAE_TSNE_TILE_COLS, leaves per-slice partials in ws; one
 *   thread per row adds the slices in order; one workgroup adds the rows' zrow (in f64). A slice is
 *   svae_tsne_repulse_slice_cols(N) columns (a multiple of the tile), chosen from N alone so that the grid reaches
 *   about 2048 workgroups where N allows. ws: caller-owned, 8-byte aligned, >= svae_tsne_repulse_ws_bytes(N) =
 *   slices * 3 * N * 4 (rounded up to 8) + ceil(N / 256) * 8 bytes; its contents need not survive.
 * tsne_attract: attr_i = sum over row i's own edges (j = nbr[i][s]) of p[i][s] q_ij (y_i - y_j) + sum over the edges
 *   that point at i (e = j * k + s with nbr[j][s] = i) of p[j][s] q_ij (y_i - y_j): the two directed halves of the
 *   symmetrised affinity (p_{j|i} + p_{i|j}) / 2N, whose 1 / 2N the update applies. rev_ptr int32 [N + 1] and rev_edge
 *   int32 [N * k] are the edge ids grouped by target (sparse_vae.tsne.reverse_edges). One wave per row; neighbour
 *   and edge ids are clamped into range before they index anything.
 * tsne_update: in place, per coordinate: g = 4 (exaggeration / (2 N) * attr - rep / zsum); gains += 0.2 where vel and g
 *   have strictly opposite signs, else gains *= 0.8, floor 0.01; vel = momentum * vel - learning_rate * gains * g;
 *   y += vel. zsum is read from the device. */
#define SVAE_TSNE_ROWS_PER_BLOCK 512
#define SVAE_TSNE_TILE_COLS 256
int svae_tsne_affinities(const float* dist, int32_t N, int32_t k, float perplexity, float* p, float* beta,
                         svae_stream_t stream);
int64_t svae_tsne_repulse_slice_cols(int32_t N);
int64_t svae_tsne_repulse_ws_bytes(int32_t N);
int svae_tsne_repulse(const float* y, int32_t N, void* ws, int64_t ws_bytes, float* rep, float* zrow, float* zsum,
                      svae_stream_t stream);
int svae_tsne_attract(const float* y, const int32_t* nbr, const float* p, const int32_t* rev_ptr,
                      const int32_t* rev_edge, int32_t N, int32_t k, float* attr, svae_stream_t stream);
int svae_tsne_update(float* y, float* vel, float* gains, const float* attr, const float* rep, const float* zsum,
                     int32_t N, float exaggeration, float learning_rate, float momentum, svae_stream_t stream);

/* ---- aggregate-posterior diagnostics: the sums behind the MMD estimators of math_utils.py:104-184, and the
 * per-dimension statistics of the latent index (csrc/mmd.hip) ---------------------------------------------------
 * Rows are f32 [rows][Z], 16-byte aligned, Z a multiple of 4 in 4..256; 1 <= rows <= 2^24. Every f64 result leaves
 * through a device pointer. Nothing below uses an atomic: grids and summation orders depend on the shapes alone, so
 * two calls on one input agree bit for bit. ws: caller-owned, 8-byte aligned, contents need not survive.
 * svae_pairsum: out[p] (f64 [P] on the device, 1 <= P <= 8) = sum over the pairs of k_p(d2(x_i, y_j) + c_j), with
 *   d2 the squared distance formed from direct differences (fmaf of (x - y)^2, so its error is relative to d2 itself
 *   whatever offset the rows share). triangular != 0: y is ignored (may be NULL or x), M must equal N, the pairs are
 *   i < j (what pdist enumerates), N >= 2, col_off must be NULL. triangular == 0: all N * M pairs of x [N][Z] with
 *   y [M][Z]; col_off f32 [M] or NULL (= 0) is added to d2 before the kernel function (the IMQ cross term of
 *   math_utils.py:181 is not a true distance). kind SVAE_PAIR_RBF: k_p = exp(-params[p] * d2), params[p] >= 0;
 *   SVAE_PAIR_IMQ: k_p = params[p] / (params[p] + d2), params[p] > 0. params is a HOST pointer to P floats, read
 *   during the call. A workgroup owns svae_pairsum_geometry's rows (a lane holds its rows in registers) against a
 *   slice of the columns in LDS tiles of SVAE_PAIRSUM_TILE_COLS; a term is added in f32 only within one tile (at most
 *   SVAE_PAIRSUM_TILE_COLS terms per accumulator), from there on in f64. ws >= svae_pairsum_ws_bytes(...) =
 *   row_blocks * slices * 8 * 8 bytes.
 * svae_pairsum_geometry: geom (HOST int32 [5]) = {rows per workgroup (512 for Z <= 64, else 256), row blocks, column
 *   slices, columns per slice (a multiple of the tile), tile columns}; returns 1 (nothing written) on a bad shape.
 * svae_mmd_rowterm: out (f64 [1]) = sum_i exp(-0.5 sum_j (x_ij - m_j)^2 w_j); m f32 [Z] or NULL (= 0), w f32 [Z].
 *   ws >= svae_mmd_rowterm_ws_bytes(N).
 * svae_latent_colstats: per latent dimension over the N rows of loc / scale, in f64: mean_loc, var_loc (unbiased;
 *   NaN at N = 1), mean_kl = mean of 0.5 (mu^2 + sigma^2 - 1 - log sigma^2); f64 [Z] each. The sums are taken of
 *   loc - loc[0] (exact in f64), so a common offset of the rows costs no accuracy. ws >=
 *   svae_latent_colstats_ws_bytes(N, Z).
 * svae_latent_draw: z = fmaf(scale, eps, loc), f32 [N][Z]; eps f32 [N][Z] or NULL: standard normals from the
 *   library's counter RNG keyed by (seed, row, column) (Box-Muller of counters 2 (row Z + col) and + 1). */
#define SVAE_PAIR_RBF 0
#define SVAE_PAIR_IMQ 1
#define SVAE_PAIRSUM_TILE_COLS 32
#define SVAE_PAIRSUM_MAX_P 8
#define SVAE_MMD_REDUCE_BLOCKS 256
int svae_pairsum_geometry(int32_t N, int32_t M, int32_t Z, int32_t triangular, int32_t* geom);
int64_t svae_pairsum_ws_bytes(int32_t N, int32_t M, int32_t Z, int32_t triangular);
int svae_pairsum(const float* x, int32_t N, const float* y, int32_t M, int32_t Z, int32_t triangular, int32_t kind,
                 const float* params, int32_t P, const float* col_off, void* ws, int64_t ws_bytes, double* out,
                 svae_stream_t stream);
int64_t svae_mmd_rowterm_ws_bytes(int32_t N);
int svae_mmd_rowterm(const float* x, const float* m, const float* w, int32_t N, int32_t Z, void* ws, int64_t ws_bytes,
                     double* out, svae_stream_t stream);
int64_t svae_latent_colstats_ws_bytes(int32_t N, int32_t Z);
int svae_latent_colstats(const float* loc, const float* scale, int32_t N, int32_t Z, void* ws, int64_t ws_bytes,
                         double* mean_loc, double* var_loc, double* mean_kl, svae_stream_t stream);
int svae_latent_draw(const float* loc, const float* scale, const float* eps, uint64_t seed, int32_t N, int32_t Z,
                     float* z, svae_stream_t stream);

/* ---- k-means of the latent index: k-means++ seeding and Lloyd's iteration over the posterior means (csrc/kmeans.hip;
 * what stands in for the LDA topic colouring of tsne.py:38-63) ------------------------------------------------------
 * x is f32 [N][Z], cent f32 [K][Z], both 16-byte aligned; Z a multiple of 4 in 4..256; 1 <= K <= SVAE_KMEANS_MAX_K,
 * K <= N <= 2^24. Every entry point returns 1 before any launch on a NULL operand, a shape out of range or a
 * workspace that is too small; the *_ws_bytes companions return 0 on a bad shape. ws: caller-owned, 8-byte aligned,
 * contents need not survive. Nothing below uses an atomic: grids and summation orders depend on (N, K, Z) alone, so
 * two calls on one input agree bit for bit.
 * The distance d2(x, c) = sum_z (x_z - c_z)^2 is formed from direct differences in f32: per float4 chunk d = x - c,
 *   then two fmaf chains (elements 0, 2 and elements 1, 3 of the chunks, in chunk order) and their sum. The order
 *   depends on Z alone, contraction is off, and assign and seed share the function: a (row, centroid) pair has one
 *   f32 distance, whichever kernel, lane or workgroup computes it. |error| <= (Z / 2 + 3) 2^-24 d2 to first order.
 * svae_kmeans_assign: label int32 [N], in/out: the previous labels on entry (any value outside 0..K-1 means none), the
 *   nearest centroid on return. Smallest distance wins, ties go to the lower centroid index, a NaN distance loses to
 *   every number; a row whose distances are all NaN gets label 0 and d2 NaN. d2 f32 [N] or NULL: the winning distance.
 *   changed int32 [1]: the number of rows whose label differs from its value on entry. inertia f64 [1]: sum of the
 *   winning distances, added in f64 in a fixed order. A workgroup owns svae_kmeans_geometry's rows per workgroup (a
 *   lane holds its rows in registers) and streams the centroids through LDS in tiles of SVAE_KMEANS_TILE_CENTROIDS;
 *   a lane carries its best (d2, index) across the tiles. ws >= svae_kmeans_assign_ws_bytes = row blocks * 16 bytes.
 * svae_kmeans_update: count int32 [K] = the rows per label; cent in/out: cent[c] = (float)(S_c / count_c) with S_c
 *   the f64 sum of the rows labelled c and the division in f64; an empty cluster keeps the centroid it had on entry.
 *   Labels outside 0..K-1 are ignored (clamped before anything is indexed). S_c is a fixed tree: the rows are cut into
 *   B sort blocks of consecutive rows and the blocks into G groups of consecutive blocks (both from (N, K) alone:
 *   svae_kmeans_geometry); a group's rows of cluster c are added in ascending row order, the groups in ascending order.
 *   The route is a stable counting sort of the row numbers by label (per-block histograms, a scan over [block][K], a
 *   scatter by rank within the block), then one segment sum per (centroid, group). ws >= svae_kmeans_update_ws_bytes
 *   = G * K * Z * 8 (the group sums) + (B * K + K + 1 + N) * 4 (histograms, offsets, the sorted rows) rounded up to
 *   8; B <= SVAE_KMEANS_SORT_BLOCKS and G = min(B, max(1, 4096 / K)) regrouped evenly, so at N = 2^24, K = 1024,
 *   Z = 64 that is 2 MiB + 1 MiB + 64 MiB (the sorted row numbers).
 * svae_kmeans_seed: k-means++. u f32 [K] or NULL: the uniforms in [0, 1), injected or drawn from the library's counter
 *   RNG keyed by (seed, step). Step 0 takes row min(floor(u_0 N), N - 1). Step s >= 1 lowers every row's running
 *   minimum d2 against the centroid of step s - 1, takes the inclusive prefix sums of the minima in f64 in row order
 *   and chooses the first row i with cumsum_i > (double)u_s * total, so a row at distance 0 is never drawn; total == 0
 *   chooses row 0. The prefix is nested three deep, each level in ascending order: over the rows of a block of
 *   SVAE_KMEANS_SEED_BLOCK_ROWS, over the blocks of a run of 256 blocks, over the runs (cumsum_i = P + (Q + w_i)); up
 *   to N = 256 that is the plain running sum. rows int32 [K]: the chosen rows; cent [K][Z]: their copies. The chosen
 *   row never travels to the host: the 2 K - 1 launches queue without synchronisation. Rows must be finite. ws >=
 *   svae_kmeans_seed_ws_bytes = ceil(N / 256) * 8 + N * 4 (rounded up to 8).
 * svae_kmeans_geometry: geom (HOST int32 [8]) = {assign rows per workgroup (512 for Z <= 64, else 256), assign row
 *   blocks, centroid tile, sort blocks B, rows per sort block, row groups G, seed block rows, seed blocks}. */
#define SVAE_KMEANS_MAX_K 1024
#define SVAE_KMEANS_TILE_CENTROIDS 32
#define SVAE_KMEANS_SORT_BLOCKS 256
#define SVAE_KMEANS_SEED_BLOCK_ROWS 256
int svae_kmeans_geometry(int32_t N, int32_t K, int32_t Z, int32_t* geom);
int64_t svae_kmeans_assign_ws_bytes(int32_t N, int32_t K, int32_t Z);
int svae_kmeans_assign(const float* x, int32_t N, const float* cent, int32_t K, int32_t Z, int32_t* label, float* d2,
                       int32_t* changed, double* inertia, void* ws, int64_t ws_bytes, svae_stream_t stream);
int64_t svae_kmeans_update_ws_bytes(int32_t N, int32_t K, int32_t Z);
int svae_kmeans_update(const float* x, int32_t N, const int32_t* label, int32_t K, int32_t Z, float* cent,
                       int32_t* count, void* ws, int64_t ws_bytes, svae_stream_t stream);
int64_t svae_kmeans_seed_ws_bytes(int32_t N, int32_t K, int32_t Z);
int svae_kmeans_seed(const float* x, int32_t N, int32_t K, int32_t Z, const float* u, uint64_t seed, int32_t* rows,
                     float* cent, void* ws, int64_t ws_bytes, svae_stream_t stream);

/* ---- a Gaussian-mixture prior of the latents: EM over the index, a density and a sampler (csrc/gmm.hip; it stands
 * where the reference has only torch.randn at transformer_vae.py:103) ---------------------------------------------------
 * The mixture has K diagonal components. A row is the Gaussian q_i = N(x_i, diag(s2_i)) (x the posterior mean, s2 the
 * posterior variance), or the point x_i when s2 is NULL. With
 *   a_ik = log pi_k - 1/2 sum_d [log(2 pi v_kd) + ((x_id - m_kd)^2 + s2_id) / v_kd]      (= E_{q_i} log pi_k N(z; m_k, v_k))
 * EM ascends L = (1 / N) sum_i logsumexp_k a_ik, a lower bound (Jensen) on the aggregate posterior's expected
 * log-density under the mixture; for points it is the log-likelihood and this is the textbook diagonal GMM.
 * x and s2 are f32 [N][Z], 16-byte aligned; Z a multiple of 4 in 4..256; 1 <= K <= SVAE_GMM_MAX_K; 1 <= N <= 2^24.
 * Every entry point returns 1 before any launch on a NULL required operand, a misaligned pointer, a shape out of
 * range or a workspace that is too small; the *_ws_bytes companions and svae_gmm_params_floats return 0 on a bad shape.
 * ws: caller-owned, 8-byte aligned, contents need not survive. Nothing below uses an atomic: grids and summation
 * orders depend on (N, K, Z) alone, so two calls on one input agree bit for bit. Rows and parameters must be finite.
 * params: one device block of SVAE_GMM_PARAM_FLOATS(K, Z) floats per model, 16-byte aligned, with KP = K rounded up to
 *   a multiple of 4: weight [KP] at 0, logc [KP] at KP, then mean, var, inv_var, sd, f32 [K][Z] each, at 2 KP + j K Z
 *   (SVAE_GMM_OFF_*). weight, mean and var are the model; inv_var = (float)(1 / (double)var), sd =
 *   (float)sqrt((double)var) and logc = log pi_k - 1/2 sum_d log(2 pi v_kd) (formed in f64 in ascending d, rounded
 *   once; -inf for pi_k = 0) are derived.
 * svae_gmm_prepare: the derived rows from (weight, mean, var), for a loaded or hand-made model. svae_gmm_mstep's last
 *   launch calls the same device function.
 * a_ik in f32 from direct differences: per float4 chunk of the row d = x - m, e = fmaf(d, d, s2) (s2 = 0 for points),
 *   two fmaf chains s = fmaf(e, inv_var, s) (elements 0, 2 and elements 1, 3 of the chunks, in chunk order), q their
 *   sum, a = fmaf(-0.5, q, logc); logc = -inf gives a = -inf whatever q is. The order depends on Z alone, contraction
 *   is off, and every kernel shares the function: a (row, component) pair has one f32 value.
 *   |error| <= ((Z / 2 + 5) q / 2 + |logc| + |a|) 2^-24 to first order, against f64 from the same (x, s2, weight,
 *   mean, var).
 * svae_gmm_estep: lse f32 [N] = logsumexp_k a_ik, carried online over the components in index order ((M, S) from
 *   (-inf, 0); a = -inf is skipped, so a component of weight 0 contributes exactly 0; a > M: S = fmaf(S, expf(M - a),
 *   1), M = a; else S += expf(a - M); lse = M + logf(S)); a NaN a_ik makes lse_i NaN. label int32 [N] or NULL: the
 *   largest a_ik wins, ties go to the lower index, a NaN loses to every number, an all-NaN row gets 0. resp f32 [N][K]
 *   or NULL: expf(a_ik - lse_i). bound f64 [1] = sum_i lse_i, added in f64 in a fixed order. A workgroup owns
 *   SVAE_GMM_ROWS_PER_BLOCK rows (a lane holds its row, and its s2 row, in registers; with s2 and Z > 128 in four
 *   segments of 64 per tile) and streams (mean, inv_var, logc) through LDS in tiles of SVAE_GMM_TILE_COMPONENTS.
 *   ws >= svae_gmm_estep_ws_bytes = row blocks * 8 bytes.
 * svae_gmm_mstep: one EM M-step in place on params. Exactly one of lse (soft: r_ik = expf(a_ik - lse_i), a_ik from the
 *   function above) and label (hard: r_ik = 1 where label_i == k; labels outside 0..K-1 are ignored) is non-NULL. In
 *   f64 and relative to the mean on entry (d = x - m in f32, widened): N_k = sum r, S1 = sum r d, S2 = sum r (d^2 +
 *   s2). The rows are cut into G groups of consecutive rows (svae_gmm_geometry: from (N, K) alone); a group adds its
 *   rows in ascending order, then the groups are added in ascending order. m = m_old + S1 / N_k, v = S2 / N_k -
 *   (S1 / N_k)^2 + reg_covar, pi_k = N_k / (the sum of the positive N_k in index order), in f64, rounded once; then
 *   the derived rows. A component with N_k not > 0 keeps its mean and variance and gets weight 0. nk f64 [K]: N_k.
 *   reg_covar >= 0. ws >= svae_gmm_mstep_ws_bytes = (G + 1) * K * (2 Z + 1) * 8 bytes with G = ceil(N / rows per
 *   group), rows per group = ceil(N / max(1, 16384 / K)) rounded up to 64: at most 16384 + K statistics rows, 66 MiB
 *   at N = 2^24, K = 256, Z = 256.
 * svae_gmm_sample: comp int32 [n], z f32 [n][Z], 1 <= n <= 2^24. u f32 [n] or NULL: the uniforms in [0, 1), injected
 *   or drawn from the library's counter RNG keyed by (seed ^ 0x636F6D706F6E656E, row). Row j takes the first k with
 *   cum_k > (double)u_j * cum_{K-1}, cum the inclusive prefix sums of the weights in f64 in index order (a weight that
 *   is not > 0 adds nothing, so it is never drawn), clamped to the last component of positive weight. z_jd =
 *   fmaf(sd_kd, eps_jd, mean_kd); eps f32 [n][Z] or NULL: svae_latent_draw's normals (keyed by (seed, row, column)),
 *   so one standard-normal component reproduces svae_latent_draw(0, 1) bit for bit.
 * svae_gmm_geometry: geom (HOST int32 [6]) = {E-step rows per workgroup, row blocks, component tile, M-step row
 *   groups G, rows per group, E-step row segments (4 with s2 at Z > 128, else 1)}. */
#define SVAE_GMM_MAX_K 256
#define SVAE_GMM_TILE_COMPONENTS 16
#define SVAE_GMM_ROWS_PER_BLOCK 256
#define SVAE_GMM_KPAD(K) (((int64_t)(K) + 3) / 4 * 4)
#define SVAE_GMM_OFF_WEIGHT(K, Z) ((int64_t)0)
#define SVAE_GMM_OFF_LOGC(K, Z) SVAE_GMM_KPAD(K)
#define SVAE_GMM_OFF_MEAN(K, Z) (2 * SVAE_GMM_KPAD(K))
#define SVAE_GMM_OFF_VAR(K, Z) (2 * SVAE_GMM_KPAD(K) + (int64_t)(K) * (Z))
#define SVAE_GMM_OFF_INV_VAR(K, Z) (2 * SVAE_GMM_KPAD(K) + 2 * (int64_t)(K) * (Z))
#define SVAE_GMM_OFF_SD(K, Z) (2 * SVAE_GMM_KPAD(K) + 3 * (int64_t)(K) * (Z))
#define SVAE_GMM_PARAM_FLOATS(K, Z) (2 * SVAE_GMM_KPAD(K) + 4 * (int64_t)(K) * (Z))
int64_t svae_gmm_params_floats(int32_t K, int32_t Z);
int svae_gmm_geometry(int32_t N, int32_t K, int32_t Z, int32_t has_s2, int32_t* geom);
int svae_gmm_prepare(float* params, int32_t K, int32_t Z, svae_stream_t stream);
int64_t svae_gmm_estep_ws_bytes(int32_t N, int32_t K, int32_t Z);
int svae_gmm_estep(const float* x, const float* s2, int32_t N, const float* params, int32_t K, int32_t Z, float* lse,
                   int32_t* label, float* resp, double* bound, void* ws, int64_t ws_bytes, svae_stream_t stream);
int64_t svae_gmm_mstep_ws_bytes(int32_t N, int32_t K, int32_t Z);
int svae_gmm_mstep(const float* x, const float* s2, int32_t N, const float* lse, const int32_t* label, float* params,
                   int32_t K, int32_t Z, float reg_covar, double* nk, void* ws, int64_t ws_bytes, svae_stream_t stream);
int svae_gmm_sample(const float* params, int32_t K, int32_t Z, int32_t n, const float* u, const float* eps,
                    uint64_t seed, float* z, int32_t* comp, svae_stream_t stream);

/* ---- ELBO surgery of the latents: the density of the aggregate posterior q(z) = (1 / N) sum_j q(z | x_j) against all
 * N rows of the index, and the split of the mean KL built on it (csrc/aggpost.hip; the corpus-level form of marginal_kl,
 * math_utils.py:51-58, which estimates the split inside one batch and so cannot exceed log B) ------------------------------
 * Row j of the index is N(loc_j, diag(scale_j^2)). For a point z_i:
 *   l_ijd    = -1/2 ((z_id - loc_jd) / scale_jd)^2 - log scale_jd - 1/2 log 2 pi,      l_ij = sum_d l_ijd
 *   logq_i   = logsumexp_{j not skip_i} l_ij  - log n_i
 *   logq_dim = logsumexp_{j not skip_i} l_ijd - log n_i                                 (one per dimension d)
 * with n_i = N, or N - 1 where skip_i names a row (leave-one-out: the point's own component is left out).
 * z is f32 [M][Z], loc and scale f32 [N][Z], all 16-byte aligned; Z a multiple of 4 in 4..256; 1 <= M, N <= 2^24; with a
 * non-NULL skip N >= 2. Every entry point returns 1 before any launch on a NULL required operand, a misaligned pointer,
 * a shape out of range or a workspace that is too small; the *_ws_bytes companions return 0 on a bad shape. ws:
 * caller-owned, 16-byte aligned, contents need not survive. Nothing below uses an atomic: grids and orders depend on
 * (M, N, Z) alone, so two calls on one input agree bit for bit. Operands must be finite, scale > 0, and every
 * |(z - loc) / scale| below 2^63, so that every term is a finite f32.
 * svae_aggpost_logq: skip int32 [M] or NULL: the row each point leaves out; -1, or any value outside 0..N-1, leaves
 *   none out. logq f32 [M]; logq_dim f32 [M][Z] or NULL (then no per-dimension work is done: it is another kernel).
 *   A workgroup owns SVAE_AGGPOST_POINTS_PER_BLOCK points (one per lane, in registers) and one slice of consecutive
 *   rows; the rows are cut into slices (svae_aggpost_geometry: from (M, N) alone) so that a small M still fills the
 *   chip. It streams its slice through LDS in tiles of SVAE_AGGPOST_TILE_ROWS rows, staging per element loc, the
 *   multiplier w = 1.f / scale (one rounding) and logf(scale) (1 ulp), computed once per tile on load.
 *   Terms, in f32 from direct differences (no |z|^2 - 2 z.loc + |loc|^2 expansion), d = z - loc, t = d * w:
 *     joint    q from two fmaf chains acc = fmaf(t, t, acc) over elements 0, 2 and elements 1, 3 of the float4 chunks in
 *              chunk order, q their sum; c_j = (float)(-(sum_d (double)logf(scale_jd)) - Z / 2 log 2 pi), the sum in f64;
 *              l_ij = fmaf(-0.5, q, c_j).
 *              |error| <= ((Z / 2 + 7) q / 2 + 2 sum_d |log scale_jd| + |c_j| + |l_ij|) 2^-24 to first order.
 *     per dim  l_ijd = fmaf(-0.5f * t, t, nc), nc = -(logf(scale) + 0.9189385f) in f32.
 *              |error| <= (3 t^2 + 3 |log scale| + 1.84 + |l_ijd|) 2^-24 to first order.
 *   Accumulation, per output and slice: a running maximum Mx (f32, from the finite floor -1e38, so the loop forms
 *   neither NaN nor -inf) and a carried sum S (f64, from 0). Per tile s (f32) = 0 and M0 = Mx; per row in ascending
 *   order Mn = max(Mx, l), s = fmaf(s, ex(Mx - Mn), ex(l - Mn)), Mx = Mn, with ex(x) = v_exp_f32(x * 1.442695f) (one of
 *   the two arguments is 0 and ex(0) is exactly 1); a skipped row leaves Mx alone and adds 0. After the tile S = S + s
 *   where Mx == M0, else S = S * exp((double)M0 - (double)Mx) + s in f64. An f32 sum therefore spans at most
 *   SVAE_AGGPOST_TILE_ROWS terms and everything carried further is f64: relative to the true sum of the device's own
 *   terms, S is off by at most [sum_j r_j (3 |l_j - max| + 2) + T (3 + 3 max(1, ln T))] 2^-24 with r the terms' shares
 *   and T the tile rows, whatever N is. Each (point block, slice) workgroup leaves the partial (Mx, S) per point, and
 *   the per-dimension kernel (grid: point blocks x slices x dimension passes of SVAE_AGGPOST_PASS_DIMS dimensions, so a
 *   lane holds its point, the maxima and the f64 sums of one pass in registers whatever Z is) one per (point,
 *   dimension); a slice whose rows are all skipped leaves (-inf, 0). A second kernel merges the slices in ascending
 *   order in f64: Mt = max_s Mx_s, St = sum_s S_s exp(Mx_s - Mt) over the slices that are not (-inf, 0) (-inf - (-inf)
 *   is never formed), output (float)(Mt + log St - log n_i), rounded once.
 *   ws >= svae_aggpost_ws_bytes = slices * M * (per_dim ? 1 + Z : 1) * 16 bytes, slices = ceil(N / rows per slice),
 *   rows per slice = max(64, ceil(N / ceil(1024 / point blocks))) rounded up to the tile rows (one slice from 1024
 *   point blocks on): slices * M stays below 1024 * 256 + M + 256.
 * svae_aggpost_decompose: src int32 [M]: the row of (loc, scale) each point was drawn from (0 <= src_i < N is the
 *   caller's to guarantee: the entry point does not know N); logq, logq_dim as above, both required.
 *   out f64 [4 + Z] = {mi, marginal_kl, tc, kl_mc, dim_kl[Z]} with, for p = N(0, I),
 *     mi = mean_i(log q(z_i | x_src_i) - logq_i),       marginal_kl = mean_i(logq_i - log p(z_i)),
 *     tc = mean_i(logq_i - sum_d logq_dim_id),          dim_kl_d = mean_i(logq_dim_id - log p(z_id)),
 *   kl_mc = mi + marginal_kl; marginal_kl = tc + sum_d dim_kl_d to f64 rounding. Every term is formed in f64 from the
 *   f32 operands (sums over d in ascending d). The means are f64 sums in a fixed order, as svae_mmd_rowterm's: B =
 *   min(ceil(M / 256), 1024) workgroups; thread t of workgroup b adds its points b 256 + t + k B 256 in ascending k, a
 *   64-lane xor butterfly, the four waves in order; for dim_kl thread d adds the workgroup's points in ascending
 *   order; one workgroup then adds the B partials in ascending order and divides by M.
 *   ws >= svae_aggpost_decompose_ws_bytes = B * (3 + Z) * 8 bytes.
 * svae_aggpost_geometry: geom (HOST int32 [6]) = {points per workgroup, point blocks, row slices, rows per slice, tile
 *   rows, dimensions held per pass (per_dim: min(Z, SVAE_AGGPOST_PASS_DIMS); else Z, the joint kernel holds the whole
 *   point)}. */
#define SVAE_AGGPOST_POINTS_PER_BLOCK 256
#define SVAE_AGGPOST_TILE_ROWS 16
#define SVAE_AGGPOST_PASS_DIMS 16
int svae_aggpost_geometry(int32_t M, int32_t N, int32_t Z, int32_t per_dim, int32_t* geom);
int64_t svae_aggpost_ws_bytes(int32_t M, int32_t N, int32_t Z, int32_t per_dim);
int svae_aggpost_logq(const float* z, int32_t M, const float* loc, const float* scale, int32_t N, int32_t Z,
                      const int32_t* skip, float* logq, float* logq_dim, void* ws, int64_t ws_bytes,
                      svae_stream_t stream);
int64_t svae_aggpost_decompose_ws_bytes(int32_t M, int32_t Z);
int svae_aggpost_decompose(const float* z, const int32_t* src, const float* loc, const float* scale, const float* logq,
                           const float* logq_dim, int32_t M, int32_t Z, void* ws, int64_t ws_bytes, double* out,
                           svae_stream_t stream);

/* ---- reconstruction scoring over token ids: the integer counts behind BLEU, token accuracy and the edit rate of P
 * (candidate, reference) pairs (csrc/textscore.hip; what stands in for reconstruction_bleu of math_utils.py:9-38, whose
 * keys past its second order are not n-grams) --------------------------------------------------------------------------
 * cand is int16 [P][wc], ref int16 [P][wr], row-major with the width as leading dimension, 2-byte aligned; ids are
 * 0..32767 (taken modulo 2^15; the Python layer refuses others), and 0 is an ordinary token. cand_len, ref_len: int32
 * [P] on the device; row p is valid in [0, len_p) with len_p clamped into [0, width], and nothing at or beyond it is
 * read. 1 <= wc, wr <= SVAE_TEXT_MAX_LEN, P >= 1. Both entry points return 1 before any launch on a NULL operand,
 * P < 1 or a width out of range. No atomics, no workspace: a pair's result is a pure function of its two valid parts.
 * svae_ngram_overlap: out int32 [P][5] = {m1, m2, m3, m4, exact}. m_n = sum over the distinct n-grams g (n consecutive
 *   tokens) of min(count_cand(g), count_ref(g)), 0 when either side has fewer than n tokens; exact = the number of
 *   positions j < min(Lc, Lr) with cand[j] == ref[j]. One 256-thread workgroup per pair: position j gives the 64-bit
 *   key of (token + 1) at j..j+3 (first token in the top 16 bits, 0 past the end), both sides' keys are sorted once
 *   in LDS (bitonic over the next power of two of the longer side), order n is the keys' top n fields, and the first
 *   key of a run of equal prefixes on the candidate side looks its run up on the reference side by binary search.
 *   Static LDS at SVAE_TEXT_MAX_LEN = 2048: keys 2 * 2048 * 8 + tokens 2 * 2052 * 2 + partials 80 = 41,056 bytes; the
 *   next power of two would need 81,968, past the 64 KiB of a static declaration.
 * svae_edit_distance: out int32 [P] = the Levenshtein distance of the two valid parts with unit insert, delete and
 *   substitute costs; an empty side gives the other side's length. One wave per pair, four pairs per workgroup:
 *   lane l owns R >= ceil(Lc / 64) consecutive rows of the table (R the smallest of 1, 2, 3, 4, 6, 8, 12, 16, 24, 32
 *   that covers the pair), their previous column in registers, and runs one column behind lane l - 1 (one shuffle per
 *   step, no barrier); the reference row sits in LDS (4 * 2048 * 2 = 16 KiB). */
#define SVAE_TEXT_MAX_LEN 2048
int svae_ngram_overlap(const int16_t* cand, int32_t wc, const int16_t* ref, int32_t wr, const int32_t* cand_len,
                       const int32_t* ref_len, int32_t P, int32_t* out, svae_stream_t stream);
int svae_edit_distance(const int16_t* cand, int32_t wc, const int16_t* ref, int32_t wr, const int32_t* cand_len,
                       const int32_t* ref_len, int32_t P, int32_t* out, svae_stream_t stream);

/* library identification: returns a static string (build id, target arch). */
const char* svae_version(void);

#ifdef __cplusplus
}
#endif
#endif
