// Beam search decoding of p(x|z): R = B * W decoder rows, row r = b * W + w is hypothesis w of
// document b. The KV caches never move when the hypotheses are reordered: an ancestry table anc uint8 [R][T] says,
// for hypothesis r and key position j, which beam of the same document holds that key in its physical cache row.
//
//   svae_beam_attn:     svae_dec_attn (decode.hip) reading key j < p from cache row b * W + anc[r][j]; same body,
//                       same summation order, so the identity table gives dec_attn's output bit for bit.
//   svae_beam_topk:     one workgroup per row (dec_sample's layout: 1024 threads x 32 entries): row maximum,
//                       log-sum-exp with expf / logf, the C = 2W largest logits by (value descending, id ascending),
//                       cand_score = cum + logp.
//   svae_beam_select:   one workgroup per document: merges the W * C candidates by (score descending, beam
//                       ascending, then the row's own order: logit descending, token ascending), walks them
//                       (end tokens of rank < W into the pool, the others become the next live hypotheses), writes the next cum, id rows, ancestry rows, the pool, the
//                       done flag and the step history. The new rows go to a second buffer (a new row's parent may
//                       be another row of the document); a commit launch copies them back and counts the documents
//                       that are not done. No atomics: one workgroup owns a document.
//   svae_beam_finalize: live hypotheses of documents not done enter the pool as unfinished; each pool is sorted and
//                       the best n are written out.
#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int BEAM_MAX_W = 16;

template <int NW>
__device__ __forceinline__ float block_max(float v, float* sh) {
  v = wave_max(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float r = sh[0];
#pragma unroll
  for (int i = 1; i < NW; ++i) r = fmaxf(r, sh[i]);
  return r;
}
template <int NW>
__device__ __forceinline__ float block_sum(float v, float* sh) {
  v = wave_sum(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  __syncthreads();
  if (lane == 0) sh[w] = v;
  __syncthreads();
  float r = 0.f;
#pragma unroll
  for (int i = 0; i < NW; ++i) r += sh[i];
  return r;
}

// ------------------------------------------------------------------ attention through the ancestry table
// grid (H, R), 1024 threads; dec_attn_kernel's body with the cache row of key j < p taken from anc[r][j].
constexpr int BA_THREADS = 1024, BA_WAVES = BA_THREADS / 64;

__global__ __launch_bounds__(BA_THREADS) void beam_attn_kernel(const float* __restrict__ qkv, long long ldq,
                                                               float* __restrict__ kc, float* __restrict__ vc,
                                                               const unsigned char* __restrict__ anc, int W, int H,
                                                               int hd, int T, const int* __restrict__ cur, int window,
                                                               float scale, float* __restrict__ O, long long ldo) {
  extern __shared__ float sc[];
  __shared__ float qs[128], ks[128], vs[128], red[2 * BA_WAVES], osum[BA_THREADS];
  const int h = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  const int d = H * hd;
  const int p = *cur - 1;
  if (p < 0 || p >= T) return;                 // uniform over the workgroup, before any barrier
  const float* qrow = qkv + (long long)b * ldq + h * hd;
  const long long cbase = ((long long)b * H + h) * T * hd;
  const int doc0 = (b / W) * W;
  const unsigned char* arow = anc + (long long)b * T;
  const long long hstride = (long long)T * hd;
  if (tid < hd) {
    qs[tid] = qrow[tid];
    ks[tid] = qrow[d + tid];
    vs[tid] = qrow[2 * d + tid];
    kc[cbase + (long long)p * hd + tid] = ks[tid];
    vc[cbase + (long long)p * hd + tid] = vs[tid];
  }
  __syncthreads();
  // visible keys: [0, n1) then [lo2, p]
  int n1, lo2, n;
  if (window > 0) {
    n1 = min(p + 1, 32);
    lo2 = max(32, (p / 32 - (window - 1)) * 32);
    n = n1 + max(0, p + 1 - lo2);
  } else {
    n1 = p + 1;
    lo2 = 0;
    n = p + 1;
  }
  float mx = -INFINITY;
  for (int t = tid; t < n; t += BA_THREADS) {
    const int j = t < n1 ? t : lo2 + (t - n1);
    // key j < p lives in the cache row of beam anc[r][j] of this document
    const long long jbase = (j == p) ? cbase : ((long long)(doc0 + min((int)arow[j], W - 1)) * H + h) * hstride;
    const float* kr = (j == p) ? ks : kc + jbase + (long long)j * hd;
    float s = 0.f;
    for (int c = 0; c < hd; c += 4) {
      const f32x4 k4 = (j == p) ? *(const f32x4*)(ks + c) : *(const f32x4*)(kr + c);
      s += qs[c] * k4[0] + qs[c + 1] * k4[1] + qs[c + 2] * k4[2] + qs[c + 3] * k4[3];
    }
    s *= scale;
    sc[t] = s;
    mx = fmaxf(mx, s);
  }
  mx = block_max<BA_WAVES>(mx, red);
  float se = 0.f;
  for (int t = tid; t < n; t += BA_THREADS) {
    const float e = __expf(sc[t] - mx);
    sc[t] = e;
    se += e;
  }
  se = block_sum<BA_WAVES>(se, red + BA_WAVES);
  // O[c] = sum_t sc[t] v[key(t)][c]: thread = (column c, key group gi)
  const int G = BA_THREADS / hd, c = tid % hd, gi = tid / hd;
  float acc = 0.f;
  if (gi < G) {
    for (int t = gi; t < n; t += G) {
      const int j = t < n1 ? t : lo2 + (t - n1);
      const long long jbase = (j == p) ? cbase : ((long long)(doc0 + min((int)arow[j], W - 1)) * H + h) * hstride;
      const float v = (j == p) ? vs[c] : vc[jbase + (long long)j * hd + c];
      acc += sc[t] * v;
    }
  }
  osum[tid] = acc;
  __syncthreads();
  if (tid < hd) {
    float o = 0.f;
    for (int i = 0; i < G; ++i) o += osum[i * hd + tid];
    O[(long long)b * ldo + h * hd + tid] = o / se;
  }
}

// ------------------------------------------------------------------ per-row log-softmax and top 2W
constexpr int BT_T = 1024;          // threads per row
constexpr int BT_E = 32;            // elements per thread (V <= 32768)

__device__ __forceinline__ unsigned fkey(float x) {     // order-preserving float -> uint
  const unsigned u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float fkey_inv(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// Thread t holds vocabulary entries t + 1024 e. The selection key of entry i is (fkey(x) << 32) | ~i, so the largest
// key is the largest value and, among equal values, the lowest id. C rounds of a block-wide maximum; only the
// winner's thread rescans its 32 entries.
__global__ __launch_bounds__(BT_T) void beam_topk_kernel(const float* __restrict__ logits, long long ldl, int V, int W,
                                                         int C, const float* __restrict__ cum,
                                                         const unsigned char* __restrict__ done,
                                                         float* __restrict__ cand_score, int* __restrict__ cand_tok) {
  __shared__ float shf[BT_T / 64];
  __shared__ unsigned long long shk[BT_T / 64];
  const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const float cr = cum[r];
  if (!(cr > -INFINITY) || (done && done[r / W])) return;     // uniform over the workgroup
  const float* row = logits + (long long)r * ldl;
  float x[BT_E];
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    const int i = tid + BT_T * e;
    x[e] = i < V ? row[i] : -INFINITY;
  }
  float mx = -INFINITY;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) mx = fmaxf(mx, x[e]);
  mx = block_max<BT_T / 64>(mx, shf);
  float s = 0.f;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) s += expf(x[e] - mx);      // entries past V are -inf: exp gives 0
  s = block_sum<BT_T / 64>(s, shf);
  const float lse = logf(s);
  unsigned taken = 0;
  unsigned long long best = 0;
#pragma unroll
  for (int e = 0; e < BT_E; ++e) {
    const unsigned i = tid + BT_T * e;
    const unsigned long long k = (int)i < V ? ((unsigned long long)fkey(x[e]) << 32) | (0xFFFFFFFFu - i) : 0ull;
    best = k > best ? k : best;
  }
  for (int c = 0; c < C; ++c) {
    unsigned long long k = best;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const unsigned long long k2 = __shfl_xor(k, o, 64);
      k = k2 > k ? k2 : k;
    }
    __syncthreads();
    if (lane == 0) shk[w] = k;
    __syncthreads();
    unsigned long long top = shk[0];
#pragma unroll
    for (int i = 1; i < BT_T / 64; ++i) top = shk[i] > top ? shk[i] : top;
    const unsigned id = 0xFFFFFFFFu - (unsigned)(top & 0xFFFFFFFFull);
    if (tid == 0) {
      const bool ok = top != 0ull;
      const float xv = fkey_inv((unsigned)(top >> 32));
      cand_score[(long long)r * C + c] = ok ? cr + ((xv - mx) - lse) : -INFINITY;
      cand_tok[(long long)r * C + c] = ok ? (int)id : -1;
    }
    if (top != 0ull && (int)(id & (BT_T - 1)) == tid) {      // the owner drops the winner and rescans
      taken |= 1u << (id / BT_T);
      best = 0;
#pragma unroll
      for (int e = 0; e < BT_E; ++e) {
        const unsigned i = tid + BT_T * e;
        const unsigned long long k2 =
            ((int)i < V && !((taken >> e) & 1u)) ? ((unsigned long long)fkey(x[e]) << 32) | (0xFFFFFFFFu - i) : 0ull;
        best = k2 > best ? k2 : best;
      }
    }
  }
}

// ------------------------------------------------------------------ per-document selection
struct BS {
  const float* cand_score; const int* cand_tok;
  float* cum; long long* ids; unsigned char* anc; long long* ids_next; unsigned char* anc_next;
  int B, W, T;
  const int* cur; int end_token; const float* len_pen; int alpha_pos;
  float* pool_score; float* pool_logp; int* pool_len; long long* pool_ids; int* pool_n;
  unsigned char* done; int* not_done; int* stamp;
  int* hist_parent; int* hist_token; float* hist_score;
};

// The pool rule, shared by select and finalize: a free slot while there is one, else the worst entry (lowest score,
// the later slot among equals) if the arrival is strictly better. Returns the slot or -1.
__device__ __forceinline__ int pool_insert(float* ps, int& pn, int W, float score) {
  if (pn < W) return pn++;
  int worst = 0;
  for (int i = 1; i < W; ++i)
    if (ps[i] <= ps[worst]) worst = i;
  return score > ps[worst] ? worst : -1;
}

constexpr int BSEL_T = 512;         // >= W * C = 2 W^2 candidates per document

__global__ __launch_bounds__(BSEL_T) void beam_select_kernel(BS a) {
  __shared__ float s_sc[BSEL_T];
  __shared__ int s_tok[BSEL_T];
  __shared__ float o_sc[2 * BEAM_MAX_W];
  __shared__ int o_par[2 * BEAM_MAX_W], o_tok[2 * BEAM_MAX_W];
  __shared__ int l_par[BEAM_MAX_W], l_tok[BEAM_MAX_W], p_src[BEAM_MAX_W];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int W = a.W, C = 2 * W, N = W * C, T = a.T, R = a.B * W;
  if (a.done[b]) return;                       // uniform: a finished document is left as it is
  const int c = *a.cur;
  if (c < 1 || c > T - 2) return;
  // gather: candidates of dead rows (cum = -inf: their outputs were never written) and -inf scores do not count
  bool valid = false;
  float sc = -INFINITY;
  int tok = -1;
  if (tid < N) {
    const int w = tid / C, r = b * W + w;
    if (a.cum[r] > -INFINITY) {
      sc = a.cand_score[(long long)r * C + (tid - w * C)];
      tok = a.cand_tok[(long long)r * C + (tid - w * C)];
      valid = sc > -INFINITY && tok >= 0;
    }
  }
  s_sc[tid] = valid ? sc : -INFINITY;
  s_tok[tid] = valid ? tok : -1;
  const int nvalid = __syncthreads_count(valid);
  // rank by (score descending, beam ascending, the row's own candidate order): a strict total order. A row's
  // candidates arrive by (logit descending, token ascending), so within a beam this is the order of the exact sums
  // even where cum + logp rounds two of them to the same f32 (one beam without length penalty stays greedy).
  if (valid) {
    int rank = 0;
    for (int u = 0; u < N; ++u) {
      const float su = s_sc[u];
      const bool before = s_tok[u] >= 0 && (su > sc || (su == sc && u < tid));
      rank += before ? 1 : 0;
    }
    const int w = tid / C;
    if (rank < C) {
      o_sc[rank] = sc;
      o_par[rank] = w;
      o_tok[rank] = tok;
    }
  }
  __syncthreads();
  if (tid == 0) {
    const int ncand = min(nvalid, C);
    float ps[BEAM_MAX_W];
    int pn = a.pool_n[b];
    for (int i = 0; i < W; ++i) {
      ps[i] = i < pn ? a.pool_score[b * W + i] : -INFINITY;
      p_src[i] = -1;
    }
    int nl = 0;
    float cstar = -INFINITY;
    for (int i = 0; i < ncand && nl < W; ++i) {
      if (o_tok[i] == a.end_token) {
        if (i < W) {                           // an end token of rank >= W is dropped
          const float score = o_sc[i] / a.len_pen[c];
          const int slot = pool_insert(ps, pn, W, score);
          if (slot >= 0) {
            ps[slot] = score;
            p_src[slot] = o_par[i];
            a.pool_score[b * W + slot] = score;
            a.pool_logp[b * W + slot] = o_sc[i];
            a.pool_len[b * W + slot] = c;
          }
        }
      } else {
        if (nl == 0) cstar = o_sc[i];
        l_par[nl] = o_par[i];
        l_tok[nl] = o_tok[i];
        a.cum[b * W + nl] = o_sc[i];
        if (a.hist_parent) {
          const long long hi = (long long)c * R + b * W + nl;
          a.hist_parent[hi] = o_par[i];
          a.hist_token[hi] = o_tok[i];
          a.hist_score[hi] = o_sc[i];
        }
        ++nl;
      }
    }
    for (int j = nl; j < W; ++j) {             // fewer than W continuations: the rest of the rows go dead
      l_par[j] = j;
      l_tok[j] = 0;
      a.cum[b * W + j] = -INFINITY;
      if (a.hist_parent) {
        const long long hi = (long long)c * R + b * W + j;
        a.hist_parent[hi] = -1;
        a.hist_token[hi] = -1;
        a.hist_score[hi] = -INFINITY;
      }
    }
    a.pool_n[b] = pn;
    // done: the pool is full and the best live hypothesis can no longer beat its worst entry
    bool dn = false;
    if (pn == W) {
      float worst = ps[0];
      for (int i = 1; i < W; ++i) worst = fminf(worst, ps[i]);
      const int Lb = a.alpha_pos ? T - 2 : c;
      dn = cstar / a.len_pen[Lb] <= worst;
    }
    a.done[b] = dn ? 1 : 0;
    a.stamp[b] = c;
  }
  __syncthreads();
  // new rows into the second buffer: the parent's prefix, then the token; ancestry: the parent's prefix, then the
  // parent itself at position c - 1 (the key it appended this step)
  for (int i = tid; i < W * (c + 1); i += BSEL_T) {
    const int j = i / (c + 1), t = i - j * (c + 1);
    const long long src = (long long)(b * W + l_par[j]) * T, dst = (long long)(b * W + j) * T;
    a.ids_next[dst + t] = t < c ? a.ids[src + t] : (long long)l_tok[j];
    if (t < c) a.anc_next[dst + t] = t < c - 1 ? a.anc[src + t] : (unsigned char)l_par[j];
  }
  // pool rows that arrived this step: prefix, end token, zeros
  for (int sl = 0; sl < W; ++sl) {
    const int par = p_src[sl];
    if (par < 0) continue;
    const long long src = (long long)(b * W + par) * T, dst = (long long)(b * W + sl) * T;
    for (int t = tid; t < T; t += BSEL_T)
      a.pool_ids[dst + t] = t < c ? a.ids[src + t] : (t == c ? (long long)a.end_token : 0ll);
  }
}

// grid R + 1: block r copies row r's new prefix back if its document was selected this step; the last block counts
// the documents that are not done.
__global__ __launch_bounds__(256) void beam_commit_kernel(BS a) {
  const int W = a.W, T = a.T, R = a.B * W, tid = threadIdx.x;
  const int c = *a.cur;
  if ((int)blockIdx.x == R) {
    int total = 0;
    for (int b0 = 0; b0 < a.B; b0 += 256) {
      const int b = b0 + tid;
      total += __syncthreads_count(b < a.B && !a.done[b]);
    }
    if (tid == 0) *a.not_done = total;
    return;
  }
  const int r = blockIdx.x;
  if (c < 1 || c > T - 2 || a.stamp[r / W] != c) return;
  const long long base = (long long)r * T;
  for (int t = tid; t <= c; t += 256) {
    a.ids[base + t] = a.ids_next[base + t];
    if (t < c) a.anc[base + t] = a.anc_next[base + t];
  }
}

// ------------------------------------------------------------------ finalize
__global__ __launch_bounds__(256) void beam_finalize_kernel(const float* __restrict__ cum, const long long* __restrict__ ids,
                                                            int B, int W, int T, const float* __restrict__ len_pen,
                                                            const float* __restrict__ pool_score,
                                                            const float* __restrict__ pool_logp,
                                                            const int* __restrict__ pool_len,
                                                            const long long* __restrict__ pool_ids,
                                                            const int* __restrict__ pool_n,
                                                            const unsigned char* __restrict__ done, int n,
                                                            long long* __restrict__ out_ids, float* __restrict__ out_scores,
                                                            float* __restrict__ out_logp, int* __restrict__ out_len) {
  __shared__ float ps[BEAM_MAX_W], pl[BEAM_MAX_W];
  __shared__ int plen[BEAM_MAX_W], src[BEAM_MAX_W], order[BEAM_MAX_W];
  __shared__ int s_pn;
  const int b = blockIdx.x, tid = threadIdx.x;
  if (tid == 0) {
    int pn = min(max(pool_n[b], 0), W);
    for (int i = 0; i < pn; ++i) {
      ps[i] = pool_score[b * W + i];
      pl[i] = pool_logp[b * W + i];
      plen[i] = pool_len[b * W + i];
      src[i] = i;                              // < W: a pool row; W + w: live row w
    }
    if (!done[b]) {
      for (int w = 0; w < W; ++w) {
        const float cw = cum[b * W + w];
        if (!(cw > -INFINITY)) continue;
        const float score = cw / len_pen[T - 2];
        const int slot = pool_insert(ps, pn, W, score);
        if (slot >= 0) {
          ps[slot] = score;
          pl[slot] = cw;
          plen[slot] = T - 2;
          src[slot] = W + w;
        }
      }
    }
    // stable insertion sort by score descending
    for (int i = 0; i < pn; ++i) {
      int k = i;
      while (k > 0 && ps[order[k - 1]] < ps[i]) {
        order[k] = order[k - 1];
        --k;
      }
      order[k] = i;
    }
    s_pn = pn;
  }
  __syncthreads();
  const int pn = s_pn;
  for (int i = 0; i < n; ++i) {
    const bool have = i < pn;
    const int sl = have ? order[i] : 0;
    const int len = have ? min(plen[sl], T - 1) : 0;
    if (tid == 0) {
      out_scores[b * n + i] = have ? ps[sl] : -INFINITY;
      out_logp[b * n + i] = have ? pl[sl] : -INFINITY;
      out_len[b * n + i] = len;
    }
    const long long* row = nullptr;
    if (have) row = src[sl] < W ? pool_ids + (long long)(b * W + src[sl]) * T : ids + (long long)(b * W + src[sl] - W) * T;
    long long* orow = out_ids + (long long)(b * n + i) * (T - 1);
    for (int t = tid; t < T - 1; t += 256) orow[t] = (have && t < len) ? row[t + 1] : 0ll;
  }
}

}  // namespace

static bool beam_shape_ok(int32_t B, int32_t W, int32_t T) {
  return B > 0 && W >= 1 && W <= BEAM_MAX_W && T >= 3 && T <= 32768 && (long long)B * W <= 0x7fffffffll / 32768;
}

SVAE_EXPORT int svae_beam_attn(const float* qkv, int64_t ldq, float* kcache, float* vcache, const uint8_t* anc,
                               int32_t R, int32_t W, int32_t H, int32_t hd, int32_t T, const int32_t* cur,
                               int32_t window, float scale, float* O, int64_t ldo, svae_stream_t stream) {
  if (!qkv || !kcache || !vcache || !anc || !cur || !O || R <= 0 || H <= 0 || T <= 0) return SVAE_EINVAL;
  if (W < 1 || W > BEAM_MAX_W || R % W || R > 65535) return SVAE_EINVAL;
  if (hd <= 0 || hd > 128 || hd % 4 || window < 0 || T > 32768) return SVAE_EINVAL;
  if ((((uintptr_t)kcache | (uintptr_t)vcache) & 15) || ldq % 4) return SVAE_EINVAL;
  hipLaunchKernelGGL(beam_attn_kernel, dim3(H, R), dim3(BA_THREADS), (size_t)T * sizeof(float), (hipStream_t)stream, qkv,
                     ldq, kcache, vcache, (const unsigned char*)anc, W, H, hd, T, cur, window, scale, O, ldo);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_beam_topk(const float* logits, int64_t ldl, int32_t V, int32_t R, int32_t W, const float* cum,
                               const uint8_t* done, float* cand_score, int32_t* cand_tok, svae_stream_t stream) {
  if (!logits || !cum || !cand_score || !cand_tok || R <= 0) return SVAE_EINVAL;
  if (W < 1 || W > BEAM_MAX_W || V < 2 * W || V > BT_T * BT_E || ldl < V) return SVAE_EINVAL;
  hipLaunchKernelGGL(beam_topk_kernel, dim3(R), dim3(BT_T), 0, (hipStream_t)stream, logits, (long long)ldl, V, W, 2 * W,
                     cum, (const unsigned char*)done, cand_score, (int*)cand_tok);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_beam_select(const float* cand_score, const int32_t* cand_tok, float* cum, int64_t* ids,
                                 uint8_t* anc, int64_t* ids_next, uint8_t* anc_next, int32_t B, int32_t W, int32_t T,
                                 const int32_t* cur, int32_t end_token, const float* len_pen, int32_t alpha_pos,
                                 float* pool_score, float* pool_logp, int32_t* pool_len, int64_t* pool_ids,
                                 int32_t* pool_n, uint8_t* done, int32_t* not_done, int32_t* stamp,
                                 int32_t* hist_parent, int32_t* hist_token, float* hist_score, svae_stream_t stream) {
  if (!cand_score || !cand_tok || !cum || !ids || !anc || !ids_next || !anc_next || !cur || !len_pen) return SVAE_EINVAL;
  if (!pool_score || !pool_logp || !pool_len || !pool_ids || !pool_n || !done || !not_done || !stamp) return SVAE_EINVAL;
  if (!beam_shape_ok(B, W, T)) return SVAE_EINVAL;
  if ((hist_parent || hist_token || hist_score) && !(hist_parent && hist_token && hist_score)) return SVAE_EINVAL;
  BS a;
  a.cand_score = cand_score; a.cand_tok = (const int*)cand_tok;
  a.cum = cum; a.ids = (long long*)ids; a.anc = anc; a.ids_next = (long long*)ids_next; a.anc_next = anc_next;
  a.B = B; a.W = W; a.T = T;
  a.cur = cur; a.end_token = end_token; a.len_pen = len_pen; a.alpha_pos = alpha_pos;
  a.pool_score = pool_score; a.pool_logp = pool_logp; a.pool_len = (int*)pool_len; a.pool_ids = (long long*)pool_ids;
  a.pool_n = (int*)pool_n;
  a.done = done; a.not_done = (int*)not_done; a.stamp = (int*)stamp;
  a.hist_parent = (int*)hist_parent; a.hist_token = (int*)hist_token; a.hist_score = hist_score;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(beam_select_kernel, dim3(B), dim3(BSEL_T), 0, s, a);
  hipLaunchKernelGGL(beam_commit_kernel, dim3(B * W + 1), dim3(256), 0, s, a);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_beam_finalize(const float* cum, const int64_t* ids, int32_t B, int32_t W, int32_t T,
                                   const float* len_pen, const float* pool_score, const float* pool_logp,
                                   const int32_t* pool_len, const int64_t* pool_ids, const int32_t* pool_n,
                                   const uint8_t* done, int32_t n, int64_t* out_ids, float* out_scores, float* out_logp,
                                   int32_t* out_len, svae_stream_t stream) {
  if (!cum || !ids || !len_pen || !pool_score || !pool_logp || !pool_len || !pool_ids || !pool_n || !done) return SVAE_EINVAL;
  if (!out_ids || !out_scores || !out_logp || !out_len || !beam_shape_ok(B, W, T) || n < 1 || n > W) return SVAE_EINVAL;
  hipLaunchKernelGGL(beam_finalize_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, cum, (const long long*)ids, B, W, T,
                     len_pen, pool_score, pool_logp, (const int*)pool_len, (const long long*)pool_ids, (const int*)pool_n,
                     (const unsigned char*)done, n, (long long*)out_ids, out_scores, out_logp, (int*)out_len);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
