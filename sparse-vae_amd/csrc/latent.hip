// Latent index: the posterior latents after training (gather_latents.py:26-31, knn.py:28-50 and
// math_utils.py:90-101 in the reference, where they are torch expressions over [N, Z] temporaries + topk).
//
//   svae_latent_prepare: per corpus row, once: inv_var = 1 / scale^2, logdet = sum_j log scale_j,
//                        inv_norm = 1 / max(|mu|, 1e-8) (precise logf / division / sqrtf).
//   svae_latent_scores:  the dense [Q, N] score matrix of a metric (pairwise_gaussian_kl, the tests).
//   svae_latent_topk:    fused score + select, two launches. Phase 1: a persistent grid streams the corpus once per
//                        tile of QT queries; every workgroup owns a contiguous run of rows and leaves its best k
//                        (key, index) candidates per query in the workspace. Phase 2: one workgroup per query merges
//                        the blocks * k candidates. No atomics, no cross-workgroup synchronisation inside a launch.
//
// Access shape: a row of Z f32 is read by a group of 16 lanes, one float4 per lane and chunk (Z = 64: 256 B per
// group), so a wave-instruction covers four whole consecutive rows = 1 KiB contiguous. Lane `sub` of the group sums the
// chunks sub, sub + 16, ... in order (two packed-FMA chains, elements (0, 2) and (1, 3)), then the 16 partial sums are
// added by a DPP butterfly whose adds are commutative pairs: every lane ends with the same bits. The order depends on Z
// alone, never on the lane group, wave or workgroup that holds the row, and `scores` and `topk` share the one function
// (latent_score), so the score of a (query, row) pair is bit-identical in both and identical rows score identically.
//
// Selection order: a score becomes a 64-bit key (order-preserving u32 image of the float, negated for COSINE, in the
// high word; the row index in the low word), smaller key = better. Ties therefore go to the lower index whatever the
// grid, a NaN score maps to one key above +inf (it ranks after every number, before the sentinel), and the sentinel
// (all ones: worst score, index -1) pads workgroups that hold fewer than k rows. A wave keeps its running best 64 per
// query in registers, entry i in lane i, sorted: a candidate is inserted (ballot + popcount + lane shift) only when it
// beats the wave's current k-th best, which becomes rare after the first few thousand rows.
#include <atomic>

#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

typedef unsigned long long u64;

constexpr int QT = 8;                              // queries per corpus pass
constexpr int MAXB = SVAE_LATENT_MAX_BLOCKS;       // phase-1 grid cap (the workspace is sized for it)
constexpr int MIN_ROWS = 256;                      // fewest rows worth a workgroup of their own
constexpr u64 SENT = ~0ull;
constexpr unsigned NAN_KEY = 0xFFFFFFFEu;

__device__ __forceinline__ float dpp_f(float v, int ctrl_sel) {
  // ctrl_sel is folded at compile time (the builtin needs an immediate)
  const int x = __float_as_int(v);
  int r;
  switch (ctrl_sel) {
    case 0: r = __builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, true); break;    // quad_perm [1, 0, 3, 2]
    case 1: r = __builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, true); break;    // quad_perm [2, 3, 0, 1]
    case 2: r = __builtin_amdgcn_update_dpp(0, x, 0x141, 0xF, 0xF, true); break;   // row_half_mirror
    default: r = __builtin_amdgcn_update_dpp(0, x, 0x140, 0xF, 0xF, true); break;  // row_mirror
  }
  return __int_as_float(r);
}

// Sum over the 16 lanes of a row group; all 64 lanes must be active. After the two quad steps a quad's lanes hold
// one value, so the mirrors pair each lane with the other quad / the other half: every add is x + y in one lane and
// y + x in its partner, and all 16 lanes end bit-identical.
__device__ __forceinline__ float sum16(float v) {
  v += dpp_f(v, 0);
  v += dpp_f(v, 1);
  v += dpp_f(v, 2);
  v += dpp_f(v, 3);
  return v;
}

// The one score function. m / iv: this lane's chunks of the row's mu and inv_var (zeros where the lane has no chunk),
// qm / qv: the same chunks of the query's mu and variance. Explicit fmaf / single operations only: nothing is left for
// the compiler to contract differently at different call sites.
template <int METRIC, int ZC>
__device__ __forceinline__ float latent_score(const f32x4 (&m)[ZC], const f32x4 (&iv)[ZC], float ld_i, float in_i,
                                              const f32x4 (&qm)[ZC], const f32x4 (&qv)[ZC], float ld_q, float in_q,
                                              float half_z) {
#pragma clang fp contract(off)
  // two running sums per lane, over the chunk elements (0, 2) and (1, 3): the packed f32 FMAs (v_pk_fma_f32) take
  // the halves of a float4 as one operand, half the instructions of four scalar FMAs
  f32x2 acc2 = {0.f, 0.f};
#pragma unroll
  for (int c = 0; c < ZC; ++c) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const f32x2 mh = {m[c][2 * h], m[c][2 * h + 1]}, qh = {qm[c][2 * h], qm[c][2 * h + 1]};
      if constexpr (METRIC == SVAE_LATENT_COSINE) {
        acc2 = __builtin_elementwise_fma(qh, mh, acc2);
      } else {
        const f32x2 d = qh - mh;
        if constexpr (METRIC == SVAE_LATENT_L2) {
          acc2 = __builtin_elementwise_fma(d, d, acc2);
        } else {
          const f32x2 vh = {qv[c][2 * h], qv[c][2 * h + 1]}, ih = {iv[c][2 * h], iv[c][2 * h + 1]};
          acc2 = __builtin_elementwise_fma(__builtin_elementwise_fma(d, d, vh), ih, acc2);
        }
      }
    }
  }
  const float acc = sum16(acc2[0] + acc2[1]);
  if constexpr (METRIC == SVAE_LATENT_L2) return acc;   // a sum of squares from +0: never -0
  float s;
  if constexpr (METRIC == SVAE_LATENT_COSINE) s = (acc * in_q) * in_i;
  else s = fmaf(0.5f, acc, ld_i - ld_q) - half_z;
  return s + 0.0f;   // -0 -> +0: one zero, so the key below orders equal scores equally
}

// The selection key of a score as a float (smaller = better): the score, negated for COSINE.
template <int METRIC>
__device__ __forceinline__ float key_float(float s) {
  return METRIC == SVAE_LATENT_COSINE ? 0.0f - s : s;
}
// order-preserving u32 image of a key float
__device__ __forceinline__ unsigned float_key(float k) {
  const unsigned u = __float_as_uint(k);
  const unsigned o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  return k != k ? NAN_KEY : o;
}
// and back (NaN for the NaN key and the sentinel)
__device__ __forceinline__ float key_to_float(unsigned o) {
  if (o >= NAN_KEY) return __uint_as_float(0x7FC00000u);
  return __uint_as_float((o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o);
}
__device__ __forceinline__ float key_score(unsigned o, int metric) {
  const float k = key_to_float(o);
  return metric == SVAE_LATENT_COSINE ? 0.0f - k : k;
}

__device__ __forceinline__ u64 bcast64(u64 v, int src_lane) {   // src_lane wave-uniform: the result is scalar
  const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)v, src_lane);
  const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)(unsigned)(v >> 32), src_lane);
  return ((u64)hi << 32) | lo;
}

// sorted insert of the wave-uniform candidate c into the list held one entry per lane (entry 63 falls off)
__device__ __forceinline__ void list_insert(u64& lst, u64 c, int lane) {
  const int pos = __popcll(__ballot(lst < c));
  const u64 up = __shfl_up(lst, 1, 64);
  lst = lane < pos ? lst : (lane == pos ? c : up);
}

struct Corpus {
  const float* mu;
  const float* inv_var;
  const float* logdet;
  const float* inv_norm;
  int N, Z;
};
struct Queries {
  const float* mu;
  const float* scale;
  const float* logdet;
  const float* inv_norm;
  int Q;
};

// LDS: the query tile (mu, variance) while the corpus streams; the waves' lists for the merge afterwards
struct Smem {
  union {
    struct {
      float mu[QT * 256];
      float var[QT * 256];
    } q;
    u64 keys[4][QT][64];
  };
  float ld[QT], in[QT];
};

template <int METRIC>
__device__ __forceinline__ void stage_queries(Smem& sm, const Queries& qs, int q0, int Z) {
  for (int i = threadIdx.x; i < QT * Z; i += blockDim.x) {
    const int q = i / Z, j = i - q * Z, qq = q0 + q;
    const bool ok = qq < qs.Q;
    sm.q.mu[i] = ok ? qs.mu[(long long)qq * Z + j] : 0.f;
    if constexpr (METRIC == SVAE_LATENT_KL) {
      const float s = ok ? qs.scale[(long long)qq * Z + j] : 0.f;
      sm.q.var[i] = __fmul_rn(s, s);
    }
  }
  if (threadIdx.x < QT) {
    const int qq = q0 + threadIdx.x;
    const bool ok = qq < qs.Q;
    sm.ld[threadIdx.x] = (METRIC == SVAE_LATENT_KL && ok) ? qs.logdet[qq] : 0.f;
    sm.in[threadIdx.x] = (METRIC == SVAE_LATENT_COSINE && ok) ? qs.inv_norm[qq] : 0.f;
  }
  __syncthreads();
}

template <int METRIC, int ZC>
__device__ __forceinline__ void load_query(const Smem& sm, int qi, int Z, int sub, f32x4 (&qm)[ZC], f32x4 (&qv)[ZC]) {
#pragma unroll
  for (int c = 0; c < ZC; ++c) {
    const int ch = sub + 16 * c;
    const bool ok = 4 * ch < Z;
    const int off = qi * Z + (ok ? 4 * ch : 0);
    const f32x4 a = *(const f32x4*)&sm.q.mu[off];
    qm[c] = ok ? a : (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (METRIC == SVAE_LATENT_KL) {
      const f32x4 b = *(const f32x4*)&sm.q.var[off];
      qv[c] = ok ? b : (f32x4){0.f, 0.f, 0.f, 0.f};
    } else {
      qv[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
}

// this lane's chunks of row r (r in range)
template <int METRIC, int ZC>
__device__ __forceinline__ void load_row(const Corpus& cp, long long r, int sub, f32x4 (&m)[ZC], f32x4 (&iv)[ZC],
                                         float& ld, float& in) {
#pragma unroll
  for (int c = 0; c < ZC; ++c) {
    const int ch = sub + 16 * c;
    const bool ok = 4 * ch < cp.Z;
    const long long off = r * cp.Z + (ok ? 4 * ch : 0);
    const f32x4 a = *(const f32x4*)(cp.mu + off);
    m[c] = ok ? a : (f32x4){0.f, 0.f, 0.f, 0.f};
    if constexpr (METRIC == SVAE_LATENT_KL) {
      const f32x4 b = *(const f32x4*)(cp.inv_var + off);
      iv[c] = ok ? b : (f32x4){0.f, 0.f, 0.f, 0.f};
    } else {
      iv[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  ld = METRIC == SVAE_LATENT_KL ? cp.logdet[r] : 0.f;
  in = METRIC == SVAE_LATENT_COSINE ? cp.inv_norm[r] : 0.f;
}

// ---- prepare ---------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void latent_prepare_kernel(const float* __restrict__ mu,
                                                             const float* __restrict__ scale,
                                                             float* __restrict__ inv_var, float* __restrict__ logdet,
                                                             float* __restrict__ inv_norm, int N, int Z) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
  const int nch = Z >> 2;
  for (long long r0 = ((long long)blockIdx.x * 4 + wave) * 4; r0 < N; r0 += (long long)gridDim.x * 16) {
    const long long r = r0 + g;
    const bool valid = r < N;
    const long long rc = valid ? r : N - 1;
    float lsum = 0.f, nsum = 0.f;
    for (int ch = sub; ch < 64; ch += 16) {   // fixed trip count: the lanes stay together for the DPP sums
      const bool ok = ch < nch;
      const long long off = rc * Z + (ok ? 4 * ch : 0);
      const f32x4 m = *(const f32x4*)(mu + off), s = *(const f32x4*)(scale + off);
      f32x4 iv;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        iv[e] = __fdiv_rn(1.0f, __fmul_rn(s[e], s[e]));
        lsum += ok ? logf(s[e]) : 0.f;
        nsum = ok ? fmaf(m[e], m[e], nsum) : nsum;
      }
      if (ok && valid) *(f32x4*)(inv_var + off) = iv;
    }
    lsum = sum16(lsum);
    nsum = sum16(nsum);
    if (valid && sub == 0) {
      logdet[r] = lsum;
      inv_norm[r] = __fdiv_rn(1.0f, fmaxf(__fsqrt_rn(nsum), 1e-8f));
    }
  }
}

// ---- dense scores ------------------------------------------------------------------------------------------------
template <int METRIC, int ZC>
__global__ __launch_bounds__(256) void latent_scores_kernel(Corpus cp, Queries qs, float half_z,
                                                            float* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) Smem sm;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
  const int q0 = blockIdx.y * QT, nq = min(QT, qs.Q - q0);
  stage_queries<METRIC>(sm, qs, q0, cp.Z);
  for (long long r0 = ((long long)blockIdx.x * 4 + wave) * 4; r0 < cp.N; r0 += (long long)gridDim.x * 16) {
    const long long r = r0 + g;
    const bool valid = r < cp.N;
    f32x4 m[ZC], iv[ZC];
    float ld, in;
    load_row<METRIC, ZC>(cp, valid ? r : cp.N - 1, sub, m, iv, ld, in);
    for (int qi = 0; qi < nq; ++qi) {
      f32x4 qm[ZC], qv[ZC];
      load_query<METRIC, ZC>(sm, qi, cp.Z, sub, qm, qv);
      const float s = latent_score<METRIC, ZC>(m, iv, ld, in, qm, qv, sm.ld[qi], sm.in[qi], half_z);
      if (valid && sub == 0) out[(long long)(q0 + qi) * cp.N + r] = s;
    }
  }
}

// ---- top-k -------------------------------------------------------------------------------------------------------
// Best k of the four waves' lists for query slot qi, by counting: a candidate's rank is the number of candidates that
// precede it (key, then position: sentinels are equal keys). emit(rank, key) for rank < k. One wave per call.
template <class Emit>
__device__ __forceinline__ void merge_lists(const Smem& sm, int qi, int k, int lane, Emit emit) {
  for (int c = lane; c < 4 * k; c += 64) {
    const u64 mine = sm.keys[c / k][qi][c % k];
    int rank = 0, j = 0;
    for (int w = 0; w < 4; ++w)
      for (int e = 0; e < k; ++e, ++j) {
        const u64 o = sm.keys[w][qi][e];
        rank += (o < mine || (o == mine && j < c)) ? 1 : 0;
      }
    if (rank < k) emit(rank, mine);
  }
}

template <int METRIC, int ZC>
__global__ __launch_bounds__(256) void latent_topk_phase1_kernel(Corpus cp, Queries qs, float half_z, int q0, int k,
                                                                 int rows_per_block, u64* __restrict__ ws) {
  constexpr int U = ZC == 1 ? 8 : (ZC == 2 ? 4 : 2);   // row groups in flight per wave: U KiB (2 U for KL) at Z = 64
  constexpr bool QREG = ZC == 1;                       // the query tile lives in registers
  __shared__ __attribute__((aligned(16))) Smem sm;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, sub = lane & 15;
  const int nq = min(QT, qs.Q - q0);
  stage_queries<METRIC>(sm, qs, q0, cp.Z);

  f32x4 qm_r[QREG ? QT : 1][ZC], qv_r[QREG ? QT : 1][ZC];
  float qld[QT], qin[QT], thrf[QT];
  u64 lst[QT], thr[QT];
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) {
    if constexpr (QREG) load_query<METRIC, ZC>(sm, qi, cp.Z, sub, qm_r[qi], qv_r[qi]);
    qld[qi] = sm.ld[qi];
    qin[qi] = sm.in[qi];
    lst[qi] = SENT;
    thr[qi] = SENT;
    thrf[qi] = key_to_float((unsigned)(SENT >> 32));   // NaN: every score goes to the exact test until k are held
  }

  const long long row_begin = (long long)blockIdx.x * rows_per_block;
  const long long row_end = min((long long)cp.N, row_begin + rows_per_block);
  for (long long r0 = row_begin + wave * (4 * U); r0 < row_end; r0 += 4 * (4 * U)) {
    f32x4 m[U][ZC], iv[U][ZC];
    float ld[U], in[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const long long r = r0 + 4 * u + g;
      load_row<METRIC, ZC>(cp, r < row_end ? r : row_end - 1, sub, m[u], iv[u], ld[u], in[u]);
    }
#pragma unroll
    for (int qi = 0; qi < QT; ++qi) {
      if (qi < nq) {
        f32x4 qm[ZC], qv[ZC];
        if constexpr (QREG) {
#pragma unroll
          for (int c = 0; c < ZC; ++c) qm[c] = qm_r[qi][c], qv[c] = qv_r[qi][c];
        } else {
          load_query<METRIC, ZC>(sm, qi, cp.Z, sub, qm, qv);
        }
        // Fast test, one compare per score: can this key float beat or tie the k-th best's? (Conservative: ties, NaNs
        // and the rows past the end go on to the exact 64-bit key test below, which alone decides.)
        // fminf drops a NaN operand; a NaN key can only enter a list whose k-th entry is not yet a number, and then
        // thrf is NaN and the compare below is true for every score.
        float kf[U], best = __builtin_inff();
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const float s = latent_score<METRIC, ZC>(m[u], iv[u], ld[u], in[u], qm, qv, qld[qi], qin[qi], half_z);
          kf[u] = key_float<METRIC>(s);
          best = fminf(best, kf[u]);
        }
        if (__ballot(!(best > thrf[qi]))) {
#pragma unroll
          for (int u = 0; u < U; ++u) {
            const long long r = r0 + 4 * u + g;
            const u64 key = r < row_end ? (((u64)float_key(kf[u]) << 32) | (unsigned)r) : SENT;
            u64 mask = __ballot(key < thr[qi]) & 0x0001000100010001ull;   // one lane per row group
            while (mask) {
              const int src = __ffsll((long long)mask) - 1;
              mask &= mask - 1;
              const u64 c = bcast64(key, src);
              if (c < thr[qi]) {
                list_insert(lst[qi], c, lane);
                thr[qi] = bcast64(lst[qi], k - 1);
                thrf[qi] = key_to_float((unsigned)(thr[qi] >> 32));
              }
            }
          }
        }
      }
    }
  }

  __syncthreads();   // the query tile is dead: its LDS becomes the merge buffer
#pragma unroll
  for (int qi = 0; qi < QT; ++qi) sm.keys[wave][qi][lane] = lst[qi];
  __syncthreads();
  const int nblk = gridDim.x;
  for (int qi = wave; qi < nq; qi += 4) {
    u64* dst = ws + ((long long)(q0 + qi) * nblk + blockIdx.x) * k;
    merge_lists(sm, qi, k, lane, [&](int rank, u64 key) { dst[rank] = key; });
  }
}

// one workgroup per query: the blocks * k candidates -> the sorted result
__global__ __launch_bounds__(256) void latent_topk_phase2_kernel(const u64* __restrict__ ws, int ncand, int k,
                                                                 int metric, float* __restrict__ scores,
                                                                 int32_t* __restrict__ indices) {
  __shared__ __attribute__((aligned(16))) Smem sm;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.x;
  const u64* src = ws + (long long)q * ncand;
  u64 lst = SENT, thr = SENT;
  for (int base = wave * 64; base < ncand; base += 256) {
    const int i = base + lane;
    const u64 key = i < ncand ? src[i] : SENT;
    u64 mask = __ballot(key < thr);
    while (mask) {
      const int s = __ffsll((long long)mask) - 1;
      mask &= mask - 1;
      const u64 c = bcast64(key, s);
      if (c < thr) {
        list_insert(lst, c, lane);
        thr = bcast64(lst, k - 1);
      }
    }
  }
  sm.keys[wave][0][lane] = lst;
  __syncthreads();
  if (wave == 0)
    merge_lists(sm, 0, k, lane, [&](int rank, u64 key) {
      scores[(long long)q * k + rank] = key_score((unsigned)(key >> 32), metric);
      indices[(long long)q * k + rank] = (int32_t)(unsigned)key;
    });
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

bool bad_shape(int32_t metric, const Queries& qs, const Corpus& cp) {
  if (metric < SVAE_LATENT_L2 || metric > SVAE_LATENT_KL) return true;
  if (cp.Z < 4 || cp.Z > 256 || cp.Z % 4 || cp.N < 1 || qs.Q < 1) return true;
  if (!qs.mu || !cp.mu || !aligned16(qs.mu) || !aligned16(cp.mu)) return true;
  if (metric == SVAE_LATENT_COSINE && (!qs.inv_norm || !cp.inv_norm)) return true;
  if (metric == SVAE_LATENT_KL &&
      (!qs.scale || !qs.logdet || !cp.inv_var || !cp.logdet || !aligned16(qs.scale) || !aligned16(cp.inv_var)))
    return true;
  return false;
}

#define LATENT_DISPATCH(KERNEL, metric, zc, ...)                                         \
  do {                                                                                   \
    switch ((metric) * 4 + (zc) - 1) {                                                   \
      case 0: KERNEL(SVAE_LATENT_L2, 1, __VA_ARGS__); break;                             \
      case 1: KERNEL(SVAE_LATENT_L2, 2, __VA_ARGS__); break;                             \
      case 2: KERNEL(SVAE_LATENT_L2, 3, __VA_ARGS__); break;                             \
      case 3: KERNEL(SVAE_LATENT_L2, 4, __VA_ARGS__); break;                             \
      case 4: KERNEL(SVAE_LATENT_COSINE, 1, __VA_ARGS__); break;                         \
      case 5: KERNEL(SVAE_LATENT_COSINE, 2, __VA_ARGS__); break;                         \
      case 6: KERNEL(SVAE_LATENT_COSINE, 3, __VA_ARGS__); break;                         \
      case 7: KERNEL(SVAE_LATENT_COSINE, 4, __VA_ARGS__); break;                         \
      case 8: KERNEL(SVAE_LATENT_KL, 1, __VA_ARGS__); break;                             \
      case 9: KERNEL(SVAE_LATENT_KL, 2, __VA_ARGS__); break;                             \
      case 10: KERNEL(SVAE_LATENT_KL, 3, __VA_ARGS__); break;                            \
      default: KERNEL(SVAE_LATENT_KL, 4, __VA_ARGS__); break;                            \
    }                                                                                    \
  } while (0)

#define LAUNCH_SCORES(M, ZC, grid, s, cp, qs, hz, out) \
  hipLaunchKernelGGL((latent_scores_kernel<M, ZC>), grid, dim3(256), 0, s, cp, qs, hz, out)
#define LAUNCH_PHASE1(M, ZC, grid, s, cp, qs, hz, q0, k, rpb, ws) \
  hipLaunchKernelGGL((latent_topk_phase1_kernel<M, ZC>), grid, dim3(256), 0, s, cp, qs, hz, q0, k, rpb, ws)

// Workgroups of a phase-1 instantiation that fit on the chip at once (CUs x resident workgroups per CU, by its
// registers and LDS): the persistent grid is one such round, so no second, partly filled round follows it.
// Cached per device of the current context (an atomic slot each: concurrent first calls compute the same value). A
// failed query falls back to 256 CUs x 1 and clears only its own error.
template <int METRIC, int ZC>
int phase1_resident_blocks() {
  constexpr int MAX_DEV = 64;
  static std::atomic<int> cache[MAX_DEV];
  int dev = 0;
  bool failed = hipGetDevice(&dev) != hipSuccess;
  const bool slot = !failed && dev >= 0 && dev < MAX_DEV;
  if (slot) {
    const int hit = cache[dev].load(std::memory_order_relaxed);
    if (hit) return hit;
  }
  int cus = 0, per_cu = 0;
  if (failed || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1) {
    failed = true;
    cus = 256;
  }
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, latent_topk_phase1_kernel<METRIC, ZC>, 256, 0) !=
          hipSuccess ||
      per_cu < 1) {
    failed = true;
    per_cu = 1;
  }
  if (failed) {
    (void)hipGetLastError();
    return cus * per_cu;
  }
  if (slot) cache[dev].store(cus * per_cu, std::memory_order_relaxed);
  return cus * per_cu;
}
#define RESIDENT_BLOCKS(M, ZC, out) out = phase1_resident_blocks<M, ZC>()

}  // namespace

SVAE_EXPORT int svae_latent_prepare(const float* mu, const float* scale, float* inv_var, float* logdet,
                                    float* inv_norm, int32_t N, int32_t Z, svae_stream_t stream) {
  if (!mu || !scale || !inv_var || !logdet || !inv_norm || N < 1 || Z < 4 || Z > 256 || Z % 4) return SVAE_EINVAL;
  if (!aligned16(mu) || !aligned16(scale) || !aligned16(inv_var)) return SVAE_EINVAL;
  const int grid = (int)min((long long)2048, ((long long)N + 15) / 16);
  hipLaunchKernelGGL(latent_prepare_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, mu, scale, inv_var, logdet,
                     inv_norm, N, Z);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_latent_scores(int32_t metric, const float* q_mu, const float* q_scale, const float* q_logdet,
                                   const float* q_inv_norm, int32_t Q, const float* mu, const float* inv_var,
                                   const float* logdet, const float* inv_norm, int32_t N, int32_t Z, float* out,
                                   svae_stream_t stream) {
  const Queries qs{q_mu, q_scale, q_logdet, q_inv_norm, Q};
  const Corpus cp{mu, inv_var, logdet, inv_norm, N, Z};
  if (bad_shape(metric, qs, cp) || !out) return SVAE_EINVAL;
  const int zc = (Z / 4 + 15) / 16;
  const float hz = 0.5f * (float)Z;
  constexpr int QSTEP = 65535 * QT;   // queries per launch: the grid's y limit
  for (int qb = 0; qb < Q; qb += QSTEP) {
    const int nq = min(QSTEP, Q - qb);
    const Queries part{q_mu + (long long)qb * Z, q_scale ? q_scale + (long long)qb * Z : nullptr,
                       q_logdet ? q_logdet + qb : nullptr, q_inv_norm ? q_inv_norm + qb : nullptr, nq};
    const dim3 grid((unsigned)min((long long)2048, ((long long)N + 15) / 16), (unsigned)((nq + QT - 1) / QT));
    float* dst = out + (long long)qb * N;
    LATENT_DISPATCH(LAUNCH_SCORES, metric, zc, grid, (hipStream_t)stream, cp, part, hz, dst);
  }
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_latent_topk_ws_bytes(int32_t Q, int32_t k) {
  if (Q < 1 || k < 1 || k > 64) return 0;
  return (int64_t)Q * MAXB * k * (int64_t)sizeof(u64);
}

SVAE_EXPORT int svae_latent_topk(int32_t metric, const float* q_mu, const float* q_scale, const float* q_logdet,
                                 const float* q_inv_norm, int32_t Q, const float* mu, const float* inv_var,
                                 const float* logdet, const float* inv_norm, int32_t N, int32_t Z, int32_t k, void* ws,
                                 int64_t ws_bytes, float* scores, int32_t* indices, svae_stream_t stream) {
  const Queries qs{q_mu, q_scale, q_logdet, q_inv_norm, Q};
  const Corpus cp{mu, inv_var, logdet, inv_norm, N, Z};
  if (bad_shape(metric, qs, cp) || k < 1 || k > 64 || k > N || !scores || !indices) return SVAE_EINVAL;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < svae_latent_topk_ws_bytes(Q, k)) return SVAE_EINVAL;
  const int zc = (Z / 4 + 15) / 16;
  int resident = MAXB;
  LATENT_DISPATCH(RESIDENT_BLOCKS, metric, zc, resident);
  const int nblk = (int)min((long long)min(MAXB, resident), ((long long)N + MIN_ROWS - 1) / MIN_ROWS);
  const int rpb = (int)(((long long)N + nblk - 1) / nblk);
  const float hz = 0.5f * (float)Z;
  hipStream_t s = (hipStream_t)stream;
  for (int q0 = 0; q0 < Q; q0 += QT)
    LATENT_DISPATCH(LAUNCH_PHASE1, metric, zc, dim3(nblk), s, cp, qs, hz, q0, (int)k, rpb, (u64*)ws);
  hipLaunchKernelGGL(latent_topk_phase2_kernel, dim3(Q), dim3(256), 0, s, (const u64*)ws, nblk * (int)k, (int)k,
                     (int)metric, scores, indices);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
