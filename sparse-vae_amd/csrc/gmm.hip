// A diagonal Gaussian mixture of the latent index (ex-post density estimation): EM over the rows' posteriors
// q_i = N(mu_i, diag(s2_i)) or over plain points (s2 = NULL), a sampler and a density. It stands where the reference
// has only torch.randn (transformer_vae.py:103): a prior fitted to the aggregate posterior after training.
//
//   svae_gmm_prepare: the derived rows (inv_var, sd, logc) of a parameter block from (weight, mean, var).
//   svae_gmm_estep:   per row the log-sum-exp of a_ik over the components, the argmax component and optionally the
//                     responsibilities; the bound sum_i lse_i. A workgroup owns 256 rows (one per lane, in registers)
//                     and streams (mean, inv_var, logc) through LDS in tiles; one workgroup adds the partials.
//   svae_gmm_mstep:   f64 sufficient statistics per (component, row group), one wave each, then the new parameters and
//                     their derived rows. Soft (from lse) or hard (from labels).
//   svae_gmm_sample:  the component of every row from the f64 prefix sums of the weights, then z = fmaf(sd, eps, mean).
//
// No atomics anywhere: grids and summation orders are functions of (N, K, Z) alone, so a result is a pure function of
// its inputs, bit for bit. Arithmetic and orders:
//   a_ik      = E_{q_i} log pi_k N(z; m_k, v_k) = logc_k - q / 2, q = sum_d ((x_d - m_d)^2 + s2_d) inv_var_d, in f32 from
//             direct differences: per float4 chunk of the row d = x - m (one rounding per element), e = fmaf(d, d, s2)
//             (s2 = 0 for points), then two fmaf chains s = fmaf(e, inv_var, s), one over elements 0 and 2 and one
//             over elements 1 and 3 of the chunks in chunk order (the two halves of a v_pk_fma_f32), q = chain A +
//             chain B, a = fmaf(-0.5, q, logc). Contraction is off and the FMAs are written out; the order depends on Z
//             alone and the E-step, the responsibilities and the M-step share the function, so a (row, component) pair
//             has one f32 value whichever kernel, lane or workgroup computes it. logc = -inf gives a = -inf whatever q
//             is. A chain takes Z / 2 FMAs on a partial sum of non-negative terms (one rounding each), a term carries
//             the two roundings of its difference, the rounding of e and the rounding of inv_var = (float)(1 / var),
//             and the chains' sum is one more; the last fmaf rounds a once and logc was rounded once from f64:
//             |error| <= ((Z / 2 + 5) q / 2 + |logc| + |a|) 2^-24 to first order, against the f64 value from the
//             same f32 (x, s2, weight, mean, var).
//   lse       online over the components in index order, per row: (M, S) start at (-inf, 0); a component with
//             a = -inf is skipped (it contributes exactly 0); a > M: S = fmaf(S, expf(M - a), 1), M = a; else
//             S += expf(a - M). lse = M + logf(S). A NaN a_ik makes lse_i NaN. expf and logf are the library's
//             (1 ulp), not the fast intrinsics.
//   argmax    the components in index order; a component replaces the lane's best only if its a is larger, or is a
//             number where the best is NaN: ties go to the lower index, NaN loses to every number (-inf is a number),
//             an all-NaN row keeps label 0.
//   bound     sum_i lse_i: widened to f64 per row; 64-lane xor butterfly, the four waves in order; the total: lane t
//             adds workgroups t, t + 256, ..., butterfly, waves (as k-means' inertia).
//   resp      r_ik = expf(a_ik - lse_i), one thread per row in a second launch once lse is known.
//   mstep     the rows are cut into G groups of consecutive rows (G and the rows per group, a multiple of 64, from
//             (N, K) alone: svae_gmm_geometry). One wave per (four components, group), so that a row is read once for
//             four components; per component: 64 rows at a time, lane l forms r of
//             row l (soft: expf(a - lse) with a from the function above; hard: label == k), then the 64 rows are added
//             in ascending order, lane l owning the dimensions l, l + 64, ...: N_k += r, S1_d += r d,
//             S2_d += r (d^2 + s2_d) with d = (double)(x_d - m_d) (the f32 difference) and everything else in f64. A
//             row with r == 0 is skipped (adding an exact zero changes nothing). The groups are then added in
//             ascending order. m = m_old + S1 / N_k, v = S2 / N_k - (S1 / N_k)^2 + reg_covar, pi_k = N_k / sum of the
//             positive N_k in index order, all in f64, rounded to f32 once. N_k not > 0: mean and variance stay, the
//             weight is 0.
//   derived   inv_var = (float)(1 / (double)var), sd = (float)sqrt((double)var), logc = (float)(log((double)pi) -
//             0.5 sum_d log(2 pi (double)v_d)) with the sum in ascending d.
//   sample    cum_k = the inclusive prefix sums of max(weight, 0) in f64 in index order (a NaN weight counts 0); row j
//             takes the first k with cum_k > (double)u_j * cum_{K-1}, clamped to the last component of positive weight
//             (component 0 if there is none).
#include <math.h>

#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int TC = SVAE_GMM_TILE_COMPONENTS;   // components per LDS tile
constexpr int MAXK = SVAE_GMM_MAX_K;
constexpr int RB = SVAE_GMM_ROWS_PER_BLOCK;    // rows per E-step workgroup
constexpr int SEG_ITEMS = 16384;               // (component, row group) pairs aimed at: 256 CUs x 16 waves of four
constexpr int MAX_ROWS = 1 << 24;
constexpr unsigned long long COMP_STREAM = 0x636F6D706F6E656Eull;   // the component draw's stream: seed ^ this
static_assert(RB == 256 && TC * 256 * 2 * 4 <= 32768, "geometry");

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One float4 chunk of a (row, component) pair: THE a_ik arithmetic, shared by every kernel below.
__device__ __forceinline__ void gmm_chunk(f32x2& s, const f32x4 xv, const f32x4 sv, const f32x4 mv, const f32x4 iv) {
#pragma clang fp contract(off)
  const f32x4 d = xv - mv;
  const f32x2 dlo = {d[0], d[1]}, dhi = {d[2], d[3]};
  const f32x2 elo = __builtin_elementwise_fma(dlo, dlo, (f32x2){sv[0], sv[1]});
  const f32x2 ehi = __builtin_elementwise_fma(dhi, dhi, (f32x2){sv[2], sv[3]});
  s = __builtin_elementwise_fma(elo, (f32x2){iv[0], iv[1]}, s);
  s = __builtin_elementwise_fma(ehi, (f32x2){iv[2], iv[3]}, s);
}
__device__ __forceinline__ float gmm_finish(const f32x2 s, const float logc) {
#pragma clang fp contract(off)
  const float q = s[0] + s[1];
  const float a = fmaf(-0.5f, q, logc);
  return logc == -INFINITY ? -INFINITY : a;
}
// a_ik of a row in memory against a component in memory (or LDS).
__device__ __forceinline__ float gmm_a(const float* __restrict__ xr, const float* __restrict__ sr, const float* mean,
                                       const float* iv, float logc, int zc_n) {
  f32x2 s = {0.f, 0.f};
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
  for (int zc = 0; zc < zc_n; ++zc)
    gmm_chunk(s, *(const f32x4*)(xr + 4 * zc), sr ? *(const f32x4*)(sr + 4 * zc) : zero,
              *(const f32x4*)(mean + 4 * zc), *(const f32x4*)(iv + 4 * zc));
  return gmm_finish(s, logc);
}

struct Params {
  float *weight, *logc, *mean, *var, *inv_var, *sd;
};
__host__ __device__ __forceinline__ Params params_of(float* p, int K, int Z) {
  const long long kp = SVAE_GMM_KPAD(K), kz = (long long)K * Z;
  return Params{p, p + kp, p + 2 * kp, p + 2 * kp + kz, p + 2 * kp + 2 * kz, p + 2 * kp + 3 * kz};
}

// ---- derived rows --------------------------------------------------------------------------------------------------
// One wave: the derived rows of component k from its (weight, mean, var). sh: 256 doubles of LDS owned by the wave.
__device__ __forceinline__ void derive_component(const Params& P, int k, int Z, int lane, double* sh) {
#pragma clang fp contract(off)
  for (int d = lane; d < Z; d += 64) {
    const double v = (double)P.var[(long long)k * Z + d];
    P.inv_var[(long long)k * Z + d] = (float)(1.0 / v);
    P.sd[(long long)k * Z + d] = (float)sqrt(v);
    sh[d] = log(6.283185307179586476925 * v);
  }
  __syncthreads();   // the callers run one wave per workgroup
  if (lane == 0) {
    double s = 0.0;
    for (int d = 0; d < Z; ++d) s += sh[d];
    P.logc[k] = (float)(log((double)P.weight[k]) - 0.5 * s);
  }
}

__global__ __launch_bounds__(64) void prepare_kernel(float* __restrict__ params, int K, int Z) {
  __shared__ double sh[256];
  const Params P = params_of(params, K, Z);
  derive_component(P, blockIdx.x, Z, threadIdx.x, sh);
}

// ---- E-step --------------------------------------------------------------------------------------------------------
// grid: row blocks of 256 rows. A lane holds ZCAP floats of its row (and of its s2 row) in registers. NSEG == 1: the
// whole row, loaded once. NSEG == 4 (Z > 128 with s2: two rows' worth of registers would not fit): per component tile
// the row is loaded in four segments of 64, and the tile's TC chains wait in registers between them; the chunk order is
// the same.
template <int ZCAP, int NSEG, bool S2>
__global__ __launch_bounds__(256) void estep_kernel(const float* __restrict__ x, const float* __restrict__ s2, int N,
                                                    const float* __restrict__ params, int K, int Z,
                                                    float* __restrict__ lse, int* __restrict__ label,
                                                    double* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int ZT = ZCAP * NSEG, CH = ZCAP / 4;
  __shared__ __attribute__((aligned(16))) float tmean[TC * ZT];
  __shared__ __attribute__((aligned(16))) float tiv[TC * ZT];
  __shared__ float tlogc[TC];
  __shared__ double redd[4];
  const Params P = params_of(const_cast<float*>(params), K, Z);
  const int tid = threadIdx.x, zc_n = Z >> 2;
  const int row = blockIdx.x * RB + tid;
  const long long off = (long long)min(row, N - 1) * Z;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 xi[CH], si[S2 ? CH : 1];
  auto load_seg = [&](int seg) {
#pragma unroll
    for (int zc = 0; zc < CH; ++zc) {
      const int gz = seg * CH + zc;
      xi[zc] = gz < zc_n ? *(const f32x4*)(x + off + 4 * gz) : zero;
      if constexpr (S2) si[zc] = gz < zc_n ? *(const f32x4*)(s2 + off + 4 * gz) : zero;
    }
  };
  if constexpr (NSEG == 1) load_seg(0);
  float best = __builtin_nanf(""), M = -INFINITY, S = 0.f;
  int bi = 0;
  auto take = [&](float a, int k) {
    const bool t = a > best || (best != best && a == a);
    best = t ? a : best;
    bi = t ? k : bi;
    if (a != -INFINITY) {
      if (a > M) {
        S = fmaf(S, expf(M - a), 1.f);
        M = a;
      } else {
        S += expf(a - M);
      }
    }
  };
  for (int c0 = 0; c0 < K; c0 += TC) {
    const int nc = min(TC, K - c0);   // workgroup-uniform
    __syncthreads();                  // the previous tile has been read
    for (int v = tid; v < nc * zc_n; v += 256) {
      *(f32x4*)&tmean[4 * v] = *(const f32x4*)(P.mean + (long long)c0 * Z + 4 * v);
      *(f32x4*)&tiv[4 * v] = *(const f32x4*)(P.inv_var + (long long)c0 * Z + 4 * v);
    }
    if (tid < nc) tlogc[tid] = P.logc[c0 + tid];
    __syncthreads();
    if constexpr (NSEG == 1) {
      for (int jj = 0; jj < nc; ++jj) {
        const float* mj = tmean + jj * Z;   // the same address in every lane: a broadcast
        const float* vj = tiv + jj * Z;
        f32x2 s = {0.f, 0.f};
#pragma unroll
        for (int zc = 0; zc < CH; ++zc) {
          if (zc < zc_n) {   // workgroup-uniform
            f32x4 sv = zero;
            if constexpr (S2) sv = si[zc];
            gmm_chunk(s, xi[zc], sv, *(const f32x4*)(mj + 4 * zc), *(const f32x4*)(vj + 4 * zc));
          }
        }
        take(gmm_finish(s, tlogc[jj]), c0 + jj);
      }
    } else {
      f32x2 sp[TC];
#pragma unroll
      for (int jj = 0; jj < TC; ++jj) sp[jj] = (f32x2){0.f, 0.f};
#pragma unroll
      for (int seg = 0; seg < NSEG; ++seg) {
        load_seg(seg);
#pragma unroll
        for (int jj = 0; jj < TC; ++jj) {
          if (jj < nc) {
            const float* mj = tmean + jj * Z + seg * ZCAP;
            const float* vj = tiv + jj * Z + seg * ZCAP;
#pragma unroll
            for (int zc = 0; zc < CH; ++zc) {
              if (seg * CH + zc < zc_n) {
                f32x4 sv = zero;
                if constexpr (S2) sv = si[zc];
                gmm_chunk(sp[jj], xi[zc], sv, *(const f32x4*)(mj + 4 * zc), *(const f32x4*)(vj + 4 * zc));
              }
            }
          }
        }
      }
#pragma unroll
      for (int jj = 0; jj < TC; ++jj)
        if (jj < nc) take(gmm_finish(sp[jj], tlogc[jj]), c0 + jj);
    }
  }
  const float l = M + logf(S);
  double l64 = 0.0;
  if (row < N) {
    lse[row] = l;
    if (label) label[row] = bi;
    l64 = (double)l;
  }
  l64 = wave_sum_d(l64);
  if ((tid & 63) == 0) redd[tid >> 6] = l64;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = ((redd[0] + redd[1]) + redd[2]) + redd[3];
}

__global__ __launch_bounds__(256) void estep_final_kernel(const double* __restrict__ part, int n,
                                                          double* __restrict__ bound) {
  __shared__ double redd[4];
  const int tid = threadIdx.x;
  double v = 0.0;
  for (int i = tid; i < n; i += 256) v += part[i];
  v = wave_sum_d(v);
  if ((tid & 63) == 0) redd[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) *bound = ((redd[0] + redd[1]) + redd[2]) + redd[3];
}

// One thread per row: resp[row][k] = expf(a - lse[row]).
__global__ __launch_bounds__(256) void resp_kernel(const float* __restrict__ x, const float* __restrict__ s2, int N,
                                                   const float* __restrict__ params, int K, int Z,
                                                   const float* __restrict__ lse, float* __restrict__ resp) {
#pragma clang fp contract(off)
  const Params P = params_of(const_cast<float*>(params), K, Z);
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= N) return;
  const float* xr = x + (long long)row * Z;
  const float* sr = s2 ? s2 + (long long)row * Z : nullptr;
  const float l = lse[row];
  for (int k = 0; k < K; ++k) {
    const float a = gmm_a(xr, sr, P.mean + (long long)k * Z, P.inv_var + (long long)k * Z, P.logc[k], Z >> 2);
    resp[(long long)row * K + k] = expf(a - l);
  }
}

// ---- M-step --------------------------------------------------------------------------------------------------------
// grid (ceil(K / (4 CK)), G), four waves: wave w owns the CK components from (4 blockIdx.x + w) CK inside row group
// blockIdx.y, so a row is read once for CK components. part f64 [G][K][2 Z + 1] = {N_k, S1[Z], S2[Z]}.
constexpr int CK = 4;
__global__ __launch_bounds__(256) void mstep_stats_kernel(const float* __restrict__ x, const float* __restrict__ s2,
                                                          int N, const float* __restrict__ lse,
                                                          const int* __restrict__ label,
                                                          const float* __restrict__ params, int K, int Z, int rpg,
                                                          double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float cm[4][CK][256];
  __shared__ __attribute__((aligned(16))) float cv[4][CK][256];
  const Params P = params_of(const_cast<float*>(params), K, Z);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int k0 = (blockIdx.x * 4 + w) * CK, g = blockIdx.y, zc_n = Z >> 2;
  const int nck = min(CK, K - k0);   // wave-uniform; <= 0: nothing to do
  float logc[CK];
#pragma unroll
  for (int c = 0; c < CK; ++c) {
    const int kk = min(k0 + c, K - 1);   // a component past K is computed and never used
    for (int d = lane; d < Z; d += 64)
      cm[w][c][d] = P.mean[(long long)kk * Z + d], cv[w][c][d] = P.inv_var[(long long)kk * Z + d];
    logc[c] = P.logc[kk];
  }
  __syncthreads();
  if (nck <= 0) return;
  const int r0 = g * rpg, r1 = min(N, r0 + rpg);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  float md[CK][4];
  double nk[CK], s1[CK][4], sq[CK][4];
#pragma unroll
  for (int c = 0; c < CK; ++c) {
    nk[c] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) md[c][j] = lane + 64 * j < Z ? cm[w][c][lane + 64 * j] : 0.f, s1[c][j] = sq[c][j] = 0.0;
  }
  for (int b = r0; b < r1; b += 64) {
    const int row = b + lane;
    float r[CK];
#pragma unroll
    for (int c = 0; c < CK; ++c) r[c] = 0.f;
    if (row < r1) {
      if (lse) {
        const float* xr = x + (long long)row * Z;
        const float* sr = s2 ? s2 + (long long)row * Z : nullptr;
        f32x2 s[CK];
#pragma unroll
        for (int c = 0; c < CK; ++c) s[c] = (f32x2){0.f, 0.f};
#pragma unroll 2
        for (int zc = 0; zc < zc_n; ++zc) {
          const f32x4 xv = *(const f32x4*)(xr + 4 * zc), sv = sr ? *(const f32x4*)(sr + 4 * zc) : zero;
#pragma unroll
          for (int c = 0; c < CK; ++c)
            gmm_chunk(s[c], xv, sv, *(const f32x4*)&cm[w][c][4 * zc], *(const f32x4*)&cv[w][c][4 * zc]);
        }
        const float l = lse[row];
#pragma unroll
        for (int c = 0; c < CK; ++c) r[c] = c < nck ? expf(gmm_finish(s[c], logc[c]) - l) : 0.f;
      } else {
        const int lab = label[row];
#pragma unroll
        for (int c = 0; c < CK; ++c) r[c] = c < nck && lab == k0 + c ? 1.f : 0.f;
      }
    }
    bool any = false;
#pragma unroll
    for (int c = 0; c < CK; ++c) any = any || r[c] != 0.f;   // a NaN r counts
    const unsigned long long live = __ballot(any);
    const int nb = min(64, r1 - b);
    for (int i = 0; i < nb; ++i) {
      if (!((live >> i) & 1ull)) continue;   // wave-uniform: the row has r == 0 for all CK components
      const long long o = (long long)(b + i) * Z;
      float xv[4], sv[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = lane + 64 * j < Z;
        xv[j] = in ? x[o + lane + 64 * j] : 0.f;
        sv[j] = in && s2 ? s2[o + lane + 64 * j] : 0.f;
      }
#pragma unroll
      for (int c = 0; c < CK; ++c) {
        const float ri = __shfl(r[c], i, 64);   // wave-uniform
        if (ri != 0.f) {
          const double r64 = (double)ri;
          nk[c] += r64;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (lane + 64 * j < Z) {
              const double d = (double)(xv[j] - md[c][j]);
              const double e = s2 ? d * d + (double)sv[j] : d * d;
              s1[c][j] += r64 * d;
              sq[c][j] += r64 * e;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CK; ++c) {
    if (c < nck) {
      double* out = part + ((long long)g * K + k0 + c) * (2 * Z + 1);
      if (lane == 0) out[0] = nk[c];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (lane + 64 * j < Z) out[1 + lane + 64 * j] = s1[c][j], out[1 + Z + lane + 64 * j] = sq[c][j];
    }
  }
}

// One thread per statistic: tot[k][2 Z + 1] = the groups in ascending order.
__global__ __launch_bounds__(256) void mstep_reduce_kernel(const double* __restrict__ part, int G, long long n,
                                                           double* __restrict__ tot) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += part[(long long)g * n + i];
  tot[i] = s;
}

// grid K, one wave: the new (weight, mean, var) of component k and its derived rows.
__global__ __launch_bounds__(64) void mstep_final_kernel(const double* __restrict__ tot, float* __restrict__ params,
                                                         int K, int Z, float reg_covar, double* __restrict__ nk_out) {
#pragma clang fp contract(off)
  __shared__ double sh[256];
  __shared__ double s_total;
  const Params P = params_of(params, K, Z);
  const int k = blockIdx.x, lane = threadIdx.x, st = 2 * Z + 1;
  if (lane == 0) {
    double t = 0.0;
    for (int c = 0; c < K; ++c) {
      const double n = tot[(long long)c * st];
      if (n > 0.0) t += n;
    }
    s_total = t;
  }
  __syncthreads();
  const double nk = tot[(long long)k * st];
  if (nk > 0.0) {
    for (int d = lane; d < Z; d += 64) {
      const double m1 = tot[(long long)k * st + 1 + d] / nk, m2 = tot[(long long)k * st + 1 + Z + d] / nk;
      P.mean[(long long)k * Z + d] = (float)((double)P.mean[(long long)k * Z + d] + m1);
      P.var[(long long)k * Z + d] = (float)(m2 - m1 * m1 + (double)reg_covar);
    }
  }
  if (lane == 0) {
    P.weight[k] = nk > 0.0 ? (float)(nk / s_total) : 0.f;
    nk_out[k] = nk;
  }
  __syncthreads();   // one wave: the parameters written above are read back below
  derive_component(P, k, Z, lane, sh);
}

// ---- sample --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void sample_comp_kernel(const float* __restrict__ params, int K, int Z, int n,
                                                          const float* __restrict__ u, unsigned long long seed,
                                                          int* __restrict__ comp) {
  __shared__ double cum[MAXK];
  __shared__ int s_last;
  const Params P = params_of(const_cast<float*>(params), K, Z);
  if (threadIdx.x == 0) {
    double c = 0.0;
    int last = 0;
    for (int k = 0; k < K; ++k) {
      const float wk = P.weight[k];
      if (wk > 0.f) c += (double)wk, last = k;
      cum[k] = c;
    }
    s_last = last;
  }
  __syncthreads();
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const float uj = u ? u[j] : rand_uniform(seed ^ COMP_STREAM, (unsigned long long)j);
  const double target = (double)uj * cum[K - 1];
  int lo = 0, hi = K;   // the first k with cum_k > target (cum is non-decreasing); K if there is none
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (cum[mid] > target) hi = mid;
    else lo = mid + 1;
  }
  comp[j] = min(lo, s_last);
}

__global__ __launch_bounds__(256) void sample_draw_kernel(const float* __restrict__ params, int K, int Z, long long n,
                                                          const int* __restrict__ comp, const float* __restrict__ eps,
                                                          unsigned long long seed, float* __restrict__ z) {
  const Params P = params_of(const_cast<float*>(params), K, Z);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float e;
    if (eps) {
      e = eps[i];
    } else {   // svae_latent_draw's normals: the same counters, the same arithmetic
      const unsigned long long idx = 2ull * (unsigned long long)i;   // i = row * Z + column
      const float u1 = rand_uniform(seed, idx), u2 = rand_uniform(seed, idx + 1);
      e = sqrtf(-2.f * __logf(u1)) * __cosf(6.283185307179586f * u2);
    }
    const int row = (int)(i / Z), col = (int)(i - (long long)row * Z);
    const int k = max(0, min(comp[row], K - 1));
    z[i] = fmaf(P.sd[(long long)k * Z + col], e, P.mean[(long long)k * Z + col]);
  }
}

// ---- host ----------------------------------------------------------------------------------------------------------
struct Geom {
  int row_blocks, groups, rpg, segs;
};
bool bad_kz(int32_t K, int32_t Z) { return Z < 4 || Z > 256 || (Z & 3) || K < 1 || K > MAXK; }
bool bad_shape(int32_t N, int32_t K, int32_t Z) { return N < 1 || N > MAX_ROWS || bad_kz(K, Z); }
Geom geom_of(int N, int K, int Z, bool has_s2) {
  Geom g;
  g.row_blocks = (N + RB - 1) / RB;
  int gw = SEG_ITEMS / K;
  gw = gw < 1 ? 1 : gw;
  const int per = (N + gw - 1) / gw;
  g.rpg = (per + 63) / 64 * 64;
  g.groups = (N + g.rpg - 1) / g.rpg;
  g.segs = has_s2 && Z > 128 ? 4 : 1;
  return g;
}
bool bad_ptr(const void* p, int align) { return !p || ((uintptr_t)p & (uintptr_t)(align - 1)); }
bool bad_opt(const void* p, int align) { return ((uintptr_t)p & (uintptr_t)(align - 1)) != 0; }
bool bad_ws(const void* ws, int64_t have, int64_t need) { return bad_ptr(ws, 8) || need <= 0 || have < need; }

template <int ZCAP, int NSEG, bool S2>
void launch_estep(int blocks, hipStream_t s, const float* x, const float* s2, int N, const float* params, int K, int Z,
                  float* lse, int* label, double* part) {
  hipLaunchKernelGGL((estep_kernel<ZCAP, NSEG, S2>), dim3(blocks), dim3(256), 0, s, x, s2, N, params, K, Z, lse, label,
                     part);
}

}  // namespace

SVAE_EXPORT int64_t svae_gmm_params_floats(int32_t K, int32_t Z) {
  if (bad_kz(K, Z)) return 0;
  return SVAE_GMM_PARAM_FLOATS(K, Z);
}

SVAE_EXPORT int svae_gmm_geometry(int32_t N, int32_t K, int32_t Z, int32_t has_s2, int32_t* geom) {
  if (!geom || bad_shape(N, K, Z)) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z, has_s2 != 0);
  geom[0] = RB, geom[1] = g.row_blocks, geom[2] = TC, geom[3] = g.groups, geom[4] = g.rpg, geom[5] = g.segs;
  return SVAE_OK;
}

SVAE_EXPORT int svae_gmm_prepare(float* params, int32_t K, int32_t Z, svae_stream_t stream) {
  if (bad_kz(K, Z) || bad_ptr(params, 16)) return SVAE_EINVAL;
  hipLaunchKernelGGL(prepare_kernel, dim3(K), dim3(64), 0, (hipStream_t)stream, params, (int)K, (int)Z);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_gmm_estep_ws_bytes(int32_t N, int32_t K, int32_t Z) {
  if (bad_shape(N, K, Z)) return 0;
  return (int64_t)geom_of(N, K, Z, false).row_blocks * 8;
}

SVAE_EXPORT int svae_gmm_estep(const float* x, const float* s2, int32_t N, const float* params, int32_t K, int32_t Z,
                               float* lse, int32_t* label, float* resp, double* bound, void* ws, int64_t ws_bytes,
                               svae_stream_t stream) {
  if (bad_shape(N, K, Z) || bad_ptr(x, 16) || bad_opt(s2, 16) || bad_ptr(params, 16) || bad_ptr(lse, 4) ||
      bad_opt(label, 4) || bad_opt(resp, 4) || bad_ptr(bound, 8))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_gmm_estep_ws_bytes(N, K, Z))) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z, s2 != nullptr);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  const int nb = g.row_blocks;
  if (s2) {
    if (Z <= 32) launch_estep<32, 1, true>(nb, s, x, s2, N, params, K, Z, lse, label, part);
    else if (Z <= 64) launch_estep<64, 1, true>(nb, s, x, s2, N, params, K, Z, lse, label, part);
    else if (Z <= 128) launch_estep<128, 1, true>(nb, s, x, s2, N, params, K, Z, lse, label, part);
    else launch_estep<64, 4, true>(nb, s, x, s2, N, params, K, Z, lse, label, part);
  } else {
    if (Z <= 32) launch_estep<32, 1, false>(nb, s, x, s2, N, params, K, Z, lse, label, part);
    else if (Z <= 64) launch_estep<64, 1, false>(nb, s, x, s2, N, params, K, Z, lse, label, part);
    else if (Z <= 128) launch_estep<128, 1, false>(nb, s, x, s2, N, params, K, Z, lse, label, part);
    else launch_estep<256, 1, false>(nb, s, x, s2, N, params, K, Z, lse, label, part);
  }
  hipLaunchKernelGGL(estep_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part, nb, bound);
  if (resp)
    hipLaunchKernelGGL(resp_kernel, dim3((N + 255) / 256), dim3(256), 0, s, x, s2, (int)N, params, (int)K, (int)Z,
                       (const float*)lse, resp);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_gmm_mstep_ws_bytes(int32_t N, int32_t K, int32_t Z) {
  if (bad_shape(N, K, Z)) return 0;
  return ((int64_t)geom_of(N, K, Z, false).groups + 1) * K * (2 * Z + 1) * 8;
}

SVAE_EXPORT int svae_gmm_mstep(const float* x, const float* s2, int32_t N, const float* lse, const int32_t* label,
                               float* params, int32_t K, int32_t Z, float reg_covar, double* nk, void* ws,
                               int64_t ws_bytes, svae_stream_t stream) {
  if (bad_shape(N, K, Z) || bad_ptr(x, 16) || bad_opt(s2, 16) || bad_opt(lse, 4) || bad_opt(label, 4) ||
      (lse != nullptr) == (label != nullptr) || bad_ptr(params, 16) || bad_ptr(nk, 8) || !(reg_covar >= 0.f))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_gmm_mstep_ws_bytes(N, K, Z))) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z, false);
  hipStream_t s = (hipStream_t)stream;
  const long long n = (long long)K * (2 * Z + 1);
  double* part = (double*)ws;
  double* tot = part + (long long)g.groups * n;
  hipLaunchKernelGGL(mstep_stats_kernel, dim3((K + 4 * CK - 1) / (4 * CK), g.groups), dim3(256), 0, s, x, s2, (int)N, lse, label,
                     (const float*)params, (int)K, (int)Z, g.rpg, part);
  hipLaunchKernelGGL(mstep_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const double*)part,
                     g.groups, n, tot);
  hipLaunchKernelGGL(mstep_final_kernel, dim3(K), dim3(64), 0, s, (const double*)tot, params, (int)K, (int)Z, reg_covar,
                     nk);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_gmm_sample(const float* params, int32_t K, int32_t Z, int32_t n, const float* u, const float* eps,
                                uint64_t seed, float* z, int32_t* comp, svae_stream_t stream) {
  if (bad_kz(K, Z) || n < 1 || n > MAX_ROWS || bad_ptr(params, 16) || bad_opt(u, 4) || bad_opt(eps, 4) ||
      bad_ptr(z, 4) || bad_ptr(comp, 4))
    return SVAE_EINVAL;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sample_comp_kernel, dim3((n + 255) / 256), dim3(256), 0, s, params, (int)K, (int)Z, (int)n, u,
                     (unsigned long long)seed, comp);
  const long long total = (long long)n * Z;
  const long long want = (total + 255) / 256;
  const int grid = (int)(want < 4096 ? want : 4096);
  hipLaunchKernelGGL(sample_draw_kernel, dim3(grid), dim3(256), 0, s, params, (int)K, (int)Z, total, (const int*)comp,
                     eps, (unsigned long long)seed, z);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
