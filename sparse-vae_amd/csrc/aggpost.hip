// ELBO surgery of the latent index: the log-density of the aggregate posterior q(z) = (1 / N) sum_j q(z | x_j) at M
// points against all N rows of the index, jointly and per latent dimension, and the decomposition of the mean KL built
// on it (Hoffman & Johnson 2016; Chen et al. 2018). It is the corpus-level form of marginal_kl (math_utils.py:51-58 of
// the reference), which estimates the same split inside one batch and so cannot exceed log B.
//
//   svae_aggpost_logq:      logq_i = logsumexp_j l_ij - log n_i and, optionally, logq_dim_id = logsumexp_j l_ijd - log n_i,
//                           an M x N x Z streaming log-sum-exp. A workgroup owns 256 points (one per lane, in registers)
//                           and one slice of the rows, which it streams through LDS in tiles of 16 rows; it leaves a
//                           (max, sum) partial per point (and per (point, dimension)); a second kernel merges the slices.
//   svae_aggpost_decompose: the f64 means behind {mi, marginal_kl, tc, kl_mc, dim_kl[Z]}: per-block partials, one reduce.
//
// No atomics: grids and orders are functions of (M, N, Z) alone, so a result is a pure function of its inputs, bit for
// bit. No |z|^2 - 2 z.mu + |mu|^2 expansion: every term is formed from the direct difference z - loc, so it keeps its
// digits where scale is small. Arithmetic and orders (contraction is off, the FMAs are written out):
//   staged    per element of a row tile, once per tile on load: w = 1.f / scale (IEEE division, one rounding) and
//             logf(scale) (the library's, 1 ulp).
//   joint     l_ij = fmaf(-0.5, q, c_j). q: per float4 chunk of the row d = z - loc, t = d * w (one rounding each), then
//             two fmaf chains acc = fmaf(t, t, acc), one over elements 0 and 2 and one over elements 1 and 3 of the
//             chunks in chunk order (the two halves of a v_pk_fma_f32), q = chain A + chain B. c_j = (float)(-(sum_d
//             (double)logf(scale_jd)) - Z * 0.5 log 2 pi): 16 lanes per row add the dimensions p, p + 16, ... in f64,
//             an xor butterfly over the 16, one rounding.
//             |error| <= ((Z / 2 + 7) q / 2 + 2 sum_d |log scale_jd| + |c_j| + |l_ij|) 2^-24 to first order.
//   per dim   l_ijd = fmaf(-0.5f * t, t, nc) (the product by -0.5 is exact), nc = -(logf(scale) + 0.9189385f) in f32.
//             |error| <= (3 t^2 + 3 |log scale| + 2 * 0.919 + |l_ijd|) 2^-24 to first order.
//   lse       a lane carries (Mx, S) per output over its slice. Mx (f32) starts at -1e38, a finite floor below every
//             term, so the loop meets neither NaN nor -inf; S (f64) starts at 0. Per tile: s (f32) = 0, M0 = Mx; per
//             row in order Mn = max(Mx, l), s = fmaf(s, ex(Mx - Mn), ex(l - Mn)), Mx = Mn with ex(x) =
//             v_exp_f32(x * 1.442695f) (one of the two arguments is always 0, and ex(0) = 1 exactly); a skipped row
//             leaves Mx alone and adds 0. After the tile S = S + s where Mx == M0, else S = S * exp((double)M0 -
//             (double)Mx) + s in f64 (the library's exp). So f32 sums span at most 16 terms, and everything carried
//             across tiles is f64. Requires every l finite (|(z - loc) / scale| < 2^63).
//   merge     the slices in ascending order, in f64: Mt = max_s Mx_s, St = sum_s S_s exp(Mx_s - Mt), a slice with
//             (-inf, 0) (all its rows skipped) left out so that -inf - (-inf) is never formed; the output is
//             (float)(Mt + log St - log n_i), one rounding.
//   decompose every term in f64 from the f32 operands; a thread adds its points i = t, t + stride, ... in order, then a
//             64-lane xor butterfly and the four waves in order; dim_kl: thread d adds the workgroup's points in
//             ascending order; the reduce adds the workgroups in ascending order and divides by M.
#include <math.h>

#include <type_traits>

#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int PB = SVAE_AGGPOST_POINTS_PER_BLOCK;   // points per workgroup, one per lane
constexpr int TR = SVAE_AGGPOST_TILE_ROWS;          // rows per LDS tile
constexpr int ZP = SVAE_AGGPOST_PASS_DIMS;          // dimensions a per-dimension workgroup holds
constexpr int TARGET_WG = 1024;                     // (point block, slice) workgroups aimed at: 256 CUs x 4
constexpr int MIN_SLICE_ROWS = 64;
constexpr int DEC_BLOCKS = 1024;                    // decompose: at most this many workgroups
constexpr int MAX_ROWS = 1 << 24;
constexpr float FLOOR = -1.0e38f;
constexpr float LOG2E = 1.44269504f;
constexpr double HALF_LOG_2PI = 0.918938533204672741780;
static_assert(PB == 256 && TR == 16 && ZP == 16, "geometry");

struct __attribute__((aligned(16))) Partial {
  double mx, sum;
};

__device__ __forceinline__ float ex(float x) {
#pragma clang fp contract(off)
  return __builtin_amdgcn_exp2f(x * LOG2E);
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// After a tile: the tile's f32 sum s (relative to mx) joins the carried f64 sum S (relative to m0 <= mx).
__device__ __forceinline__ void fold(double& S, float m0, float mx, float s) {
  if (mx == m0) S += (double)s;
  else S = S * exp((double)m0 - (double)mx) + (double)s;
}

// ---- joint: logsumexp_j sum_d l_ijd -------------------------------------------------------------------------------
// grid (point blocks, slices). part [slices][M].
template <int ZCAP>
__global__ __launch_bounds__(256) void joint_kernel(const float* __restrict__ z, int M, const float* __restrict__ loc,
                                                    const float* __restrict__ scale, int N, int Z,
                                                    const int* __restrict__ skip, int rps, Partial* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int CH = ZCAP / 4;
  __shared__ __attribute__((aligned(16))) float tloc[TR * ZCAP];
  __shared__ __attribute__((aligned(16))) float tw[TR * ZCAP];
  __shared__ __attribute__((aligned(16))) float tl[TR * ZCAP];
  __shared__ float tc[TR];
  const int tid = threadIdx.x, zc_n = Z >> 2;
  const int i = blockIdx.x * PB + tid;
  const long long off = (long long)min(i, M - 1) * Z;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 zi[CH];
#pragma unroll
  for (int zc = 0; zc < CH; ++zc) zi[zc] = zc < zc_n ? *(const f32x4*)(z + off + 4 * zc) : zero;
  const int sk = skip ? skip[min(i, M - 1)] : -1;
  const int r0 = blockIdx.y * rps, r1 = min(N, r0 + rps);
  float mx = FLOOR;
  double S = 0.0;
  for (int j0 = r0; j0 < r1; j0 += TR) {
    const int nr = min(TR, r1 - j0);   // workgroup-uniform
    __syncthreads();                   // the previous tile has been read
    for (int v = tid; v < nr * zc_n; v += 256) {   // the tile is nr * Z consecutive floats
      const f32x4 sv = *(const f32x4*)(scale + (long long)j0 * Z + 4 * v);
      *(f32x4*)&tloc[4 * v] = *(const f32x4*)(loc + (long long)j0 * Z + 4 * v);
      *(f32x4*)&tw[4 * v] = (f32x4){1.f / sv[0], 1.f / sv[1], 1.f / sv[2], 1.f / sv[3]};
      *(f32x4*)&tl[4 * v] = (f32x4){logf(sv[0]), logf(sv[1]), logf(sv[2]), logf(sv[3])};
    }
    __syncthreads();
    {   // c_j: 16 lanes per row
      const int r = tid >> 4, p = tid & 15;
      double a = 0.0;
      if (r < nr)
        for (int d = p; d < Z; d += 16) a += (double)tl[r * Z + d];
#pragma unroll
      for (int o = 8; o > 0; o >>= 1) a += __shfl_xor(a, o, 64);
      if (p == 0 && r < nr) tc[r] = (float)(-a - (double)Z * HALF_LOG_2PI);
    }
    __syncthreads();
    const float m0 = mx;
    float s = 0.f;
    auto rows = [&](auto has_skip) {
      for (int jj = 0; jj < nr; ++jj) {
        const float* lj = tloc + jj * Z;   // the same address in every lane: a broadcast
        const float* wj = tw + jj * Z;
        f32x2 acc = {0.f, 0.f};
#pragma unroll
        for (int zc = 0; zc < CH; ++zc) {
          if (zc < zc_n) {   // workgroup-uniform
            const f32x4 d = zi[zc] - *(const f32x4*)(lj + 4 * zc);
            const f32x4 t = d * *(const f32x4*)(wj + 4 * zc);
            const f32x2 tlo = {t[0], t[1]}, thi = {t[2], t[3]};
            acc = __builtin_elementwise_fma(tlo, tlo, acc);
            acc = __builtin_elementwise_fma(thi, thi, acc);
          }
        }
        float l = fmaf(-0.5f, acc[0] + acc[1], tc[jj]);
        float one = 1.f;
        if constexpr (decltype(has_skip)::value) {
          const bool live = j0 + jj != sk;
          l = live ? l : mx;
          one = live ? 1.f : 0.f;
        }
        const float mn = fmaxf(mx, l);
        s = fmaf(s, ex(mx - mn), one * ex(l - mn));
        mx = mn;
      }
    };
    if (__ballot(sk >= j0 && sk < j0 + nr)) rows(std::true_type{});   // wave-uniform
    else rows(std::false_type{});
    fold(S, m0, mx, s);
  }
  if (i < M) {
    Partial p;
    p.mx = S > 0.0 ? (double)mx : -INFINITY;
    p.sum = S;
    part[(long long)blockIdx.y * M + i] = p;
  }
}

// ---- per dimension: logsumexp_j l_ijd, ZP dimensions per workgroup ------------------------------------------------
// grid (point blocks, slices, dimension passes). part [slices][M][Z].
__global__ __launch_bounds__(256) void dim_kernel(const float* __restrict__ z, int M, const float* __restrict__ loc,
                                                  const float* __restrict__ scale, int N, int Z,
                                                  const int* __restrict__ skip, int rps, Partial* __restrict__ part) {
#pragma clang fp contract(off)
  constexpr int CH = ZP / 4;
  __shared__ __attribute__((aligned(16))) float tloc[TR * ZP];
  __shared__ __attribute__((aligned(16))) float tw[TR * ZP];
  __shared__ __attribute__((aligned(16))) float tn[TR * ZP];
  const int tid = threadIdx.x;
  const int d0 = blockIdx.z * ZP, nch = min(ZP, Z - d0) >> 2;   // this pass's dimensions, in float4 chunks
  const int i = blockIdx.x * PB + tid;
  const long long off = (long long)min(i, M - 1) * Z + d0;
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 zi[CH], mx[CH];
  double S[CH][4];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    zi[c] = c < nch ? *(const f32x4*)(z + off + 4 * c) : zero;
    mx[c] = (f32x4){FLOOR, FLOOR, FLOOR, FLOOR};
#pragma unroll
    for (int e = 0; e < 4; ++e) S[c][e] = 0.0;
  }
  const int sk = skip ? skip[min(i, M - 1)] : -1;
  const int r0 = blockIdx.y * rps, r1 = min(N, r0 + rps);
  const float cf = (float)HALF_LOG_2PI;
  for (int j0 = r0; j0 < r1; j0 += TR) {
    const int nr = min(TR, r1 - j0);   // workgroup-uniform
    __syncthreads();                   // the previous tile has been read
    for (int v = tid; v < nr * nch; v += 256) {
      const int r = v / nch, c = v - r * nch;
      const long long g = (long long)(j0 + r) * Z + d0 + 4 * c;
      const f32x4 sv = *(const f32x4*)(scale + g);
      *(f32x4*)&tloc[r * ZP + 4 * c] = *(const f32x4*)(loc + g);
      *(f32x4*)&tw[r * ZP + 4 * c] = (f32x4){1.f / sv[0], 1.f / sv[1], 1.f / sv[2], 1.f / sv[3]};
      *(f32x4*)&tn[r * ZP + 4 * c] =
          (f32x4){-(logf(sv[0]) + cf), -(logf(sv[1]) + cf), -(logf(sv[2]) + cf), -(logf(sv[3]) + cf)};
    }
    __syncthreads();
    auto rows = [&](auto has_skip) {
#pragma unroll
      for (int c = 0; c < CH; ++c) {
        if (c < nch) {   // workgroup-uniform
          const f32x4 m0 = mx[c];
          f32x4 m = m0, s = zero;
          for (int jj = 0; jj < nr; ++jj) {
            const f32x4 d = zi[c] - *(const f32x4*)&tloc[jj * ZP + 4 * c];   // broadcast reads
            const f32x4 t = d * *(const f32x4*)&tw[jj * ZP + 4 * c];
            const f32x4 h = t * -0.5f;
            f32x4 l = __builtin_elementwise_fma(h, t, *(const f32x4*)&tn[jj * ZP + 4 * c]);
            float one = 1.f;
            if constexpr (decltype(has_skip)::value) {
              const bool live = j0 + jj != sk;
              l = live ? l : m;
              one = live ? 1.f : 0.f;
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              const float mn = fmaxf(m[e], l[e]);
              s[e] = fmaf(s[e], ex(m[e] - mn), one * ex(l[e] - mn));
              m[e] = mn;
            }
          }
          mx[c] = m;
#pragma unroll
          for (int e = 0; e < 4; ++e) fold(S[c][e], m0[e], m[e], s[e]);
        }
      }
    };
    if (__ballot(sk >= j0 && sk < j0 + nr)) rows(std::true_type{});   // wave-uniform
    else rows(std::false_type{});
  }
  if (i < M) {
    Partial* out = part + ((long long)blockIdx.y * M + i) * Z + d0;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (c < nch) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          Partial p;
          p.mx = S[c][e] > 0.0 ? (double)mx[c][e] : -INFINITY;
          p.sum = S[c][e];
          out[4 * c + e] = p;
        }
      }
    }
  }
}

// One thread per output: the slices in ascending order. per = 1 (joint) or Z (per dimension) outputs per point.
__global__ __launch_bounds__(256) void merge_kernel(const Partial* __restrict__ part, long long cnt, int slices, int per,
                                                    const int* __restrict__ skip, int N, float* __restrict__ out) {
  const long long o = (long long)blockIdx.x * 256 + threadIdx.x;
  if (o >= cnt) return;
  double mt = -INFINITY;
  for (int s = 0; s < slices; ++s) mt = fmax(mt, part[(long long)s * cnt + o].mx);
  double st = 0.0;
  for (int s = 0; s < slices; ++s) {
    const Partial p = part[(long long)s * cnt + o];
    if (p.mx != -INFINITY) st += p.sum * exp(p.mx - mt);
  }
  int n = N;
  if (skip) {
    const int sk = skip[o / per];
    n -= sk >= 0 && sk < N ? 1 : 0;
  }
  out[o] = (float)(mt + log(st) - log((double)n));
}

// ---- decompose -----------------------------------------------------------------------------------------------------
// part f64 [blocks][3 + Z] = the workgroup's sums of {log q(z|x) - logq, logq - log p, logq - sum_d logq_dim, and per
// dimension logq_dim - log p_d}.
__global__ __launch_bounds__(256) void decomp_block_kernel(const float* __restrict__ z, const int* __restrict__ src,
                                                           const float* __restrict__ loc,
                                                           const float* __restrict__ scale,
                                                           const float* __restrict__ logq,
                                                           const float* __restrict__ logq_dim, int M, int Z,
                                                           double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[3][4];
  const int tid = threadIdx.x, stride = gridDim.x * 256;
  double a = 0.0, b = 0.0, c = 0.0;
  for (int i = blockIdx.x * 256 + tid; i < M; i += stride) {
    const float* zr = z + (long long)i * Z;
    const float* lr = loc + (long long)src[i] * Z;
    const float* sr = scale + (long long)src[i] * Z;
    const float* qr = logq_dim + (long long)i * Z;
    double cond = 0.0, lp = 0.0, sd = 0.0;
    for (int d = 0; d < Z; ++d) {
      const double zv = (double)zr[d], sv = (double)sr[d], t = (zv - (double)lr[d]) / sv;
      cond += -0.5 * t * t - log(sv) - HALF_LOG_2PI;
      lp += -0.5 * zv * zv - HALF_LOG_2PI;
      sd += (double)qr[d];
    }
    const double lq = (double)logq[i];
    a += cond - lq;
    b += lq - lp;
    c += lq - sd;
  }
  a = wave_sum_d(a), b = wave_sum_d(b), c = wave_sum_d(c);
  if ((tid & 63) == 0) red[0][tid >> 6] = a, red[1][tid >> 6] = b, red[2][tid >> 6] = c;
  __syncthreads();
  double* out = part + (long long)blockIdx.x * (3 + Z);
  if (tid < 3) out[tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
  if (tid < Z) {
    double s = 0.0;
    for (int b0 = blockIdx.x * 256; b0 < M; b0 += stride) {
      const int e = min(M, b0 + 256);
      for (int i = b0; i < e; ++i) {
        const double zv = (double)z[(long long)i * Z + tid];
        s += (double)logq_dim[(long long)i * Z + tid] - (-0.5 * zv * zv - HALF_LOG_2PI);
      }
    }
    out[3 + tid] = s;
  }
}

// One workgroup: out f64 [4 + Z] = {mi, marginal_kl, tc, kl_mc, dim_kl[Z]}.
__global__ __launch_bounds__(256) void decomp_final_kernel(const double* __restrict__ part, int blocks, int M, int Z,
                                                           double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double head[2];
  for (int t = threadIdx.x; t < 3 + Z; t += 256) {
    double s = 0.0;
    for (int b = 0; b < blocks; ++b) s += part[(long long)b * (3 + Z) + t];
    const double v = s / (double)M;
    out[t < 3 ? t : t + 1] = v;
    if (t < 2) head[t] = v;
  }
  __syncthreads();
  if (threadIdx.x == 0) out[3] = head[0] + head[1];
}

// ---- host ----------------------------------------------------------------------------------------------------------
struct Geom {
  int point_blocks, slices, rps, passes;
};
bool bad_shape(int32_t M, int32_t N, int32_t Z) {
  return M < 1 || M > MAX_ROWS || N < 1 || N > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3);
}
Geom geom_of(int M, int N, int Z) {
  Geom g;
  g.point_blocks = (M + PB - 1) / PB;
  const int want = g.point_blocks >= TARGET_WG ? 1 : (TARGET_WG + g.point_blocks - 1) / g.point_blocks;
  int per = (N + want - 1) / want;
  per = per < MIN_SLICE_ROWS ? MIN_SLICE_ROWS : per;
  g.rps = (per + TR - 1) / TR * TR;
  g.slices = (N + g.rps - 1) / g.rps;
  g.passes = (Z + ZP - 1) / ZP;
  return g;
}
bool bad_ptr(const void* p, int align) { return !p || ((uintptr_t)p & (uintptr_t)(align - 1)); }
bool bad_opt(const void* p, int align) { return ((uintptr_t)p & (uintptr_t)(align - 1)) != 0; }
bool bad_ws(const void* ws, int64_t have, int64_t need) { return bad_ptr(ws, 16) || need <= 0 || have < need; }
int dec_blocks(int M) {
  const int b = (M + 255) / 256;
  return b < DEC_BLOCKS ? b : DEC_BLOCKS;
}

template <int ZCAP>
void launch_joint(dim3 grid, hipStream_t s, const float* z, int M, const float* loc, const float* scale, int N, int Z,
                  const int* skip, int rps, Partial* part) {
  hipLaunchKernelGGL((joint_kernel<ZCAP>), grid, dim3(256), 0, s, z, M, loc, scale, N, Z, skip, rps, part);
}

}  // namespace

SVAE_EXPORT int svae_aggpost_geometry(int32_t M, int32_t N, int32_t Z, int32_t per_dim, int32_t* geom) {
  if (!geom || bad_shape(M, N, Z)) return SVAE_EINVAL;
  const Geom g = geom_of(M, N, Z);
  geom[0] = PB, geom[1] = g.point_blocks, geom[2] = g.slices, geom[3] = g.rps, geom[4] = TR;
  geom[5] = per_dim ? (Z < ZP ? Z : ZP) : Z;
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_aggpost_ws_bytes(int32_t M, int32_t N, int32_t Z, int32_t per_dim) {
  if (bad_shape(M, N, Z)) return 0;
  const Geom g = geom_of(M, N, Z);
  return (int64_t)g.slices * M * (per_dim ? 1 + Z : 1) * (int64_t)sizeof(Partial);
}

SVAE_EXPORT int svae_aggpost_logq(const float* z, int32_t M, const float* loc, const float* scale, int32_t N, int32_t Z,
                                  const int32_t* skip, float* logq, float* logq_dim, void* ws, int64_t ws_bytes,
                                  svae_stream_t stream) {
  if (bad_shape(M, N, Z) || bad_ptr(z, 16) || bad_ptr(loc, 16) || bad_ptr(scale, 16) || bad_opt(skip, 4) ||
      bad_ptr(logq, 4) || bad_opt(logq_dim, 4) || (skip && N < 2))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_aggpost_ws_bytes(M, N, Z, logq_dim != nullptr))) return SVAE_EINVAL;
  const Geom g = geom_of(M, N, Z);
  hipStream_t s = (hipStream_t)stream;
  Partial* pj = (Partial*)ws;
  Partial* pd = pj + (long long)g.slices * M;
  const dim3 grid(g.point_blocks, g.slices);
  if (Z <= 32) launch_joint<32>(grid, s, z, M, loc, scale, N, Z, skip, g.rps, pj);
  else if (Z <= 64) launch_joint<64>(grid, s, z, M, loc, scale, N, Z, skip, g.rps, pj);
  else if (Z <= 128) launch_joint<128>(grid, s, z, M, loc, scale, N, Z, skip, g.rps, pj);
  else launch_joint<256>(grid, s, z, M, loc, scale, N, Z, skip, g.rps, pj);
  hipLaunchKernelGGL(merge_kernel, dim3((M + 255) / 256), dim3(256), 0, s, (const Partial*)pj, (long long)M, g.slices,
                     1, skip, (int)N, logq);
  if (logq_dim) {
    hipLaunchKernelGGL(dim_kernel, dim3(g.point_blocks, g.slices, g.passes), dim3(256), 0, s, z, (int)M, loc, scale,
                       (int)N, (int)Z, skip, g.rps, pd);
    const long long cnt = (long long)M * Z;
    hipLaunchKernelGGL(merge_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, s, (const Partial*)pd, cnt,
                       g.slices, (int)Z, skip, (int)N, logq_dim);
  }
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_aggpost_decompose_ws_bytes(int32_t M, int32_t Z) {
  if (M < 1 || M > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3)) return 0;
  return (int64_t)dec_blocks(M) * (3 + Z) * (int64_t)sizeof(double);
}

SVAE_EXPORT int svae_aggpost_decompose(const float* z, const int32_t* src, const float* loc, const float* scale,
                                       const float* logq, const float* logq_dim, int32_t M, int32_t Z, void* ws,
                                       int64_t ws_bytes, double* out, svae_stream_t stream) {
  if (M < 1 || M > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3) || bad_ptr(z, 16) || bad_ptr(src, 4) || bad_ptr(loc, 16) ||
      bad_ptr(scale, 16) || bad_ptr(logq, 4) || bad_ptr(logq_dim, 4) || bad_ptr(out, 8))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_aggpost_decompose_ws_bytes(M, Z))) return SVAE_EINVAL;
  const int blocks = dec_blocks(M);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(decomp_block_kernel, dim3(blocks), dim3(256), 0, s, z, src, loc, scale, logq, logq_dim, (int)M,
                     (int)Z, (double*)ws);
  hipLaunchKernelGGL(decomp_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, blocks, (int)M, (int)Z, out);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
