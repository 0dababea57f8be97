// Aggregate-posterior diagnostics: the sums behind the MMD estimators of the reference's math_utils.py:104-184
// (analytic / custom Gaussian-RBF MMD^2, the 7-scale IMQ MMD^2) and the per-dimension statistics of a latent index.
//
//   svae_pairsum:         out[p] = sum over pairs of k_p(|x_i - y_j|^2 + c_j), p < P <= 8, over the pairs i < j of one
//                         set (what pdist enumerates) or all pairs of two sets. Two launches: a (row block, column
//                         slice) grid of workgroups leaves one f64 partial per workgroup and p; one workgroup adds them.
//   svae_mmd_rowterm:     sum_i exp(-0.5 sum_j (x_ij - m_j)^2 w_j): 16 lanes per row. Two launches.
//   svae_latent_colstats: per latent dimension mean and unbiased variance of loc and the mean KL to the prior, all
//                         in f64. Two launches.
//   svae_latent_draw:     z = loc + scale * eps, eps injected or from the counter RNG.
//
// Arithmetic and summation orders (no atomics: grids and orders are functions of the shapes alone, so a result is a
// pure function of its inputs, bit for bit):
//   pairsum   d2 from direct differences: per float4 chunk of the row, d = x - y (one rounding per element), then two
//             fmaf chains, one over elements 0 and 2 and one over elements 1 and 3 of the chunks in chunk order
//             (packed f32 math: the chains are the two halves of a v_pk_fma_f32), d2 = chain A + chain B (+ the column's
//             offset). At most Z / 2 + 2 roundings on a partial sum of non-negative terms plus 2 on each square:
//             |error| <= (Z + 3) 2^-24 d2, whatever offset the rows share. The kernel function: RBF
//             exp2(fl(-a log2 e) * d2) with v_exp_f32 (one rounding of the constant, one of the product, both relative
//             to the exponent, then 1 ulp); IMQ s * rcp(s + d2) with v_rcp_f32 (sum, 1 ulp, product).
//             A lane adds the terms of ONE column tile (TJ = 32 columns) per row and p in f32, column by column; after
//             the tile each f32 sum is widened and added to the lane's f64 accumulator of that p, the lane's rows in
//             order, the tiles in column order. Workgroup: 64-lane xor butterfly in f64, the four waves in order.
//             Total: lane t adds workgroups t, t + 256, ... in order (row block major, slice minor), butterfly, waves.
//   rowterm   lane l of a row's 16 adds chunks l, l + 16, ... (elements in order, fmaf(d * d, w, q)), xor butterfly
//             over the 16 lanes, exp2(fl(-0.5 log2 e) * q); the row's value is widened to f64; a group of 16 lanes
//             adds rows g, g + 16 * grid, ... in order; workgroup and total as above.
//   colstats  every element is widened to f64 first. Row group r of a workgroup adds rows r, r + stride, ... in order;
//             the workgroup's row groups in order; the total adds the workgroups in order.
#include <math.h>

#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int TJ = SVAE_PAIRSUM_TILE_COLS;   // columns per LDS tile = the most terms an f32 accumulator ever holds
constexpr int MAXP = SVAE_PAIRSUM_MAX_P;
constexpr int MAX_ROWS = 1 << 24;
constexpr int MAX_SLICES = 64;
constexpr int TARGET_BLOCKS = 2048;          // 256 CUs x 8, as the t-SNE repulsion
constexpr int RED_BLOCKS = SVAE_MMD_REDUCE_BLOCKS;
static_assert(512 % TJ == 0 && 256 % TJ == 0, "a row block starts on a tile boundary (the triangular enumeration)");

struct PairParams {
  float v[MAXP];
};

struct PairGeom {
  int rb, row_blocks, slices, slice_cols;
};
inline int pair_rb(int Z) { return Z <= 64 ? 512 : 256; }
inline PairGeom pair_geom(int N, int M, int Z) {
  PairGeom g;
  g.rb = pair_rb(Z);
  g.row_blocks = (N + g.rb - 1) / g.rb;
  const int tiles = (M + TJ - 1) / TJ;
  int s = (TARGET_BLOCKS + g.row_blocks - 1) / g.row_blocks;
  s = s < tiles ? s : tiles;
  s = s < MAX_SLICES ? s : MAX_SLICES;
  const int tiles_per_slice = (tiles + s - 1) / s;
  g.slice_cols = tiles_per_slice * TJ;
  g.slices = (tiles + tiles_per_slice - 1) / tiles_per_slice;
  return g;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ f32x2 fma2(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }

// One tile of columns against the lane's RPL rows. CHECK: some pair of the tile is masked (a ragged edge of the rows
// or the columns, or the diagonal of the triangular set).
template <int ZCAP, int RPL, int KIND, bool CHECK>
__device__ __forceinline__ void pair_tile(const float* tile, const float* offs, int Z, int j0, int jend, int N, int tri,
                                          const f32x4 (&xi)[RPL][ZCAP / 4], const int (&ri)[RPL], const PairParams& prm,
                                          int P, float (&acc)[RPL][MAXP]) {
#pragma clang fp contract(off)
  const int zc_n = Z >> 2;
  for (int jj = 0; jj < TJ; ++jj) {
    const float* yj = tile + jj * Z;   // -y_j; the same address in every lane: a broadcast
    f32x2 s[RPL];
#pragma unroll
    for (int r = 0; r < RPL; ++r) s[r] = (f32x2){0.f, 0.f};
#pragma unroll
    for (int zc = 0; zc < ZCAP / 4; ++zc) {
      if (zc < zc_n) {   // workgroup-uniform
        const f32x4 yv = *(const f32x4*)(yj + 4 * zc);
#pragma unroll
        for (int r = 0; r < RPL; ++r) {
          const f32x4 d = xi[r][zc] + yv;   // x + (-y): fl(x - y), one rounding per element
          const f32x2 lo = {d[0], d[1]}, hi = {d[2], d[3]};
          s[r] = fma2(lo, lo, s[r]);
          s[r] = fma2(hi, hi, s[r]);
        }
      }
    }
    const float off = offs[jj];
    const int j = j0 + jj;
#pragma unroll
    for (int r = 0; r < RPL; ++r) {
      const float v = (s[r][0] + s[r][1]) + off;
      bool ok = true;
      if constexpr (CHECK) ok = j < jend && ri[r] < N && (!tri || ri[r] < j);
#pragma unroll
      for (int p = 0; p < MAXP; ++p) {
        if (p < P) {   // workgroup-uniform
          float t;
          if constexpr (KIND == SVAE_PAIR_RBF) t = __builtin_amdgcn_exp2f(prm.v[p] * v);   // v[p] = fl(-a log2 e)
          else t = prm.v[p] * __builtin_amdgcn_rcpf(prm.v[p] + v);
          if constexpr (CHECK) t = ok ? t : 0.f;
          acc[r][p] += t;
        }
      }
    }
  }
}

// grid (row blocks, slices). part f64 [row_blocks * slices][MAXP].
template <int ZCAP, int RPL, int KIND>
__global__ __launch_bounds__(256) void pairsum_kernel(const float* __restrict__ x, int N, const float* __restrict__ y,
                                                      int M, int Z, int tri, PairParams prm, int P,
                                                      const float* __restrict__ col_off, int slice_cols,
                                                      double* __restrict__ part) {
  constexpr int RB = 256 * RPL;
  __shared__ __attribute__((aligned(16))) float tile[TJ * ZCAP];
  __shared__ float offs[TJ];
  __shared__ double red[MAXP][4];
  const int tid = threadIdx.x, zc_n = Z >> 2;
  const int row0 = blockIdx.x * RB;
  int jbeg = blockIdx.y * slice_cols;
  const int jend = min(M, jbeg + slice_cols);
  // i < j: no column below the block's first row pairs with one of its rows (row0 is a multiple of the tile)
  if (tri) jbeg = max(jbeg, row0);
  f32x4 xi[RPL][ZCAP / 4];
  int ri[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    ri[r] = row0 + 256 * r + tid;
    const float* src = x + (long long)min(ri[r], N - 1) * Z;
#pragma unroll
    for (int zc = 0; zc < ZCAP / 4; ++zc) {
      if (zc < zc_n) xi[r][zc] = *(const f32x4*)(src + 4 * zc);
      else xi[r][zc] = (f32x4){0.f, 0.f, 0.f, 0.f};
    }
  }
  double acc64[MAXP];
#pragma unroll
  for (int p = 0; p < MAXP; ++p) acc64[p] = 0.0;
  for (int j0 = jbeg; j0 < jend; j0 += TJ) {
    __syncthreads();   // the previous tile has been read
    const float* src = y + (long long)j0 * Z;
    for (int v = tid; v < TJ * zc_n; v += 256) {
      const int jj = v / zc_n;
      f32x4 val = {0.f, 0.f, 0.f, 0.f};
      if (j0 + jj < M) val = -*(const f32x4*)(src + 4 * (long long)v);   // negated: x + (-y) is a v_pk_add_f32
      *(f32x4*)&tile[4 * v] = val;
    }
    if (tid < TJ) offs[tid] = (col_off && j0 + tid < M) ? col_off[j0 + tid] : 0.f;
    __syncthreads();
    float acc[RPL][MAXP];
#pragma unroll
    for (int r = 0; r < RPL; ++r)
#pragma unroll
      for (int p = 0; p < MAXP; ++p) acc[r][p] = 0.f;
    const bool check = j0 + TJ > jend || row0 + RB > N || (tri && j0 < row0 + RB);   // workgroup-uniform
    if (check) pair_tile<ZCAP, RPL, KIND, true>(tile, offs, Z, j0, jend, N, tri, xi, ri, prm, P, acc);
    else pair_tile<ZCAP, RPL, KIND, false>(tile, offs, Z, j0, jend, N, tri, xi, ri, prm, P, acc);
#pragma unroll
    for (int r = 0; r < RPL; ++r)
#pragma unroll
      for (int p = 0; p < MAXP; ++p)
        if (p < P) acc64[p] += (double)acc[r][p];
  }
#pragma unroll
  for (int p = 0; p < MAXP; ++p) {
    const double v = wave_sum_d(acc64[p]);
    if ((tid & 63) == 0) red[p][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < MAXP)
    part[((long long)blockIdx.x * gridDim.y + blockIdx.y) * MAXP + tid] =
        ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// One workgroup: out[q] = sum over i < n of part[i * stride + q], q < nq <= MAXP.
__global__ __launch_bounds__(256) void sum_parts_kernel(const double* __restrict__ part, long long n, int stride,
                                                        int nq, double* __restrict__ out) {
  __shared__ double red[MAXP][4];
  const int tid = threadIdx.x;
  for (int q = 0; q < nq; ++q) {
    double v = 0.0;
    for (long long i = tid; i < n; i += 256) v += part[i * stride + q];
    v = wave_sum_d(v);
    if ((tid & 63) == 0) red[q][tid >> 6] = v;
  }
  __syncthreads();
  if (tid < nq) out[tid] = ((red[tid][0] + red[tid][1]) + red[tid][2]) + red[tid][3];
}

// ---- rowterm -------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rowterm_kernel(const float* __restrict__ x, const float* __restrict__ m,
                                                      const float* __restrict__ w, int N, int Z,
                                                      double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[4];
  const int tid = threadIdx.x, g = tid >> 4, l = tid & 15, zc_n = Z >> 2;
  double acc = 0.0;
  for (long long row = (long long)blockIdx.x * 16 + g; row < N; row += (long long)gridDim.x * 16) {
    float q = 0.f;
    for (int c = l; c < zc_n; c += 16) {
      const f32x4 xv = *(const f32x4*)(x + row * Z + 4 * c);
      const f32x4 mv = m ? *(const f32x4*)(m + 4 * c) : (f32x4){0.f, 0.f, 0.f, 0.f};
      const f32x4 wv = *(const f32x4*)(w + 4 * c);
      const f32x4 d = xv - mv;
#pragma unroll
      for (int e = 0; e < 4; ++e) q = fmaf(d[e] * d[e], wv[e], q);
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);   // the row's 16 lanes leave the loop together
    const float t = __builtin_amdgcn_exp2f(-0.72134752044448170f * q);   // -0.5 log2 e
    if (l == 0) acc += (double)t;
  }
  const double v = wave_sum_d(acc);
  if ((tid & 63) == 0) red[tid >> 6] = v;
  __syncthreads();
  if (tid == 0) part[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// ---- colstats ------------------------------------------------------------------------------------------------------
// A thread owns one float4 chunk of the columns for one of the workgroup's 256 / (Z / 4) row groups.
// part f64 [blocks][3][Z]: sum (loc - loc[0]), sum (loc - loc[0])^2, sum KL.
__global__ __launch_bounds__(256) void colstats_kernel(const float* __restrict__ loc, const float* __restrict__ scale,
                                                       int N, int Z, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double sm[256][12];
  const int tid = threadIdx.x, zc_n = Z >> 2, rpi = 256 / zc_n;
  const int c = tid % zc_n, rl = tid / zc_n;
  double s1[4], s2[4], sk[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) s1[e] = s2[e] = sk[e] = 0.0;
  if (rl < rpi) {
    const f32x4 k0 = *(const f32x4*)(loc + 4 * c);
    for (long long row = (long long)blockIdx.x * rpi + rl; row < N; row += (long long)gridDim.x * rpi) {
      const f32x4 mu = *(const f32x4*)(loc + row * Z + 4 * c);
      const f32x4 sg = *(const f32x4*)(scale + row * Z + 4 * c);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const double d = (double)mu[e] - (double)k0[e];
        s1[e] += d;
        s2[e] = fma(d, d, s2[e]);
        const double mm = (double)mu[e], var = (double)sg[e] * (double)sg[e];
        sk[e] += 0.5 * (((mm * mm + var) - 1.0) - log(var));
      }
    }
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    sm[tid][e] = s1[e];
    sm[tid][4 + e] = s2[e];
    sm[tid][8 + e] = sk[e];
  }
  __syncthreads();
  for (int idx = tid; idx < 3 * Z; idx += 256) {
    const int q = idx / Z, col = idx - q * Z;
    double v = 0.0;
    for (int r = 0; r < rpi; ++r) v += sm[r * zc_n + (col >> 2)][4 * q + (col & 3)];
    part[((long long)blockIdx.x * 3 + q) * Z + col] = v;
  }
}

__global__ __launch_bounds__(256) void colstats_final_kernel(const double* __restrict__ part, int blocks,
                                                             const float* __restrict__ loc, int N, int Z,
                                                             double* __restrict__ mean_loc, double* __restrict__ var_loc,
                                                             double* __restrict__ mean_kl) {
#pragma clang fp contract(off)
  const int col = threadIdx.x;
  if (col >= Z) return;
  double s[3] = {0.0, 0.0, 0.0};
  for (int b = 0; b < blocks; ++b)
#pragma unroll
    for (int q = 0; q < 3; ++q) s[q] += part[((long long)b * 3 + q) * Z + col];
  const double n = (double)N;
  mean_loc[col] = (double)loc[col] + s[0] / n;
  var_loc[col] = (s[1] - s[0] * s[0] / n) / (n - 1.0);   // N = 1: 0 / 0
  mean_kl[col] = s[2] / n;
}

// ---- draw ----------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void latent_draw_kernel(const float* __restrict__ loc, const float* __restrict__ scale,
                                                          const float* __restrict__ eps, unsigned long long seed,
                                                          long long n, float* __restrict__ z) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
    float e;
    if (eps) {
      e = eps[i];
    } else {
      const unsigned long long idx = 2ull * (unsigned long long)i;   // i = row * Z + column
      const float u1 = rand_uniform(seed, idx), u2 = rand_uniform(seed, idx + 1);
      e = sqrtf(-2.f * __logf(u1)) * __cosf(6.283185307179586f * u2);
    }
    z[i] = fmaf(scale[i], e, loc[i]);
  }
}

bool bad_rows(const void* p, int32_t rows, int32_t Z) {
  return !p || ((uintptr_t)p & 15) || rows < 1 || rows > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3);
}
bool bad_pair_shape(int32_t N, int32_t M, int32_t Z, int32_t tri) {
  if (N < 1 || N > MAX_ROWS || M < 1 || M > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3)) return true;
  return tri && (N < 2 || M != N);
}
bool bad_ws(const void* ws, int64_t have, int64_t need) { return !ws || ((uintptr_t)ws & 7) || need <= 0 || have < need; }

template <int ZCAP, int RPL>
void launch_pairsum(int kind, dim3 grid, hipStream_t s, const float* x, int N, const float* y, int M, int Z, int tri,
                    const PairParams& prm, int P, const float* col_off, int slice_cols, double* part) {
  if (kind == SVAE_PAIR_RBF)
    hipLaunchKernelGGL((pairsum_kernel<ZCAP, RPL, SVAE_PAIR_RBF>), grid, dim3(256), 0, s, x, N, y, M, Z, tri, prm, P,
                       col_off, slice_cols, part);
  else
    hipLaunchKernelGGL((pairsum_kernel<ZCAP, RPL, SVAE_PAIR_IMQ>), grid, dim3(256), 0, s, x, N, y, M, Z, tri, prm, P,
                       col_off, slice_cols, part);
}

}  // namespace

SVAE_EXPORT int svae_pairsum_geometry(int32_t N, int32_t M, int32_t Z, int32_t triangular, int32_t* geom) {
  if (!geom || bad_pair_shape(N, M, Z, triangular)) return SVAE_EINVAL;
  const PairGeom g = pair_geom(N, M, Z);
  geom[0] = g.rb, geom[1] = g.row_blocks, geom[2] = g.slices, geom[3] = g.slice_cols, geom[4] = TJ;
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_pairsum_ws_bytes(int32_t N, int32_t M, int32_t Z, int32_t triangular) {
  if (bad_pair_shape(N, M, Z, triangular)) return 0;
  const PairGeom g = pair_geom(N, M, Z);
  return (int64_t)g.row_blocks * g.slices * MAXP * (int64_t)sizeof(double);
}

SVAE_EXPORT int svae_pairsum(const float* x, int32_t N, const float* y, int32_t M, int32_t Z, int32_t triangular,
                             int32_t kind, const float* params, int32_t P, const float* col_off, void* ws,
                             int64_t ws_bytes, double* out, svae_stream_t stream) {
  if (!params || !out || P < 1 || P > MAXP || (kind != SVAE_PAIR_RBF && kind != SVAE_PAIR_IMQ)) return SVAE_EINVAL;
  if (bad_pair_shape(N, M, Z, triangular) || bad_rows(x, N, Z)) return SVAE_EINVAL;
  if (triangular) {
    if (col_off || (y && y != x)) return SVAE_EINVAL;
    y = x;
  } else if (bad_rows(y, M, Z)) {
    return SVAE_EINVAL;
  }
  if (bad_ws(ws, ws_bytes, svae_pairsum_ws_bytes(N, M, Z, triangular))) return SVAE_EINVAL;
  PairParams prm;
  for (int p = 0; p < MAXP; ++p) {
    const float a = p < P ? params[p] : 1.0f;
    if (kind == SVAE_PAIR_RBF) {
      if (!(a >= 0.f) || !(a < INFINITY)) return SVAE_EINVAL;
      prm.v[p] = (float)(-(double)a * 1.4426950408889634);   // one rounding of -a log2 e
    } else {
      if (!(a > 0.f) || !(a < INFINITY)) return SVAE_EINVAL;
      prm.v[p] = a;
    }
  }
  const PairGeom g = pair_geom(N, M, Z);
  const dim3 grid(g.row_blocks, g.slices);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  const int tri = triangular ? 1 : 0;
  if (Z <= 32) launch_pairsum<32, 2>(kind, grid, s, x, N, y, M, Z, tri, prm, P, col_off, g.slice_cols, part);
  else if (Z <= 64) launch_pairsum<64, 2>(kind, grid, s, x, N, y, M, Z, tri, prm, P, col_off, g.slice_cols, part);
  else if (Z <= 128) launch_pairsum<128, 1>(kind, grid, s, x, N, y, M, Z, tri, prm, P, col_off, g.slice_cols, part);
  else launch_pairsum<256, 1>(kind, grid, s, x, N, y, M, Z, tri, prm, P, col_off, g.slice_cols, part);
  hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, s, (const double*)part,
                     (long long)g.row_blocks * g.slices, MAXP, (int)P, out);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_mmd_rowterm_ws_bytes(int32_t N) {
  if (N < 1 || N > MAX_ROWS) return 0;
  const int blocks = (N + 15) / 16 < RED_BLOCKS ? (N + 15) / 16 : RED_BLOCKS;
  return (int64_t)blocks * (int64_t)sizeof(double);
}

SVAE_EXPORT int svae_mmd_rowterm(const float* x, const float* m, const float* w, int32_t N, int32_t Z, void* ws,
                                 int64_t ws_bytes, double* out, svae_stream_t stream) {
  if (bad_rows(x, N, Z) || !w || ((uintptr_t)w & 15) || ((uintptr_t)m & 15) || !out) return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_mmd_rowterm_ws_bytes(N))) return SVAE_EINVAL;
  const int blocks = (int)(svae_mmd_rowterm_ws_bytes(N) / (int64_t)sizeof(double));
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(rowterm_kernel, dim3(blocks), dim3(256), 0, s, x, m, w, (int)N, (int)Z, (double*)ws);
  hipLaunchKernelGGL(sum_parts_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, (long long)blocks, 1, 1, out);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

static int colstats_blocks(int32_t N, int32_t Z) {
  const int rpi = 256 / (Z >> 2);
  const int b = (N + rpi - 1) / rpi;
  return b < RED_BLOCKS ? b : RED_BLOCKS;
}

SVAE_EXPORT int64_t svae_latent_colstats_ws_bytes(int32_t N, int32_t Z) {
  if (N < 1 || N > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3)) return 0;
  return (int64_t)colstats_blocks(N, Z) * 3 * Z * (int64_t)sizeof(double);
}

SVAE_EXPORT int svae_latent_colstats(const float* loc, const float* scale, int32_t N, int32_t Z, void* ws,
                                     int64_t ws_bytes, double* mean_loc, double* var_loc, double* mean_kl,
                                     svae_stream_t stream) {
  if (bad_rows(loc, N, Z) || bad_rows(scale, N, Z) || !mean_loc || !var_loc || !mean_kl) return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_latent_colstats_ws_bytes(N, Z))) return SVAE_EINVAL;
  const int blocks = colstats_blocks(N, Z);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(colstats_kernel, dim3(blocks), dim3(256), 0, s, loc, scale, (int)N, (int)Z, (double*)ws);
  hipLaunchKernelGGL(colstats_final_kernel, dim3(1), dim3(256), 0, s, (const double*)ws, blocks, loc, (int)N, (int)Z,
                     mean_loc, var_loc, mean_kl);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_latent_draw(const float* loc, const float* scale, const float* eps, uint64_t seed, int32_t N,
                                 int32_t Z, float* z, svae_stream_t stream) {
  if (bad_rows(loc, N, Z) || bad_rows(scale, N, Z) || !z) return SVAE_EINVAL;
  const long long n = (long long)N * Z;
  const int grid = (int)min((long long)2048, (n + 255) / 256);
  hipLaunchKernelGGL(latent_draw_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, loc, scale, eps,
                     (unsigned long long)seed, n, z);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
