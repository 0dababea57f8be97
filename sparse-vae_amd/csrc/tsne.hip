// Exact t-SNE of the latent index in two output dimensions (the reference's tsne.py:16-30, where the embedding is
// tsnecuda's, or sklearn.manifold.TSNE on the CPU when there is no CUDA device).
//
//   svae_tsne_affinities: per row of the k-NN graph, the perplexity-calibrated conditional p_{j|i} (bisection on the
//                         precision beta with sklearn's _binary_search_perplexity constants). One wave per row, one
//                         lane per neighbour.
//   svae_tsne_repulse:    the exact all-pairs Student-t repulsion, rep_i = sum_{j != i} q_ij^2 (y_i - y_j), with the
//                         row sums zrow_i = sum_{j != i} q_ij and their total zsum. Three launches: (rows, column
//                         slices) partials, the per-row sum over the slices, the total.
//   svae_tsne_attract:    the attraction over the k-NN edges, both directions of the symmetrised affinity from the
//                         one conditional p: a row's own edges and, through the reverse lists, the edges that point
//                         at it. One wave per row.
//   svae_tsne_update:     gradient, per-coordinate gains, momentum step, in place.
//
// Summation orders (nothing here uses an atomic, so every result is a pure function of its inputs):
//   affinities  64-lane xor butterflies over the row's k values padded with zeros: the order depends on k alone.
//   repulse     a row's terms are added column by column inside a slice (one accumulator per row, a lane owns the
//               row), the slices in slice order, zrow -> zsum in f64 (256-row workgroup sums by butterfly + four
//               wave sums in order, then one workgroup over those): N and the constants below decide everything.
//   attract     lane l adds the row's edges l, l + 64, ... (its own k first, then its reverse list in list order),
//               then a butterfly: k and the row's in-degree decide.
#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int RPL = 2;                              // rows per lane of the repulsion
constexpr int RB = SVAE_TSNE_ROWS_PER_BLOCK;        // rows per repulsion workgroup
constexpr int TJ = SVAE_TSNE_TILE_COLS;             // columns per LDS tile (one point per thread to stage)
constexpr int MAX_SLICES = 64;
constexpr int MAX_N = 1 << 24;                      // rows: 2N is exact in f32, N + a tile cannot overflow int
constexpr int TARGET_BLOCKS = 2048;                 // 256 CUs x 8: the slices multiply the row blocks up to this
static_assert(RB == 256 * RPL && TJ == 256, "the repulsion kernel stages one point and owns RPL rows per thread");

__device__ __forceinline__ float wave_min(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- affinities ----------------------------------------------------------------------------------------------------
// exp(-beta * x) for x = xh + xl (xl: the rounding error of xh = d - dmin, so the distance gap enters exactly) with
// the product's own rounding error folded back in: the result is within an ulp or two of the exact exponential of the
// f32 inputs whatever the size of the exponent. th (out): the rounded exponent, for the entropy's sum of t * p.
__device__ __forceinline__ float affinity_exp(float beta, float xh, float xl, float& th) {
#pragma clang fp contract(off)
  th = beta * xh;
  const float tl = fmaf(beta, xh, -th) + beta * xl;
  const float p = expf(-th);
  return p > 0.f ? fmaf(p, -tl, p) : 0.f;   // p = 0: th may be inf and tl NaN
}

__global__ __launch_bounds__(256) void tsne_affinities_kernel(const float* __restrict__ dist, int N, int k,
                                                              float log_perp, float* __restrict__ p_out,
                                                              float* __restrict__ beta_out) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row = (long long)blockIdx.x * 4 + wave;
  if (row >= N) return;   // wave-uniform
  const bool act = lane < k;
  const float d = act ? dist[row * k + lane] : __builtin_inff();
  const float dmin = wave_min(d);
  const float xh = act ? d - dmin : 0.f;
  const float xl = act ? (0.f - dmin) - (xh - d) : 0.f;   // Fast2Sum: xh + xl = d - dmin exactly (|d| >= |dmin|)
  float beta = 1.0f, lo = -__builtin_inff(), hi = __builtin_inff();
  float p = 0.f, sum = 1.f;
  for (int step = 0; step < 100; ++step) {
    float th;
    p = act ? affinity_exp(beta, xh, xl, th) : 0.f;
    sum = wave_sum(p);                       // >= 1: the minimum's own term
    const float tp = wave_sum(p > 0.f ? th * p : 0.f);
    const float diff = (logf(sum) + tp / sum) - log_perp;
    if (__builtin_amdgcn_readfirstlane(fabsf(diff) <= 1e-5f)) break;
    if (diff > 0.f) {
      lo = beta;
      beta = hi == __builtin_inff() ? beta * 2.0f : (beta + hi) * 0.5f;
    } else {
      hi = beta;
      beta = lo == -__builtin_inff() ? beta * 0.5f : (beta + lo) * 0.5f;
    }
    if (step == 99) {   // the last move is not evaluated above: p belongs to the beta that is reported
      p = act ? affinity_exp(beta, xh, xl, th) : 0.f;
      sum = wave_sum(p);
    }
  }
  if (act) p_out[row * k + lane] = p / sum;
  if (lane == 0) beta_out[row] = beta;
}

// ---- repulsion -----------------------------------------------------------------------------------------------------
struct RepGeom {
  int row_blocks, slices, slice_cols, sum_blocks;
};
__host__ __device__ inline RepGeom rep_geom(int N) {
  RepGeom g;
  g.row_blocks = (N + RB - 1) / RB;
  const int tiles = (N + TJ - 1) / TJ;
  int s = (TARGET_BLOCKS + g.row_blocks - 1) / g.row_blocks;
  s = s < tiles ? s : tiles;
  s = s < MAX_SLICES ? s : MAX_SLICES;
  const int tiles_per_slice = (tiles + s - 1) / s;
  g.slice_cols = tiles_per_slice * TJ;
  g.slices = (tiles + tiles_per_slice - 1) / tiles_per_slice;
  g.sum_blocks = (N + 255) / 256;
  return g;
}

// One column against the lane's RPL rows. CHECK: the column may be one of the workgroup's rows or past the end.
template <bool CHECK>
__device__ __forceinline__ void rep_pair(float xj, float yj, int j, int jend, const float (&xi)[RPL],
                                         const float (&yi)[RPL], const int (&ri)[RPL], float (&rx)[RPL],
                                         float (&ry)[RPL], float (&z)[RPL]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    const float dx = xi[r] - xj, dy = yi[r] - yj;
    const float d2 = fmaf(dy, dy, fmaf(dx, dx, 1.0f));
    float q = __builtin_amdgcn_rcpf(d2);
    if constexpr (CHECK) q = (j != ri[r] && j < jend) ? q : 0.f;
    const float q2 = q * q;
    z[r] += q;
    rx[r] = fmaf(q2, dx, rx[r]);
    ry[r] = fmaf(q2, dy, ry[r]);
  }
}

template <bool CHECK>
__device__ __forceinline__ void rep_tile(const float* tile, int j0, int jend, const float (&xi)[RPL],
                                         const float (&yi)[RPL], const int (&ri)[RPL], float (&rx)[RPL],
                                         float (&ry)[RPL], float (&z)[RPL]) {
#pragma unroll 4
  for (int jj = 0; jj < TJ; jj += 2) {
    const f32x4 pj = *(const f32x4*)&tile[2 * jj];   // two points, the same address in every lane: a broadcast
    rep_pair<CHECK>(pj[0], pj[1], j0 + jj, jend, xi, yi, ri, rx, ry, z);
    rep_pair<CHECK>(pj[2], pj[3], j0 + jj + 1, jend, xi, yi, ri, rx, ry, z);
  }
}

// grid (row blocks, slices). part f32 [slices][3][N]: (rep x, rep y, zrow) of the slice's columns.
__global__ __launch_bounds__(256) void tsne_repulse_partial_kernel(const float* __restrict__ y, int N, int slice_cols,
                                                                   float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float tile[2 * TJ];
  const int row0 = blockIdx.x * RB;
  const int jbeg = blockIdx.y * slice_cols;
  const int jend = min(N, jbeg + slice_cols);   // jbeg < N by the geometry
  float xi[RPL], yi[RPL], rx[RPL], ry[RPL], z[RPL];
  int ri[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    ri[r] = row0 + 256 * r + threadIdx.x;
    const f32x2 v = *(const f32x2*)&y[2 * (long long)min(ri[r], N - 1)];
    xi[r] = v[0], yi[r] = v[1];
    rx[r] = ry[r] = z[r] = 0.f;
  }
  for (int j0 = jbeg; j0 < jend; j0 += TJ) {
    const int j = j0 + threadIdx.x;
    const f32x2 v = j < N ? *(const f32x2*)&y[2 * (long long)j] : (f32x2){0.f, 0.f};
    __syncthreads();   // the previous tile has been read
    *(f32x2*)&tile[2 * threadIdx.x] = v;
    __syncthreads();
    const bool check = j0 + TJ > jend || (j0 < row0 + RB && j0 + TJ > row0);   // workgroup-uniform
    if (check) rep_tile<true>(tile, j0, jend, xi, yi, ri, rx, ry, z);
    else rep_tile<false>(tile, j0, jend, xi, yi, ri, rx, ry, z);
  }
  float* dst = part + (long long)blockIdx.y * 3 * N;
#pragma unroll
  for (int r = 0; r < RPL; ++r)
    if (ri[r] < N) {
      dst[ri[r]] = rx[r];
      dst[(long long)N + ri[r]] = ry[r];
      dst[2 * (long long)N + ri[r]] = z[r];
    }
}

// 256 doubles of a workgroup, one per thread -> their sum in thread 0 (butterfly per wave, the four waves in order)
__device__ __forceinline__ double block_sum_d(double v, double* sm4) {
  v = wave_sum_d(v);
  if ((threadIdx.x & 63) == 0) sm4[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sm4[0] + sm4[1]) + sm4[2]) + sm4[3];
}

// one thread per row: the slices in order; the workgroup's zrow sum (f64) to bsum[blockIdx.x]
__global__ __launch_bounds__(256) void tsne_repulse_sum_kernel(const float* __restrict__ part, int N, int slices,
                                                               float* __restrict__ rep, float* __restrict__ zrow,
                                                               double* __restrict__ bsum) {
#pragma clang fp contract(off)
  __shared__ double sm4[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  float rx = 0.f, ry = 0.f, z = 0.f;
  if (i < N) {
    for (int s = 0; s < slices; ++s) {
      const float* src = part + (long long)s * 3 * N;
      rx += src[i];
      ry += src[(long long)N + i];
      z += src[2 * (long long)N + i];
    }
    *(f32x2*)&rep[2 * (long long)i] = (f32x2){rx, ry};
    zrow[i] = z;
  }
  const double t = block_sum_d((double)z, sm4);
  if (threadIdx.x == 0) bsum[blockIdx.x] = t;
}

__global__ __launch_bounds__(256) void tsne_repulse_total_kernel(const double* __restrict__ bsum, int n,
                                                                 float* __restrict__ zsum) {
  __shared__ double sm4[4];
  double v = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) v += bsum[i];
  const double t = block_sum_d(v, sm4);
  if (threadIdx.x == 0) *zsum = (float)t;
}

// ---- attraction ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_attract_kernel(const float* __restrict__ y, const int32_t* __restrict__ nbr,
                                                           const float* __restrict__ p,
                                                           const int32_t* __restrict__ rev_ptr,
                                                           const int32_t* __restrict__ rev_edge, int N, int k,
                                                           float* __restrict__ attr) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long i = (long long)blockIdx.x * 4 + wave;
  if (i >= N) return;   // wave-uniform
  const long long ne = (long long)N * k;
  // a damaged reverse list cannot send a read outside the arrays: bounds and ids are clamped, not trusted
  const long long rp = min(max((long long)rev_ptr[i], 0ll), ne);
  const long long re = min(max((long long)rev_ptr[i + 1], rp), ne);
  const int tot = k + (int)(re - rp);
  const f32x2 yi = *(const f32x2*)&y[2 * i];
  float fx = 0.f, fy = 0.f;
  for (int t = lane; t < tot; t += 64) {
    long long e;
    int j;
    if (t < k) {
      e = i * k + t;
      j = nbr[e];
    } else {
      e = min(max((long long)rev_edge[rp + (t - k)], 0ll), ne - 1);
      j = (int)((unsigned)e / (unsigned)k);   // e < N * k < 2^31: a 32-bit division
    }
    j = min(max(j, 0), N - 1);
    const float w = p[e];
    const f32x2 yj = *(const f32x2*)&y[2 * (long long)j];
    const float dx = yi[0] - yj[0], dy = yi[1] - yj[1];
    const float q = __builtin_amdgcn_rcpf(fmaf(dy, dy, fmaf(dx, dx, 1.0f)));
    const float wq = w * q;
    fx = fmaf(wq, dx, fx);
    fy = fmaf(wq, dy, fy);
  }
  fx = wave_sum(fx);
  fy = wave_sum(fy);
  if (lane == 0) *(f32x2*)&attr[2 * i] = (f32x2){fx, fy};
}

// ---- update --------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void tsne_update_kernel(float* __restrict__ y, float* __restrict__ vel,
                                                          float* __restrict__ gains, const float* __restrict__ attr,
                                                          const float* __restrict__ rep,
                                                          const float* __restrict__ zsum, long long n2, float ca,
                                                          float lr, float momentum) {
#pragma clang fp contract(off)
  const float zs = *zsum;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n2; i += (long long)gridDim.x * 256) {
    const float g = 4.0f * fmaf(ca, attr[i], -(rep[i] / zs));
    const float v = vel[i];
    float gn = gains[i];
    gn = (v * g < 0.f) ? gn + 0.2f : gn * 0.8f;
    gn = fmaxf(gn, 0.01f);
    const float vn = fmaf(momentum, v, -((lr * gn) * g));
    gains[i] = gn;
    vel[i] = vn;
    y[i] += vn;
  }
}

bool bad_graph(int32_t N, int32_t k, int32_t min_rows) {
  return N < min_rows || k < 1 || k > 64 || (int64_t)N * k >= ((int64_t)1 << 31);
}

}  // namespace

SVAE_EXPORT int svae_tsne_affinities(const float* dist, int32_t N, int32_t k, float perplexity, float* p, float* beta,
                                     svae_stream_t stream) {
  if (!dist || !p || !beta || bad_graph(N, k, 1)) return SVAE_EINVAL;
  if (!(perplexity > 1.0f && perplexity < (float)k)) return SVAE_EINVAL;
  hipLaunchKernelGGL(tsne_affinities_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, dist, (int)N, (int)k,
                     logf(perplexity), p, beta);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_tsne_repulse_slice_cols(int32_t N) {
  return N < 2 || N > MAX_N ? 0 : rep_geom(N).slice_cols;
}

SVAE_EXPORT int64_t svae_tsne_repulse_ws_bytes(int32_t N) {
  if (N < 2 || N > MAX_N) return 0;
  const RepGeom g = rep_geom(N);
  const int64_t part = (int64_t)g.slices * 3 * N * (int64_t)sizeof(float);
  return ((part + 7) & ~(int64_t)7) + (int64_t)g.sum_blocks * (int64_t)sizeof(double);
}

SVAE_EXPORT int svae_tsne_repulse(const float* y, int32_t N, void* ws, int64_t ws_bytes, float* rep, float* zrow,
                                  float* zsum, svae_stream_t stream) {
  if (!y || !rep || !zrow || !zsum || N < 2 || N > MAX_N) return SVAE_EINVAL;
  if (((uintptr_t)y & 7) || ((uintptr_t)rep & 7)) return SVAE_EINVAL;
  if (!ws || ((uintptr_t)ws & 7) || ws_bytes < svae_tsne_repulse_ws_bytes(N)) return SVAE_EINVAL;
  const RepGeom g = rep_geom(N);
  const int64_t part_bytes = ((int64_t)g.slices * 3 * N * (int64_t)sizeof(float) + 7) & ~(int64_t)7;
  float* part = (float*)ws;
  double* bsum = (double*)((char*)ws + part_bytes);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(tsne_repulse_partial_kernel, dim3(g.row_blocks, g.slices), dim3(256), 0, s, y, (int)N,
                     g.slice_cols, part);
  hipLaunchKernelGGL(tsne_repulse_sum_kernel, dim3(g.sum_blocks), dim3(256), 0, s, (const float*)part, (int)N,
                     g.slices, rep, zrow, bsum);
  hipLaunchKernelGGL(tsne_repulse_total_kernel, dim3(1), dim3(256), 0, s, (const double*)bsum, g.sum_blocks, zsum);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_tsne_attract(const float* y, const int32_t* nbr, const float* p, const int32_t* rev_ptr,
                                  const int32_t* rev_edge, int32_t N, int32_t k, float* attr, svae_stream_t stream) {
  if (!y || !nbr || !p || !rev_ptr || !rev_edge || !attr || bad_graph(N, k, 2)) return SVAE_EINVAL;
  if (((uintptr_t)y & 7) || ((uintptr_t)attr & 7)) return SVAE_EINVAL;
  hipLaunchKernelGGL(tsne_attract_kernel, dim3((N + 3) / 4), dim3(256), 0, (hipStream_t)stream, y, nbr, p, rev_ptr,
                     rev_edge, (int)N, (int)k, attr);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_tsne_update(float* y, float* vel, float* gains, const float* attr, const float* rep,
                                 const float* zsum, int32_t N, float exaggeration, float learning_rate, float momentum,
                                 svae_stream_t stream) {
  if (!y || !vel || !gains || !attr || !rep || !zsum || N < 2 || N > MAX_N) return SVAE_EINVAL;
  const long long n2 = 2 * (long long)N;
  const float ca = exaggeration / (float)n2;   // (float)(2N) is exact: N <= 2^24
  const int grid = (int)min((long long)2048, (n2 + 255) / 256);
  hipLaunchKernelGGL(tsne_update_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, y, vel, gains, attr, rep, zsum,
                     n2, ca, learning_rate, momentum);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
