// k-means of the latent index (Lloyd's iteration with k-means++ seeding) over the posterior means: what stands in for
// the topic colouring of the reference's tsne.py (an LDA model from gensim), from the latents alone.
//
//   svae_kmeans_assign: every row's nearest centroid, its squared distance, the number of labels that changed and the
//                       inertia. Two launches: a workgroup owns a block of rows (held in registers) and streams the
//                       centroids through LDS in tiles; one workgroup adds the per-workgroup partials.
//   svae_kmeans_update: the centroids as f64 means of their rows. Five launches: a stable counting sort of the row
//                       numbers by label (per-block histograms, a scan, a scatter by rank), one f64 segment sum per
//                       (centroid, row group), and the division.
//   svae_kmeans_seed:   k-means++ (D^2 sampling). Per step one pass that lowers every row's running minimum against
//                       the centroid chosen last and one workgroup that draws the next row from the f64 prefix sums.
//                       The chosen row stays on the device.
//
// No atomics anywhere: grids and summation orders are functions of (N, K, Z) alone, so a result is a pure function of
// its inputs, bit for bit. Arithmetic and orders:
//   distance  d2(x, c) from direct differences: per float4 chunk of the row, d = x - c (one rounding per element),
//             then two fmaf chains, one over elements 0 and 2 and one over elements 1 and 3 of the chunks in chunk
//             order (packed f32 math: the chains are the two halves of a v_pk_fma_f32), d2 = chain A + chain B.
//             Contraction is off and the FMAs are written out, so the f32 distance of a (row, centroid) pair is the
//             same bits in the assignment and in the seeding, whichever lane computes it. A chain takes Z / 2 FMAs on
//             a partial sum of non-negative terms (one rounding each), a square carries the two roundings of its
//             difference, and the chains' sum is one more: |error| <= (Z / 2 + 3) 2^-24 d2 to first order.
//   assign    the centroids in index order; a centroid replaces the lane's best only if its distance is smaller, or is
//             a number where the best is NaN: ties go to the lower index, NaN loses to every number, an all-NaN row
//             keeps label 0 and d2 NaN. inertia: a lane adds its rows' d2 (widened to f64) in row order; 64-lane xor
//             butterfly, the four waves in order; the total: lane t adds workgroups t, t + 256, ..., butterfly, waves.
//   update    the rows are cut into B = sort blocks of consecutive rows (svae_kmeans_geometry) and the blocks into G
//             groups of consecutive blocks. S_c = the G group sums in ascending group order; a group sum adds the
//             rows of cluster c inside the group in ascending row order; every element is widened to f64 first.
//             B and G depend on (N, K) alone, so the tree is fixed. cent = (float)(S_c / (double)count_c).
//   seed      the prefix sums are nested three deep, each level in ascending order in f64: w_i over the rows of a block
//             of 256, Q over the blocks of a run of 256 blocks, P over the runs; cumsum_i = P + (Q + w_i). Every
//             level's last value is the next level's term, so the cumsum is non-decreasing in i and its last value is
//             the total. At N <= 256 this is the plain running sum.
#include <math.h>

#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int TC = SVAE_KMEANS_TILE_CENTROIDS;   // centroids per LDS tile
constexpr int MAXK = SVAE_KMEANS_MAX_K;
constexpr int KQ = MAXK / 256;                   // bins per thread of the counting sort
constexpr int SORT_BLOCKS = SVAE_KMEANS_SORT_BLOCKS;
constexpr int SORT_CHUNK = 2048;                 // labels per LDS chunk of a sort block
constexpr int SEG_ITEMS = 4096;                  // (centroid, row group) segment sums aimed at: 256 CUs x 16 waves
constexpr int SB = SVAE_KMEANS_SEED_BLOCK_ROWS;
constexpr int MAX_ROWS = 1 << 24;
static_assert(MAXK % 256 == 0 && SORT_CHUNK % 4 == 0 && SB == 256, "geometry");
static_assert((long long)SB * SB * SB >= MAX_ROWS, "three levels of 256 cover every row");

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// One float4 chunk of a (row, centroid) pair: THE distance arithmetic, shared by the assignment and the seeding.
__device__ __forceinline__ void dist_chunk(f32x2& s, const f32x4 xv, const f32x4 cv) {
#pragma clang fp contract(off)
  const f32x4 d = xv - cv;
  const f32x2 lo = {d[0], d[1]}, hi = {d[2], d[3]};
  s = __builtin_elementwise_fma(lo, lo, s);
  s = __builtin_elementwise_fma(hi, hi, s);
}
__device__ __forceinline__ float dist_finish(const f32x2 s) {
#pragma clang fp contract(off)
  return s[0] + s[1];
}

// ---- assign --------------------------------------------------------------------------------------------------------
// grid: row blocks of 256 * RPL rows. part_in f64 [row blocks], part_ch int32 [row blocks].
template <int ZCAP, int RPL>
__global__ __launch_bounds__(256) void assign_kernel(const float* __restrict__ x, int N, const float* __restrict__ cent,
                                                     int K, int Z, int* __restrict__ label, float* __restrict__ d2out,
                                                     double* __restrict__ part_in, int* __restrict__ part_ch) {
#pragma clang fp contract(off)
  constexpr int RB = 256 * RPL;
  __shared__ __attribute__((aligned(16))) float tile[TC * ZCAP];
  __shared__ double redd[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x, zc_n = Z >> 2;
  const int row0 = blockIdx.x * RB;
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
  float best[RPL];
  int bi[RPL];
#pragma unroll
  for (int r = 0; r < RPL; ++r) best[r] = __builtin_nanf(""), bi[r] = 0;
  for (int c0 = 0; c0 < K; c0 += TC) {
    const int nc = min(TC, K - c0);   // workgroup-uniform
    __syncthreads();                  // the previous tile has been read
    const float* src = cent + (long long)c0 * Z;
    for (int v = tid; v < nc * zc_n; v += 256) *(f32x4*)&tile[4 * v] = *(const f32x4*)(src + 4 * v);
    __syncthreads();
    for (int jj = 0; jj < nc; ++jj) {
      const float* cj = tile + jj * Z;   // the same address in every lane: a broadcast
      f32x2 s[RPL];
#pragma unroll
      for (int r = 0; r < RPL; ++r) s[r] = (f32x2){0.f, 0.f};
#pragma unroll
      for (int zc = 0; zc < ZCAP / 4; ++zc) {
        if (zc < zc_n) {   // workgroup-uniform
          const f32x4 cv = *(const f32x4*)(cj + 4 * zc);
#pragma unroll
          for (int r = 0; r < RPL; ++r) dist_chunk(s[r], xi[r][zc], cv);
        }
      }
#pragma unroll
      for (int r = 0; r < RPL; ++r) {
        const float d = dist_finish(s[r]);
        const bool take = d < best[r] || (best[r] != best[r] && d == d);
        best[r] = take ? d : best[r];
        bi[r] = take ? c0 + jj : bi[r];
      }
    }
  }
  int ch = 0;
  double in64 = 0.0;
#pragma unroll
  for (int r = 0; r < RPL; ++r) {
    if (ri[r] < N) {
      ch += label[ri[r]] != bi[r];
      label[ri[r]] = bi[r];
      if (d2out) d2out[ri[r]] = best[r];
      in64 += (double)best[r];
    }
  }
  ch = wave_sum_i(ch);
  in64 = wave_sum_d(in64);
  if ((tid & 63) == 0) redi[tid >> 6] = ch, redd[tid >> 6] = in64;
  __syncthreads();
  if (tid == 0) {
    part_ch[blockIdx.x] = ((redi[0] + redi[1]) + redi[2]) + redi[3];
    part_in[blockIdx.x] = ((redd[0] + redd[1]) + redd[2]) + redd[3];
  }
}

__global__ __launch_bounds__(256) void assign_final_kernel(const double* __restrict__ part_in,
                                                           const int* __restrict__ part_ch, int n,
                                                           double* __restrict__ inertia, int* __restrict__ changed) {
  __shared__ double redd[4];
  __shared__ int redi[4];
  const int tid = threadIdx.x;
  double v = 0.0;
  int c = 0;
  for (int i = tid; i < n; i += 256) v += part_in[i], c += part_ch[i];
  v = wave_sum_d(v);
  c = wave_sum_i(c);
  if ((tid & 63) == 0) redd[tid >> 6] = v, redi[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) {
    *inertia = ((redd[0] + redd[1]) + redd[2]) + redd[3];
    *changed = ((redi[0] + redi[1]) + redi[2]) + redi[3];
  }
}

// ---- update --------------------------------------------------------------------------------------------------------
// One pass of a sort block over its rows' labels, LDS chunk by LDS chunk. Thread t owns the bins t, t + 256, ... and
// walks the chunk in row order, so its running count of a bin is the rank of the row among the block's rows of that
// label: no atomics, and the scatter is stable. SCATTER false: hist[block][bin] = the counts. SCATTER true:
// perm[base[bin] + hist[block][bin] + rank] = row (hist now holding the exclusive prefix over the blocks).
// NQ = ceil(K / 256): the bins a thread owns (a label is compared with no more).
template <bool SCATTER, int NQ>
__global__ __launch_bounds__(256) void sort_pass_kernel(const int* __restrict__ label, int N, int K, int rows_per,
                                                        int* __restrict__ hist, const int* __restrict__ base,
                                                        int* __restrict__ perm) {
  typedef int i32x4 __attribute__((ext_vector_type(4)));
  __shared__ __attribute__((aligned(16))) int lab[SORT_CHUNK];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int r0 = b * rows_per, r1 = min(N, r0 + rows_per);
  int cnt[NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const int c = tid + 256 * q;
    cnt[q] = 0;
    if constexpr (SCATTER) cnt[q] = c < K ? base[c] + hist[(long long)b * K + c] : 0;
  }
  for (int c0 = r0; c0 < r1; c0 += SORT_CHUNK) {
    __syncthreads();   // the previous chunk has been read
    for (int i = tid; i < SORT_CHUNK; i += 256) {
      int l = -1;      // rows past the block and labels outside 0..K-1 match no bin
      if (c0 + i < r1) {
        l = label[c0 + i];
        if (l < 0 || l >= K) l = -1;
      }
      lab[i] = l;
    }
    __syncthreads();
    if (tid < K) {
      const int n = min(SORT_CHUNK, r1 - c0);
      for (int i = 0; i < n; i += 4) {
        const i32x4 l4 = *(const i32x4*)&lab[i];   // a broadcast
#pragma unroll
        for (int e = 0; e < 4; ++e) {
#pragma unroll
          for (int q = 0; q < NQ; ++q) {
            if (l4[e] == tid + 256 * q) {
              if constexpr (SCATTER) {
                if (cnt[q] >= 0 && cnt[q] < N) perm[cnt[q]] = c0 + i + e;
              }
              ++cnt[q];
            }
          }
        }
      }
    }
  }
  if constexpr (!SCATTER) {
#pragma unroll
    for (int q = 0; q < NQ; ++q)
      if (tid + 256 * q < K) hist[(long long)b * K + tid + 256 * q] = cnt[q];
  }
}

// One workgroup. hist[b][c] becomes the exclusive prefix over the blocks of bin c; count[c] the bin's total;
// base[c] the exclusive prefix of the totals over the bins, base[K] their sum.
__global__ __launch_bounds__(256) void sort_scan_kernel(int* __restrict__ hist, int B, int K, int* __restrict__ base,
                                                        int* __restrict__ count) {
  __shared__ int wsum[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int carry = 0;
  for (int q = 0; q < KQ; ++q) {   // bins in ascending order: q major, thread minor
    const int c = tid + 256 * q;
    int tot = 0;
    if (c < K) {
      for (int b = 0; b < B; b += 8) {   // eight loads in flight, then their prefix
        int h[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = b + k < B ? hist[(long long)(b + k) * K + c] : 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
          if (b + k < B) hist[(long long)(b + k) * K + c] = tot;
          tot += h[k];
        }
      }
      count[c] = tot;
    }
    int inc = tot;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(inc, o, 64);
      if (lane >= o) inc += t;
    }
    __syncthreads();   // wsum of the previous q has been read
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = carry;
    for (int i = 0; i < w; ++i) off += wsum[i];
    if (c < K) base[c] = off + inc - tot;
    carry += ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
  }
  if (tid == 0) base[K] = carry;
}

// grid (K, G), one wave each: the f64 sum of cluster c's rows inside row group g (sort blocks g * bpg ..), ascending.
// part f64 [G][K][Z].
__global__ __launch_bounds__(64) void segsum_kernel(const float* __restrict__ x, int N, int Z, int K, int B, int bpg,
                                                    const int* __restrict__ hist, const int* __restrict__ base,
                                                    const int* __restrict__ perm, double* __restrict__ part) {
  const int c = blockIdx.x, g = blockIdx.y, lane = threadIdx.x;
  const int b0 = g * bpg, b1 = b0 + bpg;
  const int first = base[c], last = base[c + 1];
  int p0 = b0 < B ? first + hist[(long long)b0 * K + c] : last;
  int p1 = b1 < B ? first + hist[(long long)b1 * K + c] : last;
  p0 = max(0, min(p0, N)), p1 = max(p0, min(p1, N));   // perm holds N entries
  double s[4] = {0.0, 0.0, 0.0, 0.0};
  int p = p0;
  constexpr int UR = 16;   // rows in flight per lane: the loads are issued together, the adds stay in row order
  for (; p + UR <= p1; p += UR) {
    float v[UR][4];
#pragma unroll
    for (int u = 0; u < UR; ++u) {
      const int row = max(0, min(perm[p + u], N - 1));
#pragma unroll
      for (int j = 0; j < 4; ++j) v[u][j] = lane + 64 * j < Z ? x[(long long)row * Z + lane + 64 * j] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < UR; ++u)
#pragma unroll
      for (int j = 0; j < 4; ++j) s[j] += (double)v[u][j];
  }
  for (; p < p1; ++p) {
    const int row = max(0, min(perm[p], N - 1));
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j < Z) s[j] += (double)x[(long long)row * Z + lane + 64 * j];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (lane + 64 * j < Z) part[((long long)g * K + c) * Z + lane + 64 * j] = s[j];
}

// One thread per (centroid, column): the groups in order, the division in f64. An empty cluster keeps its centroid.
__global__ __launch_bounds__(256) void update_final_kernel(const double* __restrict__ part, int G, int K, int Z,
                                                           const int* __restrict__ base, float* __restrict__ cent) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= K * Z) return;
  const int c = i / Z;
  const int n = base[c + 1] - base[c];
  if (n <= 0) return;
  double s = 0.0;
  for (int g = 0; g < G; ++g) s += part[(long long)g * K * Z + i];
  cent[i] = (float)(s / (double)n);
}

// ---- seed ----------------------------------------------------------------------------------------------------------
// One thread per row: mind = min(mind, d2(row, the centroid chosen in step - 1)); bsum[block] = the block's 256 minima
// added in row order (by one thread: the order the draw retraces).
__global__ __launch_bounds__(256) void seed_dist_kernel(const float* __restrict__ x, int N, int Z,
                                                        const int* __restrict__ rows, int step,
                                                        float* __restrict__ mind, double* __restrict__ bsum) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float c[256];
  __shared__ double m[SB];
  const int tid = threadIdx.x, zc_n = Z >> 2;
  const int prev = max(0, min(rows[step - 1], N - 1));
  if (tid < Z) c[tid] = x[(long long)prev * Z + tid];
  __syncthreads();
  const int row = blockIdx.x * SB + tid;
  double md = 0.0;
  if (row < N) {
    const float* xr = x + (long long)row * Z;
    f32x2 s = {0.f, 0.f};
    for (int zc = 0; zc < zc_n; ++zc) dist_chunk(s, *(const f32x4*)(xr + 4 * zc), *(const f32x4*)(c + 4 * zc));
    float d = dist_finish(s);
    if (step > 1) {
      const float old = mind[row];
      d = d < old ? d : old;
    }
    mind[row] = d;
    md = (double)d;
  }
  m[tid] = md;
  __syncthreads();
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < SB; ++i) s += m[i];
    bsum[blockIdx.x] = s;
  }
}

// One workgroup: draw the row of this step, record it and copy it into cent[step].
__global__ __launch_bounds__(256) void seed_pick_kernel(const float* __restrict__ x, int N, int Z,
                                                        const float* __restrict__ mind,
                                                        const double* __restrict__ bsum, int nb,
                                                        const float* __restrict__ u, unsigned long long seed, int step,
                                                        int* __restrict__ rows, float* __restrict__ cent) {
#pragma clang fp contract(off)
  __shared__ double sh[SB];
  __shared__ double s_target, s_p, s_q;
  __shared__ int s_sel, s_done;   // s_done: the row is final (s_sel is the row); else s_sel is the run / the block
  const int tid = threadIdx.x;
  const float us = u ? u[step] : rand_uniform(seed, (unsigned long long)step);
  if (step == 0) {
    if (tid == 0) {
      const double f = floor((double)us * (double)N);
      s_sel = f >= 0.0 ? (f < (double)N ? (int)f : N - 1) : 0;   // NaN: row 0
    }
    __syncthreads();
  } else {
    const int nr = (nb + SB - 1) / SB;
    {   // the runs' sums
      double r = 0.0;
      if (tid < nr)
        for (int b = tid * SB; b < min(nb, (tid + 1) * SB); ++b) r += bsum[b];
      sh[tid] = r;
    }
    __syncthreads();
    if (tid == 0) {
      double total = 0.0;
      for (int r = 0; r < nr; ++r) total += sh[r];
      s_done = 0;
      if (!(total > 0.0)) {   // fewer distinct points than centroids (or no number): row 0
        s_done = 1, s_sel = 0;
      } else {
        const double target = (double)us * total;
        double P = 0.0;
        int r = 0;
        for (; r < nr - 1; ++r) {
          if (P + sh[r] > target) break;
          P += sh[r];
        }
        s_target = target, s_p = P, s_sel = r;   // u >= 1: the last run, block and row
      }
    }
    __syncthreads();
    if (!s_done) {   // workgroup-uniform
      const int run = s_sel, bb = run * SB;
      const int nbr = min(SB, nb - bb);
      __syncthreads();   // s_sel has been read
      sh[tid] = tid < nbr ? bsum[bb + tid] : 0.0;
      __syncthreads();
      if (tid == 0) {
        double Q = 0.0;
        int b = 0;
        for (; b < nbr - 1; ++b) {
          if (s_p + (Q + sh[b]) > s_target) break;
          Q += sh[b];
        }
        s_q = Q, s_sel = bb + b;
      }
      __syncthreads();
      const int blk = s_sel, rr = blk * SB;
      const int nrow = min(SB, N - rr);
      __syncthreads();   // s_sel has been read
      sh[tid] = tid < nrow ? (double)mind[rr + tid] : 0.0;
      __syncthreads();
      if (tid == 0) {
        double w = 0.0;
        int i = 0;
        for (; i < nrow - 1; ++i) {
          w += sh[i];
          if (s_p + (s_q + w) > s_target) break;
        }
        s_sel = rr + i;
      }
      __syncthreads();
    }
  }
  const int row = max(0, min(s_sel, N - 1));
  if (tid == 0) rows[step] = row;
  if (tid < Z) cent[(long long)step * Z + tid] = x[(long long)row * Z + tid];
}

// ---- host ----------------------------------------------------------------------------------------------------------
struct Geom {
  int rb, row_blocks, sort_blocks, rows_per, groups, bpg, seed_blocks;
};
bool bad_shape(int32_t N, int32_t K, int32_t Z) {
  return N < 1 || N > MAX_ROWS || Z < 4 || Z > 256 || (Z & 3) || K < 1 || K > MAXK || K > N;
}
Geom geom_of(int N, int K, int Z) {
  Geom g;
  g.rb = Z <= 64 ? 512 : 256;
  g.row_blocks = (N + g.rb - 1) / g.rb;
  const int want = (N + 255) / 256 < SORT_BLOCKS ? (N + 255) / 256 : SORT_BLOCKS;
  g.rows_per = (N + want - 1) / want;
  g.sort_blocks = (N + g.rows_per - 1) / g.rows_per;
  int gw = SEG_ITEMS / K;
  gw = gw < 1 ? 1 : (gw > g.sort_blocks ? g.sort_blocks : gw);
  g.bpg = (g.sort_blocks + gw - 1) / gw;
  g.groups = (g.sort_blocks + g.bpg - 1) / g.bpg;
  g.seed_blocks = (N + SB - 1) / SB;
  return g;
}
bool bad_ptr(const void* p, int align) { return !p || ((uintptr_t)p & (uintptr_t)(align - 1)); }
bool bad_ws(const void* ws, int64_t have, int64_t need) { return bad_ptr(ws, 8) || need <= 0 || have < need; }
int64_t round8(int64_t v) { return (v + 7) & ~(int64_t)7; }

template <int ZCAP, int RPL>
void launch_assign(int blocks, hipStream_t s, const float* x, int N, const float* cent, int K, int Z, int* label,
                   float* d2, double* part_in, int* part_ch) {
  hipLaunchKernelGGL((assign_kernel<ZCAP, RPL>), dim3(blocks), dim3(256), 0, s, x, N, cent, K, Z, label, d2, part_in,
                     part_ch);
}

template <bool SCATTER>
void launch_sort_pass(const Geom& g, hipStream_t s, const int* label, int N, int K, int* hist, const int* base,
                      int* perm) {
  const dim3 grid(g.sort_blocks), block(256);
  switch ((K + 255) / 256) {
    case 1: hipLaunchKernelGGL((sort_pass_kernel<SCATTER, 1>), grid, block, 0, s, label, N, K, g.rows_per, hist, base, perm); break;
    case 2: hipLaunchKernelGGL((sort_pass_kernel<SCATTER, 2>), grid, block, 0, s, label, N, K, g.rows_per, hist, base, perm); break;
    case 3: hipLaunchKernelGGL((sort_pass_kernel<SCATTER, 3>), grid, block, 0, s, label, N, K, g.rows_per, hist, base, perm); break;
    default: hipLaunchKernelGGL((sort_pass_kernel<SCATTER, KQ>), grid, block, 0, s, label, N, K, g.rows_per, hist, base, perm); break;
  }
}

}  // namespace

SVAE_EXPORT int svae_kmeans_geometry(int32_t N, int32_t K, int32_t Z, int32_t* geom) {
  if (!geom || bad_shape(N, K, Z)) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z);
  geom[0] = g.rb, geom[1] = g.row_blocks, geom[2] = TC, geom[3] = g.sort_blocks, geom[4] = g.rows_per;
  geom[5] = g.groups, geom[6] = SB, geom[7] = g.seed_blocks;
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_kmeans_assign_ws_bytes(int32_t N, int32_t K, int32_t Z) {
  if (bad_shape(N, K, Z)) return 0;
  return (int64_t)geom_of(N, K, Z).row_blocks * 16;
}

SVAE_EXPORT int svae_kmeans_assign(const float* x, int32_t N, const float* cent, int32_t K, int32_t Z, int32_t* label,
                                   float* d2, int32_t* changed, double* inertia, void* ws, int64_t ws_bytes,
                                   svae_stream_t stream) {
  if (bad_shape(N, K, Z) || bad_ptr(x, 16) || bad_ptr(cent, 16) || bad_ptr(label, 4) || ((uintptr_t)d2 & 3) ||
      bad_ptr(changed, 4) || bad_ptr(inertia, 8))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_kmeans_assign_ws_bytes(N, K, Z))) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z);
  hipStream_t s = (hipStream_t)stream;
  double* part_in = (double*)ws;
  int* part_ch = (int*)(part_in + g.row_blocks);
  if (Z <= 32) launch_assign<32, 2>(g.row_blocks, s, x, N, cent, K, Z, label, d2, part_in, part_ch);
  else if (Z <= 64) launch_assign<64, 2>(g.row_blocks, s, x, N, cent, K, Z, label, d2, part_in, part_ch);
  else if (Z <= 128) launch_assign<128, 1>(g.row_blocks, s, x, N, cent, K, Z, label, d2, part_in, part_ch);
  else launch_assign<256, 1>(g.row_blocks, s, x, N, cent, K, Z, label, d2, part_in, part_ch);
  hipLaunchKernelGGL(assign_final_kernel, dim3(1), dim3(256), 0, s, (const double*)part_in, (const int*)part_ch,
                     g.row_blocks, inertia, changed);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_kmeans_update_ws_bytes(int32_t N, int32_t K, int32_t Z) {
  if (bad_shape(N, K, Z)) return 0;
  const Geom g = geom_of(N, K, Z);
  return (int64_t)g.groups * K * Z * 8 + round8(((int64_t)g.sort_blocks * K + K + 1 + N) * 4);
}

SVAE_EXPORT int svae_kmeans_update(const float* x, int32_t N, const int32_t* label, int32_t K, int32_t Z, float* cent,
                                   int32_t* count, void* ws, int64_t ws_bytes, svae_stream_t stream) {
  if (bad_shape(N, K, Z) || bad_ptr(x, 16) || bad_ptr(label, 4) || bad_ptr(cent, 16) || bad_ptr(count, 4))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_kmeans_update_ws_bytes(N, K, Z))) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z);
  hipStream_t s = (hipStream_t)stream;
  double* part = (double*)ws;
  int* hist = (int*)(part + (int64_t)g.groups * K * Z);
  int* base = hist + (int64_t)g.sort_blocks * K;
  int* perm = base + K + 1;
  launch_sort_pass<false>(g, s, label, N, K, hist, base, perm);
  hipLaunchKernelGGL(sort_scan_kernel, dim3(1), dim3(256), 0, s, hist, g.sort_blocks, (int)K, base, count);
  launch_sort_pass<true>(g, s, label, N, K, hist, base, perm);
  hipLaunchKernelGGL(segsum_kernel, dim3(K, g.groups), dim3(64), 0, s, x, (int)N, (int)Z, (int)K, g.sort_blocks, g.bpg,
                     (const int*)hist, (const int*)base, (const int*)perm, part);
  hipLaunchKernelGGL(update_final_kernel, dim3((K * Z + 255) / 256), dim3(256), 0, s, (const double*)part, g.groups,
                     (int)K, (int)Z, (const int*)base, cent);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int64_t svae_kmeans_seed_ws_bytes(int32_t N, int32_t K, int32_t Z) {
  if (bad_shape(N, K, Z)) return 0;
  return (int64_t)geom_of(N, K, Z).seed_blocks * 8 + round8((int64_t)N * 4);
}

SVAE_EXPORT int svae_kmeans_seed(const float* x, int32_t N, int32_t K, int32_t Z, const float* u, uint64_t seed,
                                 int32_t* rows, float* cent, void* ws, int64_t ws_bytes, svae_stream_t stream) {
  if (bad_shape(N, K, Z) || bad_ptr(x, 16) || ((uintptr_t)u & 3) || bad_ptr(rows, 4) || bad_ptr(cent, 16))
    return SVAE_EINVAL;
  if (bad_ws(ws, ws_bytes, svae_kmeans_seed_ws_bytes(N, K, Z))) return SVAE_EINVAL;
  const Geom g = geom_of(N, K, Z);
  hipStream_t s = (hipStream_t)stream;
  double* bsum = (double*)ws;
  float* mind = (float*)(bsum + g.seed_blocks);
  for (int step = 0; step < K; ++step) {
    if (step > 0)
      hipLaunchKernelGGL(seed_dist_kernel, dim3(g.seed_blocks), dim3(256), 0, s, x, (int)N, (int)Z, (const int*)rows,
                         step, mind, bsum);
    hipLaunchKernelGGL(seed_pick_kernel, dim3(1), dim3(256), 0, s, x, (int)N, (int)Z, (const float*)mind,
                       (const double*)bsum, g.seed_blocks, u, (unsigned long long)seed, step, rows, cent);
  }
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
