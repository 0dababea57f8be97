// Reconstruction scoring over token ids: the integer counts behind BLEU, token accuracy and the translation edit rate
// of a batch of (candidate, reference) pairs that already sit on the device as int16 rows (what sample_stream leaves).
//
//   svae_ngram_overlap: per pair the clipped n-gram match counts of orders 1..4 and the number of equal positions.
//                       One 256-thread workgroup per pair. Every position j of a row gives one 64-bit key: (token + 1)
//                       of positions j..j+3 in four 16-bit fields, first token on top, 0 where the row has ended. Both
//                       sides' keys are sorted once in LDS (bitonic, both arrays in the same passes); the order-n gram
//                       at j is the key's top n fields, so every order is a prefix of the same sorted order and a gram
//                       is complete exactly when its lowest field is not 0. A lane that holds the first key of a run of
//                       equal prefixes on the candidate side finds the run's end there and the run on the reference
//                       side by binary search and adds min(count, count).
//   svae_edit_distance: per pair the Levenshtein distance (unit costs). One wave per pair, four pairs per workgroup, no
//                       barrier inside the recurrence: lane l owns R >= ceil(Lc / 64) consecutive rows of the DP table
//                       (their previous column in registers) and walks the columns one step behind lane l - 1, whose
//                       bottom cell it receives through one shuffle per step. Lr + (lanes in use) - 1 steps of R cells.
//
// All results are integers, nothing is accumulated across workgroups, there are no atomics: a result is a pure function
// of the valid part of its two rows. Columns at or beyond a row's (clamped) length are never read.
#include "common.h"
#include "../../include/svae.h"

using namespace svae;

namespace {

constexpr int MAXLEN = SVAE_TEXT_MAX_LEN;
constexpr int TOKPAD = 4;                          // a key reads up to 3 positions past its own
static_assert((MAXLEN & (MAXLEN - 1)) == 0 && MAXLEN >= 2048, "the bitonic network wants a power of two");
// static LDS of ngram_kernel: keys 2 * MAXLEN * 8 + tokens 2 * (MAXLEN + 4) * 2 + partials 4 * 5 * 4
static_assert(2 * MAXLEN * 8 + 2 * (MAXLEN + TOKPAD) * 2 + 80 <= 64 * 1024, "ngram_kernel's LDS stays within 64 KiB");
static_assert(4 * MAXLEN * 2 <= 64 * 1024, "edit_kernel's LDS stays within 64 KiB");

typedef unsigned long long u64;

__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ int clamp_len(int len, int width) { return len < 0 ? 0 : (len > width ? width : len); }

// first index in [lo, hi) whose prefix (key >> shift) is >= p (UPPER: > p)
template <bool UPPER>
__device__ __forceinline__ int bound(const u64* a, int lo, int hi, u64 p, int shift) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const u64 v = a[mid] >> shift;
    const bool right = UPPER ? (v <= p) : (v < p);
    lo = right ? mid + 1 : lo;
    hi = right ? hi : mid;
  }
  return lo;
}

// grid: P. out int32 [P][5].
__global__ __launch_bounds__(256) void ngram_kernel(const unsigned short* __restrict__ cand, int wc,
                                                    const unsigned short* __restrict__ ref, int wr,
                                                    const int* __restrict__ cand_len, const int* __restrict__ ref_len,
                                                    int* __restrict__ out) {
  __shared__ u64 keys[2][MAXLEN];
  __shared__ unsigned short tok[2][MAXLEN + TOKPAD];
  __shared__ int red[4][5];
  const int tid = threadIdx.x, p = blockIdx.x;
  const int Lc = clamp_len(cand_len[p], wc), Lr = clamp_len(ref_len[p], wr);
  const int Lmax = Lc > Lr ? Lc : Lr;
  int n = 2;                                        // the sorted size: a power of two >= both lengths
  while (n < Lmax) n <<= 1;

  // token + 1 in 1..32768 (ids are taken modulo 2^15), 0 from the row's end on
  const unsigned short* crow = cand + (long long)p * wc;
  const unsigned short* rrow = ref + (long long)p * wr;
  for (int j = tid; j < n + TOKPAD; j += 256) {
    tok[0][j] = j < Lc ? (unsigned short)((crow[j] & 0x7fff) + 1) : (unsigned short)0;
    tok[1][j] = j < Lr ? (unsigned short)((rrow[j] & 0x7fff) + 1) : (unsigned short)0;
  }
  __syncthreads();
  int exact = 0;
  for (int j = tid; j < n; j += 256) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const unsigned short* t = tok[s] + j;
      const u64 k = ((u64)t[0] << 48) | ((u64)t[1] << 32) | ((u64)t[2] << 16) | (u64)t[3];
      keys[s][j] = j < (s ? Lr : Lc) ? k : ~0ull;    // the filler sorts behind every key (a field is at most 0x8000)
    }
    exact += (j < Lc && j < Lr && tok[0][j] == tok[1][j]) ? 1 : 0;
  }
  __syncthreads();

  // bitonic sort of both arrays, ascending: n / 2 compare-exchanges per array and pass
  const int half = n >> 1;
  for (int k = 2; k <= n; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < n; t += 256) {
        const int s = t >= half ? 1 : 0, u = t - s * half;
        const int i = 2 * u - (u & (j - 1)), q = i + j;
        const u64 a = keys[s][i], b = keys[s][q];
        const bool up = (i & k) == 0;
        if ((a > b) == up) keys[s][i] = b, keys[s][q] = a;
      }
      __syncthreads();
    }
  }

  int m[4] = {0, 0, 0, 0};
  const u64* A = keys[0];
  const u64* B = keys[1];
  for (int i = tid; i < Lc; i += 256) {
    const u64 key = A[i], before = i > 0 ? A[i - 1] : 0ull;
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      const int shift = 16 * (3 - o);
      const u64 pre = key >> shift;
      // complete (its last token exists) and the first of its run
      if ((pre & 0xffffu) != 0 && (i == 0 || (before >> shift) != pre)) {
        const int ca = bound<true>(A, i + 1, Lc, pre, shift) - i;
        const int lo = bound<false>(B, 0, Lr, pre, shift);
        const int cb = bound<true>(B, lo, Lr, pre, shift) - lo;
        m[o] += ca < cb ? ca : cb;
      }
    }
  }
  const int wave = tid >> 6, lane = tid & 63;
  int v[5] = {m[0], m[1], m[2], m[3], exact};
#pragma unroll
  for (int c = 0; c < 5; ++c) {
    v[c] = wave_sum_i(v[c]);
    if (lane == 0) red[wave][c] = v[c];
  }
  __syncthreads();
  if (tid < 5) out[(long long)p * 5 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// The recurrence of one pair in one wave with RC rows per lane (compile time: col[] and ctok[] must stay in registers;
// a loop that leaves early on a run-time row count is re-rolled by the compiler into indexed register moves, 4.5
// times slower at 2048 tokens). D[i][j], i = 0..Lc rows, j = 0..Lr columns, Lc, Lr >= 1, RC >= ceil(Lc / 64). Lane l owns rows
// l RC + 1 .. l RC + RC; col[k] is row l RC + k + 1 of the column it finished last (column 0 at the start:
// D[i][0] = i). Rows past Lc are computed and never read. Returns D[Lc][Lr] in lane (Lc - 1) / RC.
template <int RC>
__device__ __forceinline__ int strip_distance(const unsigned short* __restrict__ crow, int Lc,
                                              const unsigned short* rtok, int Lr, int lane) {
  const int row0 = lane * RC;
  int col[RC], ctok[RC];
#pragma unroll
  for (int k = 0; k < RC; ++k) {
    const int at = row0 + k;
    const int t = crow[at < Lc ? at : Lc - 1] & 0x7fff;     // unconditional loads: issued together
    col[k] = at + 1;
    ctok[k] = at < Lc ? t : -1;
  }
  int bottom = row0 + RC;                           // D[row0 + RC][column finished last]: lane l + 1 takes it as its top
  int prevtop = row0;                               // D[row0][j - 1]
  const int last_lane = (Lc - 1) / RC, steps = Lr + last_lane;
  for (int s = 0; s < steps; ++s) {
    const int j = s - lane + 1;                     // this lane's column in this step
    const int from_above = __shfl_up(bottom, 1, 64);
    if (j >= 1 && j <= Lr && lane <= last_lane) {
      const int top = lane == 0 ? j : from_above;
      const int rj = rtok[j - 1];
      int diag = prevtop, up = top;
#pragma unroll
      for (int k = 0; k < RC; ++k) {
        const int left = col[k];
        const int a = (left < up ? left : up) + 1, b = diag + (ctok[k] != rj ? 1 : 0);
        const int d = a < b ? a : b;
        diag = left, col[k] = d, up = d;
      }
      prevtop = top, bottom = up;
    }
  }
  const int kk = (Lc - 1) - last_lane * RC;
  int res = 0;
#pragma unroll
  for (int k = 0; k < RC; ++k) res = k == kk ? col[k] : res;
  return res;
}

// grid: ceil(P / 4), 4 waves, wave w of workgroup b owns pair 4 b + w. RCAP >= ceil(wc / 64): the most rows a lane can
// own at this matrix width. A pair runs at the smallest strip of the list below that covers its own length, so a short
// document in a wide matrix pays for its own length (at most 1.5 times the cells it needs).
template <int RCAP>
__global__ __launch_bounds__(256) void edit_kernel(const unsigned short* __restrict__ cand, int wc,
                                                   const unsigned short* __restrict__ ref, int wr,
                                                   const int* __restrict__ cand_len, const int* __restrict__ ref_len,
                                                   int P, int* __restrict__ out) {
  __shared__ unsigned short rtok[4][MAXLEN];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int p = blockIdx.x * 4 + wave;
  const bool live = p < P;                          // wave-uniform
  const int Lc = live ? clamp_len(cand_len[p], wc) : 0, Lr = live ? clamp_len(ref_len[p], wr) : 0;
  const unsigned short* rrow = ref + (long long)(live ? p : 0) * wr;
  for (int j = lane; j < Lr; j += 64) rtok[wave][j] = rrow[j] & 0x7fff;
  __syncthreads();                                  // the only barrier: every wave reads its own row from here on
  if (!live) return;
  if (Lc == 0 || Lr == 0) {
    if (lane == 0) out[p] = Lc + Lr;
    return;
  }
  const unsigned short* crow = cand + (long long)p * wc;
  const unsigned short* rt = rtok[wave];
  const int need = (Lc + 63) >> 6;                  // wave-uniform, <= RCAP
  int res;
#define SVAE_STRIP(RC)                                                 \
  if constexpr (RC <= RCAP) {                                          \
    if (need <= RC) {                                                  \
      res = strip_distance<RC>(crow, Lc, rt, Lr, lane);                \
      if (lane == (Lc - 1) / RC) out[p] = res;                         \
      return;                                                          \
    }                                                                  \
  }
  SVAE_STRIP(1) SVAE_STRIP(2) SVAE_STRIP(3) SVAE_STRIP(4) SVAE_STRIP(6) SVAE_STRIP(8) SVAE_STRIP(12) SVAE_STRIP(16)
  SVAE_STRIP(24) SVAE_STRIP(32)
#undef SVAE_STRIP
}

bool bad_args(const void* cand, int32_t wc, const void* ref, int32_t wr, const void* cl, const void* rl, int32_t P,
              const void* out) {
  return !cand || !ref || !cl || !rl || !out || P < 1 || wc < 1 || wc > MAXLEN || wr < 1 || wr > MAXLEN ||
         ((uintptr_t)cand & 1) || ((uintptr_t)ref & 1) || ((uintptr_t)cl & 3) || ((uintptr_t)rl & 3) ||
         ((uintptr_t)out & 3);
}

}  // namespace

SVAE_EXPORT int svae_ngram_overlap(const int16_t* cand, int32_t wc, const int16_t* ref, int32_t wr,
                                   const int32_t* cand_len, const int32_t* ref_len, int32_t P, int32_t* out,
                                   svae_stream_t stream) {
  if (bad_args(cand, wc, ref, wr, cand_len, ref_len, P, out)) return SVAE_EINVAL;
  hipLaunchKernelGGL(ngram_kernel, dim3(P), dim3(256), 0, (hipStream_t)stream, (const unsigned short*)cand, (int)wc,
                     (const unsigned short*)ref, (int)wr, cand_len, ref_len, out);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}

SVAE_EXPORT int svae_edit_distance(const int16_t* cand, int32_t wc, const int16_t* ref, int32_t wr,
                                   const int32_t* cand_len, const int32_t* ref_len, int32_t P, int32_t* out,
                                   svae_stream_t stream) {
  if (bad_args(cand, wc, ref, wr, cand_len, ref_len, P, out)) return SVAE_EINVAL;
  const dim3 grid((P + 3) / 4), block(256);
  hipStream_t s = (hipStream_t)stream;
  const unsigned short* c = (const unsigned short*)cand;
  const unsigned short* r = (const unsigned short*)ref;
  if (wc <= 128) hipLaunchKernelGGL(edit_kernel<2>, grid, block, 0, s, c, (int)wc, r, (int)wr, cand_len, ref_len, (int)P, out);
  else if (wc <= 512) hipLaunchKernelGGL(edit_kernel<8>, grid, block, 0, s, c, (int)wc, r, (int)wr, cand_len, ref_len, (int)P, out);
  else hipLaunchKernelGGL(edit_kernel<32>, grid, block, 0, s, c, (int)wc, r, (int)wr, cand_len, ref_len, (int)P, out);
  SVAE_LAUNCH_CHECK();
  return SVAE_OK;
}
