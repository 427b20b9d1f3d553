// Mel-cepstral distortion along the dynamic-time-warping path: two time-major feature sequences a [B][Ta][M] and
// b [B][Tb][M] (a synthesized mel and its recording), a linear map basis [K][M] (a DCT), one workgroup per item over that item's own
// Na = clamp(a_lens[b], 0, Ta) and Nb = clamp(b_lens[b], 0, Tb) frames.  All arithmetic fp32:
//
//   ca[i][k] = sum_m fmaf(basis[k][m], a[i][m], acc)       m ascending from 0; cb likewise from b
//   c[i][j]  = sqrtf(s),  s = fmaf(d_k, d_k, s),  d_k = ca[i][k] - cb[j][k],  k ascending, s from 0
//   D[0][0]  = c[0][0];   D[i][j] = c[i][j] + best,  best = D[i-1][j-1] (+inf where it does not exist), then D[i-1][j] if strictly
//              smaller, then D[i][j-1] if strictly smaller
//   the path is read back from (Na - 1, Nb - 1) to (0, 0):  steps = its cells,  dist = scale * D_end / steps,  lo / hi [j] = its first and
//   last row in column j,  col[j] = scale * (sum_{i = lo .. hi} c[i][j], i ascending) / (hi - lo + 1)
//
// A cell is a pure function of its three predecessors, so the bits do not depend on the schedule.  The schedule (1024 threads):
//   1. cepstra: a thread forms whole rows, K accumulators in registers, the basis through uniform (scalar) loads; ca goes to LDS as
//      [Na][K | 1] floats (thread j reads row s - j: the odd stride keeps the 64 lanes on 64 banks), cb[j] stays in thread j's registers;
//   2. recurrence: anti-diagonal s = i + j is one step, thread j owns column j.  D[i-1][j] is the thread's own last value; D[i][j-1] is
//      what thread j - 1 wrote one step ago (two LDS rows, one LDS-only barrier a step); D[i-1][j-1] is the D[i][j-1] this thread read one
//      step ago.  One decision byte a cell is collected in LDS and leaves for the workspace every DTW_CHUNK diagonals, diagonal-major
//      ws[s][j];
//   3. read-back: chunks of diagonals come back through LDS and thread 0 walks them (as align_durations_kernel does), writing lo / hi;
//   4. col: thread j recomputes the costs of its column's path cells from ca and its cb.
// Every trip count of a loop that holds a barrier comes from Na and Nb alone.  The walker takes "left" in row 0 and "up" in column 0
// from the indices and reads any byte other than 1 (up) or 2 (left) as the diagonal: no value in a, b or the workspace, NaN included,
// moves it outside the item or keeps it from reaching (0, 0).  (A comparison with NaN is false: the diagonal stays.)
#include <cmath>

#include "common.h"
#include "evmi.h"

namespace evmi {

constexpr int DTW_THREADS = 1024;
constexpr int DTW_MAX_K = 24;
constexpr int DTW_MAX_TB = DTW_THREADS;    // thread j owns column j
constexpr int DTW_CHUNK = 32;              // diagonals of one flush / one read-back chunk
constexpr int DTW_LDS_BUDGET = 152 * 1024;  // of the 160 KiB of a compute unit
// LDS of a launch, in this order: rows [2][1024] floats (after the recurrence: lo, hi [1024] ints) | dec [DTW_CHUNK][1024] bytes |
// misc 16 bytes (D_end) | ca [Ta][K | 1] floats
constexpr int DTW_FIXED_BYTES = 2 * DTW_THREADS * 4 + DTW_CHUNK * DTW_THREADS + 16;

__host__ __device__ inline int dtw_ca_stride(int K) { return K | 1; }
__host__ __device__ inline int dtw_ws_stride(int Tb) { return (Tb + 15) & ~15; }  // bytes of a workspace diagonal: 16-byte vectors
inline int dtw_max_ta(int K) { return (DTW_LDS_BUDGET - DTW_FIXED_BYTES) / (4 * dtw_ca_stride(K)); }

template <int K>
__device__ __forceinline__ void dtw_cepstrum(const float* __restrict__ row, const float* __restrict__ basis, int M, float (&out)[K]) {
#pragma unroll
  for (int k = 0; k < K; ++k) out[k] = 0.f;
#pragma unroll 4
  for (int m = 0; m < M; ++m) {
    const float v = row[m];
#pragma unroll
    for (int k = 0; k < K; ++k) out[k] = fmaf(basis[k * M + m], v, out[k]);
  }
}

template <int K>
__device__ __forceinline__ float dtw_cost(const float* __restrict__ ca_row, const float (&cb)[K]) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float d = ca_row[k] - cb[k];
    s = fmaf(d, d, s);
  }
  return sqrtf(s);
}

template <int K>
__global__ __launch_bounds__(DTW_THREADS) void dtw_cepstral_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                                   const int* __restrict__ a_lens, const int* __restrict__ b_lens,
                                                                   const float* __restrict__ basis, float* __restrict__ dist,
                                                                   int* __restrict__ steps, int* __restrict__ lo, int* __restrict__ hi,
                                                                   float* __restrict__ col, unsigned char* __restrict__ ws, int Ta, int Tb,
                                                                   int M, float scale) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* rows = reinterpret_cast<float*>(smem);
  int* lohi = reinterpret_cast<int*>(smem);
  unsigned char* dec = smem + 2 * DTW_THREADS * 4;
  float* misc = reinterpret_cast<float*>(dec + DTW_CHUNK * DTW_THREADS);
  float* ca = misc + 4;
  constexpr int KS = K | 1;

  const int item = blockIdx.x, tid = threadIdx.x;
  const int Na = min(max(a_lens[item], 0), Ta), Nb = min(max(b_lens[item], 0), Tb);
  int* lo_row = lo + (long long)item * Tb;
  int* hi_row = hi + (long long)item * Tb;
  float* col_row = col + (long long)item * Tb;
  const bool empty = Na == 0 || Nb == 0;
  for (int j = (empty ? 0 : Nb) + tid; j < Tb; j += DTW_THREADS) {
    lo_row[j] = hi_row[j] = -1;
    col_row[j] = 0.f;
  }
  if (empty) {
    if (tid == 0) {
      dist[item] = NAN;
      steps[item] = 0;
    }
    return;
  }

  // 1. cepstra
  const float* ab = a + (long long)item * Ta * M;
  for (int i = tid; i < Na; i += DTW_THREADS) {
    float c[K];
    dtw_cepstrum<K>(ab + (long long)i * M, basis, M, c);
#pragma unroll
    for (int k = 0; k < K; ++k) ca[i * KS + k] = c[k];
  }
  const int j = tid;
  float cb[K];
  if (j < Nb) dtw_cepstrum<K>(b + ((long long)item * Tb + j) * M, basis, M, cb);
  else {
#pragma unroll
    for (int k = 0; k < K; ++k) cb[k] = 0.f;
  }
  __syncthreads();

  // 2. the recurrence over the anti-diagonals
  const int S = Na + Nb - 1;  // diagonals of the item
  const int Wp = dtw_ws_stride(Tb);
  unsigned char* wsb = ws + (long long)item * (Ta + Tb - 1) * Wp;
  float own = 0.f, left_prev = 0.f;  // D[i - 1][j]; the D[i - 1][j - 1] that was this thread's left neighbour one step ago
  for (int s0 = 0; s0 < S; s0 += DTW_CHUNK) {
    const int ns = min(DTW_CHUNK, S - s0);
    for (int ss = 0; ss < ns; ++ss) {
      const int s = s0 + ss, i = s - j;
      if (j < Nb && i >= 0 && i < Na) {
        const float c = dtw_cost<K>(ca + i * KS, cb);
        const float left = j > 0 ? rows[((s & 1) ^ 1) * DTW_THREADS + j - 1] : 0.f;
        float best = (i > 0 && j > 0) ? left_prev : INFINITY;
        unsigned char d = 0;
        if (i > 0 && own < best) {
          best = own;
          d = 1;
        }
        if (j > 0 && left < best) {
          best = left;
          d = 2;
        }
        own = s == 0 ? c : c + best;
        left_prev = left;
        rows[(s & 1) * DTW_THREADS + j] = own;
        dec[ss * DTW_THREADS + j] = d;
      }
      lds_barrier();
    }
    // the chunk's decisions -> workspace diagonals (4 bytes a store; cells outside the item hold whatever the LDS held)
    const int words = Wp >> 2;
    for (int e = tid; e < ns * words; e += DTW_THREADS) {
      const int ss = e / words, w = e - ss * words;
      *reinterpret_cast<unsigned*>(wsb + (long long)(s0 + ss) * Wp + 4 * w) = *reinterpret_cast<const unsigned*>(dec + ss * DTW_THREADS + 4 * w);
    }
    lds_barrier();  // the chunk is read before the next one's decisions land in it
  }
  if (j == Nb - 1) misc[0] = own;  // D[Na - 1][Nb - 1]
  __syncthreads();                 // every decision is in the workspace and visible to this workgroup; rows become lo / hi

  // 3. read-back: chunks of whole diagonals through LDS, walked by one thread
  int* los = lohi;
  int* his = lohi + DTW_THREADS;
  int wi = Na - 1, wj = Nb - 1, count = 1;  // (thread 0's)
  if (tid == 0) his[wj] = wi;
  for (int s1 = S; s1 > 0;) {
    const int nr = min(DTW_CHUNK, s1), sc = s1 - nr;
    const uint4* src = reinterpret_cast<const uint4*>(wsb + (long long)sc * Wp);
    for (int e = tid; e < (nr * Wp) >> 4; e += DTW_THREADS) reinterpret_cast<uint4*>(dec)[e] = src[e];
    __syncthreads();
    if (tid == 0) {
      while (wi + wj >= sc && (wi > 0 || wj > 0)) {
        unsigned char d = dec[(wi + wj - sc) * Wp + wj];
        if (wi == 0) d = 2;
        else if (wj == 0) d = 1;
        if (d == 1) --wi;
        else {
          los[wj] = wi;  // the walk leaves column wj
          if (d != 2) --wi;
          --wj;
          his[wj] = wi;
        }
        ++count;
      }
    }
    __syncthreads();
    s1 = sc;
  }
  if (tid == 0) {
    los[0] = 0;
    steps[item] = count;
    dist[item] = scale * misc[0] / (float)count;
  }
  __syncthreads();

  // 4. the path's mean cost of each column
  if (j < Nb) {
    const int l = min(max(los[j], 0), Na - 1), h = min(max(his[j], l), Na - 1);
    float sum = 0.f;
    for (int i = l; i <= h; ++i) sum += dtw_cost<K>(ca + i * KS, cb);
    lo_row[j] = l;
    hi_row[j] = h;
    col_row[j] = scale * sum / (float)(h - l + 1);
  }
}

}  // namespace evmi

using namespace evmi;

namespace {

// the refusals that the plan query and the call share; 0 where (K, Tb) is inside the limits
int dtw_check_limits(const char* who, int K, int Tb) {
  if (K > DTW_MAX_K) return fail(EVMI_ERR_UNSUPPORTED, std::string(who) + ": more than 24 cepstra (K)");
  if (Tb > DTW_MAX_TB) return fail(EVMI_ERR_UNSUPPORTED, std::string(who) + ": more than 1024 frames on the thread-owned side (Tb)");
  return EVMI_OK;
}

}  // namespace

extern "C" {

long long evmi_dtw_ws_bytes(int B, int Ta, int Tb) {
  if (B <= 0 || Ta <= 0 || Tb <= 0) return 0;
  return (long long)B * (Ta + Tb - 1) * dtw_ws_stride(Tb);
}

int evmi_dtw_plan(int K, int Tb, int* max_ta, int* diag_chunk) {
  if (!max_ta || !diag_chunk) return fail(EVMI_ERR_INVALID_ARG, "dtw_plan: null pointer");
  if (K <= 0 || Tb <= 0) return fail(EVMI_ERR_INVALID_ARG, "dtw_plan: shape");
  if (int rc = dtw_check_limits("dtw_plan", K, Tb)) return rc;
  *max_ta = dtw_max_ta(K);
  *diag_chunk = DTW_CHUNK;
  return EVMI_OK;
}

int evmi_dtw_cepstral_f32(const float* a_dev, const float* b_dev, const int* a_lens_dev, const int* b_lens_dev, const float* basis_dev,
                          float* dist_dev, int* steps_dev, int* lo_dev, int* hi_dev, float* col_dev, unsigned char* ws_dev, long long ws_bytes,
                          int B, int Ta, int Tb, int M, int K, float scale, void* stream) {
  if (!a_dev || !b_dev || !a_lens_dev || !b_lens_dev || !basis_dev || !dist_dev || !steps_dev || !lo_dev || !hi_dev || !col_dev || !ws_dev)
    return fail(EVMI_ERR_INVALID_ARG, "dtw_cepstral: null pointer");
  if (B <= 0 || Ta <= 0 || Tb <= 0 || M <= 0 || K <= 0) return fail(EVMI_ERR_INVALID_ARG, "dtw_cepstral: shape");
  if (int rc = dtw_check_limits("dtw_cepstral", K, Tb)) return rc;
  if (Ta > dtw_max_ta(K))
    return fail(EVMI_ERR_UNSUPPORTED, "dtw_cepstral: more than " + std::to_string(dtw_max_ta(K)) + " frames on the LDS-resident side (Ta) at K = " +
                                          std::to_string(K));
  if (ws_bytes < evmi_dtw_ws_bytes(B, Ta, Tb)) return fail(EVMI_ERR_INVALID_ARG, "dtw_cepstral: workspace too small");
  if ((uintptr_t)ws_dev & 15) return fail(EVMI_ERR_INVALID_ARG, "dtw_cepstral: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const size_t lds = DTW_FIXED_BYTES + (size_t)Ta * dtw_ca_stride(K) * 4;
  int rc = EVMI_OK;
#define EVMI_DTW(KK)                                                                                                                       \
  case KK:                                                                                                                                 \
    rc = launch_with_lds(dtw_cepstral_kernel<KK>, dim3(B), dim3(DTW_THREADS), lds, s, a_dev, b_dev, a_lens_dev, b_lens_dev, basis_dev, dist_dev, \
                         steps_dev, lo_dev, hi_dev, col_dev, ws_dev, Ta, Tb, M, scale);                                                    \
    break;
  switch (K) {
    EVMI_DTW(1) EVMI_DTW(2) EVMI_DTW(3) EVMI_DTW(4) EVMI_DTW(5) EVMI_DTW(6) EVMI_DTW(7) EVMI_DTW(8) EVMI_DTW(9) EVMI_DTW(10) EVMI_DTW(11)
    EVMI_DTW(12) EVMI_DTW(13) EVMI_DTW(14) EVMI_DTW(15) EVMI_DTW(16) EVMI_DTW(17) EVMI_DTW(18) EVMI_DTW(19) EVMI_DTW(20) EVMI_DTW(21)
    EVMI_DTW(22) EVMI_DTW(23) EVMI_DTW(24)
  }
#undef EVMI_DTW
  if (rc) return rc;
  EVMI_LAUNCH_CHECK("dtw_cepstral");
  return EVMI_OK;
}

}  // extern "C"
