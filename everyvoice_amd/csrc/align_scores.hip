// Alignment scores: how well the aligner's soft attention agrees with a duration row, per utterance and per
// symbol, from the same projected mel q [A][B][T] and text k [A][B][L] that align_infer.hip searches.  One workgroup per item over that
// item's own T_b frames and L_b symbols, no workspace in global memory.
//
//   logit[y][x] = -temperature * sum_a (q[a][y] - k[a][x])^2                          fp32, a ascending, fmaf, all x < L_b
//   lp[y][x]    = logit - lse_x(logit) + logf((float)prior[y][x] + 1e-8f)             (without a prior: lp = logit)
//   ctc[b]      = CTC forward-sum loss over log_softmax([blank_logprob, lp[y][0 .. L_b)]), targets 1 .. L_b, divided by L_b
//   path[b]     = -(1 / T_b) * sum_y max(lp[y][p(y)] - lse_x(lp[y]), logf(1e-12f))    p: symbol x holds dur[b][x] consecutive frames
//   symbol[b][x]= mean of the same term over symbol x's own frames
//
// The frames go through the workgroup (1024 threads) in tiles of TY frames, as many as the LDS holds at the launch's L and A:
//   1. the tile's q columns are staged in LDS;
//   2. value pass, as align_durations_kernel's with full rows: units of 64 symbols x 8 frames dealt round-robin to the 16 waves;
//   3. row pass: a wave owns a frame: lse_x(logit), the prior (read here, a row at a time), lse_x(lp); a lane keeps its own columns
//      from pass to pass, so the rows need no barrier in between;
//   4. lattice: frames in sequence, thread x owns symbol x and the blank in front of it; its left neighbour's symbol state arrives
//      through two LDS rows, one LDS-only barrier a frame; the trailing blank rides with thread L_b - 1.  In the same loop thread x adds
//      the path term of the frames its own symbol holds, in frame order.
// Every reduction's order depends on L_b and T_b alone, so an item's outputs are the same bits alone and in any batch.
#include <cmath>

#include "common.h"
#include "evmi.h"

namespace evmi {

constexpr int AS_THREADS = 1024;
constexpr int AS_WAVES = AS_THREADS / 64;
constexpr int AS_FPT = 8;  // frames of one unit of the value pass
constexpr int AS_MAX_A = 128;
constexpr int AS_MAX_L = AS_THREADS - 1;  // evmi_forward_sum_grad_f32's limit
constexpr int AS_MAX_TY = 64;
constexpr int AS_LDS_BUDGET = 152 * 1024;  // of the 160 KiB of a compute unit
constexpr int AS_MISC_BYTES = AS_THREADS * 8;
typedef float as_f32x2 __attribute__((ext_vector_type(2)));

// LDS of a launch, in this order:
//   misc 8 KiB (prefix sum of the durations; then the lattice's rows [2][VS] floats; then the final sum) | vals [TY][VS] floats |
//   qs [A][TY] floats | lses [2][TY] floats | (ks [A][VS] floats)
struct AsPlan {
  int ty, vs;
  bool k_in_lds;
  size_t bytes;
};
inline AsPlan as_plan(int A, int L) {
  AsPlan p;
  p.vs = (L + 63) & ~63;
  const size_t per_frame = (size_t)4 * p.vs + 4 * A + 8, ks = (size_t)A * p.vs * 4;
  auto frames = [&](size_t fixed) { return fixed >= (size_t)AS_LDS_BUDGET ? 0 : (int)min((size_t)AS_MAX_TY, (AS_LDS_BUDGET - fixed) / per_frame) & ~7; };
  p.k_in_lds = frames(AS_MISC_BYTES + ks) >= 32;  // (a smaller tile costs more than reading k through the caches)
  p.ty = frames(AS_MISC_BYTES + (p.k_in_lds ? ks : 0));
  p.bytes = AS_MISC_BYTES + (p.k_in_lds ? ks : 0) + (size_t)p.ty * per_frame;
  return p;
}

// log(exp(a) + exp(b) (+ exp(c))) with one logarithm and no branch: a lattice state that no path has reached holds -inf, and so does a
// sum of such states (the shift is 0 there: expf(-inf) = 0, logf(0) = -inf)
__device__ __forceinline__ float as_lse2(float a, float b) {
  const float m = fmaxf(a, b), shift = m == -INFINITY ? 0.f : m;
  return shift + logf(expf(a - shift) + expf(b - shift));
}
__device__ __forceinline__ float as_lse3(float a, float b, float c) {
  const float m = fmaxf(fmaxf(a, b), c), shift = m == -INFINITY ? 0.f : m;
  return shift + logf(expf(a - shift) + expf(b - shift) + expf(c - shift));
}

template <bool KLDS>
__global__ __launch_bounds__(AS_THREADS) void align_scores_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                  const double* __restrict__ prior, const int* __restrict__ text_lens,
                                                                  const int* __restrict__ mel_lens, const int* __restrict__ dur,
                                                                  float* __restrict__ ctc, float* __restrict__ path, float* __restrict__ symbol,
                                                                  int A, int B, int T, int L, int TY, int VS, float temperature,
                                                                  float blank_logprob) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  long long* scan = reinterpret_cast<long long*>(smem);
  float* rows = reinterpret_cast<float*>(smem);
  float* vals = reinterpret_cast<float*>(smem + AS_MISC_BYTES);
  float* qs = vals + TY * VS;
  float* lses = qs + A * TY;  // [0][yy] = lse_x(lp), [1][yy] = logaddexp(blank_logprob, lse_x(lp))
  float* ks = lses + 2 * TY;

  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lb = min(max(text_lens[b], 0), L), Tb = min(max(mel_lens[b], 0), T);
  float* srow = symbol + (long long)b * L;
  if (Lb == 0 || Tb == 0 || Tb < Lb) {  // no path uses every symbol
    for (int l = tid; l < L; l += AS_THREADS) srow[l] = 0.f;
    if (tid == 0) ctc[b] = path[b] = NAN;
    return;
  }
  for (int l = Lb + tid; l < L; l += AS_THREADS) srow[l] = 0.f;

  const int WX = (Lb + 63) >> 6;  // waves across the item's symbols
  const int lane = tid & 63, wave = tid >> 6;
  const float* kb = k + (long long)b * L;
  const float LOG_FLOOR = logf(1e-12f);

  // the frames of symbol x = tid: [first, first + count) from an inclusive prefix sum of the duration row.  An entry outside [0, T_b]
  // counts as T_b + 1: the row's sum then misses T_b whatever the others hold, and no sum leaves 64 bits
  const long long d_own = tid < Lb ? (long long)dur[(long long)b * L + tid] : 0;
  scan[tid] = (d_own < 0 || d_own > Tb) ? (long long)Tb + 1 : d_own;
  __syncthreads();
  for (int step = 1; step < AS_THREADS; step <<= 1) {
    const long long add = tid >= step ? scan[tid - step] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const bool row_ok = scan[AS_THREADS - 1] == (long long)Tb;  // (workgroup-uniform)
  const int count = row_ok && tid < Lb ? (int)d_own : 0;
  const int first = row_ok && tid < Lb ? (int)(scan[tid] - d_own) : 0;
  __syncthreads();  // the scan is read: the region becomes the lattice's rows

  if (KLDS) {
    for (int i = tid; i < A * VS; i += AS_THREADS) {
      const int a = i / VS, x = i - a * VS;
      ks[i] = x < Lb ? kb[(long long)a * B * L + x] : 0.f;
    }
  }

  float s_own = -INFINITY, b_own = -INFINITY, b_last = -INFINITY;  // symbol tid, the blank in front of it, the trailing blank
  float acc = 0.f;                                                 // path terms of this symbol's frames so far

  for (int y0 = 0; y0 < Tb; y0 += TY) {
    const int ny = min(TY, Tb - y0);
    // 1. q columns of the tile: qs[a][yy]
    for (int i = tid; i < A * TY; i += AS_THREADS) {
      const int a = i / TY, yy = i - a * TY;
      qs[i] = yy < ny ? q[((long long)a * B + b) * T + y0 + yy] : 0.f;
    }
    __syncthreads();  // (also: the previous tile's lattice has read vals and lses; the k image has landed)
    // 2. logits of the tile: unit u = (frame group g, symbol wave) -> wave u % 16
    const int units = ((ny + AS_FPT - 1) / AS_FPT) * WX;
    for (int u = wave; u < units; u += AS_WAVES) {
      const int g = u / WX, x = (u - g * WX) * 64 + lane;
      if (x >= Lb) continue;
      as_f32x2 sum[AS_FPT / 2];
#pragma unroll
      for (int f = 0; f < AS_FPT / 2; ++f) sum[f] = as_f32x2{0.f, 0.f};
      const float* qrow = qs + g * AS_FPT;
#pragma unroll 4
      for (int a = 0; a < A; ++a) {
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(qrow + a * TY), q1 = *reinterpret_cast<const f32x4*>(qrow + a * TY + 4);
        const as_f32x2 qp[4] = {as_f32x2{q0[0], q0[1]}, as_f32x2{q0[2], q0[3]}, as_f32x2{q1[0], q1[1]}, as_f32x2{q1[2], q1[3]}};
        const float kv = KLDS ? ks[a * VS + x] : kb[(long long)a * B * L + x];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const as_f32x2 d = qp[f] - kv;
          sum[f] = __builtin_elementwise_fma(d, d, sum[f]);  // per element fmaf(d, d, sum): two frames an instruction
        }
      }
#pragma unroll
      for (int f = 0; f < AS_FPT; ++f) {
        const int yy = g * AS_FPT + f;
        if (yy < ny) vals[yy * VS + x] = -temperature * sum[f >> 1][f & 1];
      }
    }
    __syncthreads();
    // 3. rows: wave w owns frames w, w + 16, ... of the tile; lane l owns columns l, l + 64, ... in every pass
    for (int yy = wave; yy < ny; yy += AS_WAVES) {
      float* row = vals + yy * VS;
      auto row_lse = [&]() {
        float m = -INFINITY;
        for (int x = lane; x < Lb; x += 64) m = fmaxf(m, row[x]);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        float s = 0.f;
        for (int x = lane; x < Lb; x += 64) s += expf(row[x] - m);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
        return m + logf(s);
      };
      float lse = row_lse();
      if (prior) {
        const double* prow = prior + ((long long)b * T + y0 + yy) * L;
        for (int x = lane; x < Lb; x += 64) {
#pragma clang fp contract(off)
          row[x] = row[x] - lse + logf((float)prow[x] + 1e-8f);
        }
        lse = row_lse();
      }
      if (lane == 0) {
        lses[yy] = lse;
        lses[TY + yy] = as_lse2(blank_logprob, lse);
      }
    }
    __syncthreads();
    // 4. the lattice over the tile's frames, and the path terms of this thread's symbol
    for (int yy = 0; yy < ny; ++yy) {
      const int y = y0 + yy, x = tid;
      float* cur = rows + (y & 1) * VS;
      const float* prev = rows + ((y & 1) ^ 1) * VS;
      if (x < Lb) {
        const float v = vals[yy * VS + x], norm = lses[TY + yy];
        const float lp_x = v - norm, lp_blank = blank_logprob - norm;
        if (y == 0) {
          b_own = x == 0 ? lp_blank : -INFINITY;
          s_own = x == 0 ? lp_x : -INFINITY;
        } else {
          const float left = x == 0 ? -INFINITY : prev[x - 1];
          if (x == Lb - 1) b_last = lp_blank + as_lse2(b_last, s_own);
          const float s_new = lp_x + as_lse3(s_own, b_own, left);
          b_own = lp_blank + as_lse2(b_own, left);
          s_own = s_new;
        }
        cur[x] = s_own;
        if (y >= first && y - first < count) acc += fmaxf(v - lses[yy], LOG_FLOOR);
      }
      lds_barrier();
    }
  }
  __syncthreads();  // the lattice's rows are read: the region becomes the final sum

  if (tid == Lb - 1) {
    const float ll = as_lse2(b_last, s_own);
    ctc[b] = ll == -INFINITY ? 0.f : -ll / (float)Lb;  // (zero_infinity, as evmi_forward_sum_loss_f32)
  }
  if (tid < Lb) srow[tid] = row_ok && count > 0 ? acc / (float)count : NAN;
  float* part = reinterpret_cast<float*>(smem);
  part[tid] = acc;  // (0 beyond L_b)
  __syncthreads();
  for (int step = AS_THREADS / 2; step > 0; step >>= 1) {
    if (tid < step) part[tid] += part[tid + step];
    __syncthreads();
  }
  if (tid == 0) path[b] = row_ok ? -part[0] / (float)Tb : NAN;
}

}  // namespace evmi

using namespace evmi;

extern "C" {

int evmi_align_scores_plan(int A, int L, int* frame_tile, int* k_in_lds) {
  if (!frame_tile || !k_in_lds) return fail(EVMI_ERR_INVALID_ARG, "align_scores_plan: null pointer");
  if (A <= 0 || L <= 0) return fail(EVMI_ERR_INVALID_ARG, "align_scores_plan: shape");
  if (A > AS_MAX_A) return fail(EVMI_ERR_UNSUPPORTED, "align_scores_plan: more than 128 attention channels");
  if (L > AS_MAX_L) return fail(EVMI_ERR_UNSUPPORTED, "align_scores_plan: more than 1023 symbols");
  const AsPlan p = as_plan(A, L);
  *frame_tile = p.ty;
  *k_in_lds = p.k_in_lds ? 1 : 0;
  return EVMI_OK;
}

int evmi_align_scores_f32(const float* q_dev, const float* k_dev, const double* prior_dev, const int* text_lens_dev, const int* mel_lens_dev,
                          const int* dur_dev, float* ctc_dev, float* path_dev, float* symbol_dev, int A, int B, int T, int L,
                          float temperature, float blank_logprob, void* stream) {
  if (!q_dev || !k_dev || !text_lens_dev || !mel_lens_dev || !dur_dev || !ctc_dev || !path_dev || !symbol_dev)
    return fail(EVMI_ERR_INVALID_ARG, "align_scores: null pointer");
  if (A <= 0 || B <= 0 || T <= 0 || L <= 0) return fail(EVMI_ERR_INVALID_ARG, "align_scores: shape");
  if (A > AS_MAX_A) return fail(EVMI_ERR_UNSUPPORTED, "align_scores: more than 128 attention channels");
  if (L > AS_MAX_L) return fail(EVMI_ERR_UNSUPPORTED, "align_scores: more than 1023 symbols");
  hipStream_t s = (hipStream_t)stream;
  const AsPlan p = as_plan(A, L);
  int rc;
#define EVMI_AS(KL)                                                                                                            \
  rc = launch_with_lds(align_scores_kernel<KL>, dim3(B), dim3(AS_THREADS), p.bytes, s, q_dev, k_dev, prior_dev, text_lens_dev, \
                       mel_lens_dev, dur_dev, ctc_dev, path_dev, symbol_dev, A, B, T, L, p.ty, p.vs, temperature, blank_logprob)
  if (p.k_in_lds) EVMI_AS(true);
  else EVMI_AS(false);
#undef EVMI_AS
  if (rc) return rc;
  EVMI_LAUNCH_CHECK("align_scores");
  return EVMI_OK;
}

}  // extern "C"
