// FastSpeech2 prosody steering: the variance adaptor's two kernels of csrc/fs2_ops.hip, generalised, and the fit of
// an utterance to a given number of frames.  fp32 / int32 in the channel-major layout x[c][b][t]; the fit's arithmetic is double.
//   * fs2_variance_apply_kernel   per column (b, t): the value that is embedded -- forced, or prediction * scalar * the control of the
//                                 column's symbol -- written to used[b][t], and its bucket's embedding added to x.  ONE thread per column
//                                 and slice of 32 channels: the two binary searches (symbol, bucket) run once per slice instead of once
//                                 per channel, and the walk over c keeps the accesses along t coalesced.
//   * fs2_durations_ctl_kernel    fs2_durations_kernel with a control per symbol, and the un-rounded weights the fit apportions
//   * fs2_fit_durations_kernel    largest-remainder apportionment of target[b] frames over an item's symbols, one workgroup per item
#include <cfloat>
#include <cmath>

#include "common.h"
#include "evmi.h"

namespace evmi {

constexpr int kApplyChannels = 32;  // channels one thread of fs2_variance_apply_kernel walks
static_assert(EVMI_FS2_FIT_MAX_SYMBOLS * sizeof(double) <= 48 * 1024, "fs2_fit_durations_kernel keeps an item's remainders in LDS");

__global__ __launch_bounds__(256) void fs2_variance_apply_kernel(float* __restrict__ x, const float* __restrict__ pred,
                                                                const float* __restrict__ forced, int forced_stride,
                                                                const float* __restrict__ control, const int* __restrict__ cum,
                                                                const int* __restrict__ lens, const float* __restrict__ bins,
                                                                const float* __restrict__ table, float* __restrict__ used, int n_bins,
                                                                int B, int L, int n, int D, float scalar) {
  const int col = blockIdx.x * blockDim.x + threadIdx.x;  // B * n fits an int: checked on the host
  if (col >= B * n) return;
  const int t = col % n, b = col / n;
  float v = 0.f;
  if (t < lens[b]) {
    if (forced) {
      v = forced[(long long)b * forced_stride + t];
    } else {
      v = pred[col] * scalar;
      if (control) {
        int sym = t;
        if (cum) {  // first l with cum[b][l] > t: the symbol the length regulator put at frame t
          const int* cb = cum + (long long)b * L;
          int lo = 0, hi = L - 1;
          while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (cb[mid] > t) hi = mid; else lo = mid + 1;
          }
          sym = lo;
        }
        v *= control[(long long)b * L + sym];
      }
    }
  }
  int lo = 0, hi = n_bins - 1;  // bins has n_bins - 1 boundaries; the bucket = the number of them strictly below v
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (bins[mid] < v) lo = mid + 1; else hi = mid;
  }
  if (blockIdx.y == 0) used[col] = v;
  const int c0 = blockIdx.y * kApplyChannels, c1 = min(D, c0 + kApplyChannels);
  const float* row = table + (long long)lo * D;
  float* xc = x + (long long)c0 * B * n + col;
  for (int c = c0; c < c1; ++c, xc += (long long)B * n) *xc += row[c];
}

// dur[b][l] = l < len[b] ? (int)max(0, (rint(exp(log_d) - 1) * scalar) * control[b][l]) : 0 ; weights = the same without the rounding
__global__ void fs2_durations_ctl_kernel(const float* __restrict__ log_d, const int* __restrict__ lens, const float* __restrict__ control,
                                         int* __restrict__ dur, float* __restrict__ weights, int B, int L, float scalar) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= B * L) return;
  const int l = i % L, b = i / L;
  const bool live = l < lens[b];
  const float raw = expf(log_d[i]) - 1.f;
  float d = rintf(raw) * scalar;
  if (control) d *= control[i];
  d = fmaxf(d, 0.f);
  dur[i] = live ? (int)d : 0;
  if (weights) {
    float w = raw * scalar;
    if (control) w *= control[i];
    weights[i] = live ? fmaxf(w, 0.f) : 0.f;
  }
}

// One workgroup per item.  n and target are read into workgroup-uniform values first: every __syncthreads() below is reached by all
// 256 threads, whatever the item's length.  Thread i owns the symbols i, i + 256, ...; the remainders of the whole item live in LDS.
__global__ __launch_bounds__(256) void fs2_fit_durations_kernel(const float* __restrict__ weights, const int* __restrict__ lens,
                                                               const int* __restrict__ target, int* __restrict__ dur, int L) {
  __shared__ double rem[EVMI_FS2_FIT_MAX_SYMBOLS];
  __shared__ double red_d[256];
  __shared__ long long red_q[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(lens[b], 0), L), tgt = target[b];
  if (tgt <= 0) return;  // (uniform: the whole workgroup leaves, the row stays as it is)
  const float* w = weights + (long long)b * L;
  int* d = dur + (long long)b * L;
  // a weight below zero or NaN counts as 0, an infinite one as the largest finite float
  auto weight = [&](int l) { const float f = w[l]; return f > 0.f ? (double)fminf(f, FLT_MAX) : 0.0; };

  double s = 0.0;
  for (int l = tid; l < n; l += 256) s += weight(l);
  red_d[tid] = s;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if (tid < step) red_d[tid] += red_d[tid + step];
    __syncthreads();
  }
  const double S = red_d[0];
  const bool flat = !(S > 0.0);  // no weight anywhere: every symbol counts as 1

  long long qs = 0;
  for (int l = tid; l < n; l += 256) {
    const double xl = flat ? (double)tgt / (double)n : (weight(l) * (double)tgt) / S;
    const double q = floor(xl);
    rem[l] = xl - q;
    d[l] = (int)q;
    qs += (long long)q;
  }
  for (int l = n + tid; l < L; l += 256) d[l] = 0;
  red_q[tid] = qs;
  __syncthreads();
  for (int step = 128; step > 0; step >>= 1) {
    if (tid < step) red_q[tid] += red_q[tid + step];
    __syncthreads();
  }
  // Frames left over.  0 <= R <= n in every case: with x'_l the real value of w_l * target / S for the S that was computed, sum x'_l is
  // target * (1 + delta), |delta| <= n 2^-53, and the computed x_l has another floor than x'_l only where a whole number lies between the
  // two, i.e. frac(x'_l) is within 2^-51 target of 0 or of 1.  sum frac(x'_l) = j + target * delta for an integer j; m symbols rounded up
  // across a whole number force j >= m, m' rounded down across one force j <= n - m', and R = j - m + m'.  (n target 2^-51 < 1 holds for
  // n <= 4096 and an int target.)  So the floors never exceed the target and there is nothing to take back.
  const long long R = (long long)tgt - red_q[0];

  if (R > 0) {
    // the R symbols with the largest remainder get one frame more, ties to the lower index: symbol l's rank = how many come before it
    for (int l = tid; l < n; l += 256) {
      const double r = rem[l];
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        const double rj = rem[j];
        rank += (rj > r || (rj == r && j < l)) ? 1 : 0;
      }
      if (rank < R) d[l] += 1;  // (d[l] was written by this thread)
    }
  }
}

}  // namespace evmi

using namespace evmi;

#define EVMI_NONNULL(cond, what) \
  if (!(cond)) return fail(EVMI_ERR_INVALID_ARG, std::string(what) + ": null pointer")

extern "C" {

int evmi_fs2_variance_apply_f32(float* x_dev, const float* pred_dev, const float* forced_dev, int forced_stride, const float* control_dev,
                                const int* cum_dev, const int* lens_dev, const float* bins_dev, const float* table_dev, float* used_dev,
                                int n_bins, int B, int L, int n, int D, float scalar, void* stream) {
  EVMI_NONNULL(x_dev && lens_dev && bins_dev && table_dev && used_dev && (pred_dev || forced_dev), "fs2_variance_apply");
  if (n_bins < 2) return fail(EVMI_ERR_INVALID_ARG, "fs2_variance_apply: n_bins");
  if (B <= 0 || L <= 0 || n <= 0 || D <= 0) return fail(EVMI_ERR_INVALID_ARG, "fs2_variance_apply: shape");
  if (!cum_dev && L != n) return fail(EVMI_ERR_INVALID_ARG, "fs2_variance_apply: without cum the control is [B][n], so L must equal n");
  if (forced_dev && forced_stride < n) return fail(EVMI_ERR_INVALID_ARG, "fs2_variance_apply: forced_stride below n");
  if ((long long)B * n > 0x7fffffffll || (long long)B * L > 0x7fffffffll) return fail(EVMI_ERR_UNSUPPORTED, "fs2_variance_apply: B * n above 2^31 - 1");
  const dim3 grid((unsigned)(((long long)B * n + 255) / 256), (unsigned)((D + kApplyChannels - 1) / kApplyChannels));
  if (grid.y > 65535) return fail(EVMI_ERR_UNSUPPORTED, "fs2_variance_apply: grid limits");
  hipLaunchKernelGGL(fs2_variance_apply_kernel, grid, dim3(256), 0, (hipStream_t)stream, x_dev, pred_dev, forced_dev, forced_stride,
                     control_dev, cum_dev, lens_dev, bins_dev, table_dev, used_dev, n_bins, B, L, n, D, scalar);
  EVMI_LAUNCH_CHECK("fs2_variance_apply");
  return EVMI_OK;
}

int evmi_fs2_durations_ctl_i32(const float* log_d_dev, const int* lens_dev, const float* control_dev, int* dur_dev, float* weights_dev,
                               int B, int L, float scalar, void* stream) {
  EVMI_NONNULL(log_d_dev && lens_dev && dur_dev, "fs2_durations_ctl");
  if (B <= 0 || L <= 0 || (long long)B * L > 0x7fffffffll) return fail(EVMI_ERR_INVALID_ARG, "fs2_durations_ctl: shape");
  hipLaunchKernelGGL(fs2_durations_ctl_kernel, dim3((unsigned)(((long long)B * L + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                     log_d_dev, lens_dev, control_dev, dur_dev, weights_dev, B, L, scalar);
  EVMI_LAUNCH_CHECK("fs2_durations_ctl");
  return EVMI_OK;
}

int evmi_fs2_fit_durations_i32(const float* weights_dev, const int* lens_dev, const int* target_dev, int* dur_dev, int B, int L,
                               void* stream) {
  EVMI_NONNULL(weights_dev && lens_dev && target_dev && dur_dev, "fs2_fit_durations");
  if (B <= 0 || L <= 0) return fail(EVMI_ERR_INVALID_ARG, "fs2_fit_durations: shape");
  if (L > EVMI_FS2_FIT_MAX_SYMBOLS)
    return fail(EVMI_ERR_UNSUPPORTED, "fs2_fit_durations: L above EVMI_FS2_FIT_MAX_SYMBOLS = " + std::to_string(EVMI_FS2_FIT_MAX_SYMBOLS));
  hipLaunchKernelGGL(fs2_fit_durations_kernel, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, weights_dev, lens_dev, target_dev,
                     dur_dev, L);
  EVMI_LAUNCH_CHECK("fs2_fit_durations");
  return EVMI_OK;
}

}  // extern "C"
