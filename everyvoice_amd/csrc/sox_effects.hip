// SoX effect chains of the preprocessor on the device (everyvoice/preprocessor/preprocessor.py:187-194 hands a
// dataset's sox_effects to SoX before resampling).  `norm` is evmi_peak_normalize_f32 (preprocess_ops.hip); this file holds
// `reverse` and SoX 14.4's `silence` on a zero-padded batch x [items][t_max] with lengths [items] on the device.
//
// silence (the rules, restated sample by sample in tests/sox_oracle.py): samples on SoX's int32 scale s = x * 2^31; the RMS at
// sample i covers the last W = rate / 50 samples, i included (missing ones count as zero, the divisor is always W):
// rms = (int32) sqrt(sum / W); a sample is "above" a threshold when rms >= rms_min (the host turns the % / dB test into that
// integer, rms_min, so the device runs no transcendental of its own).  Leading trim: drop samples until D_start consecutive
// samples are above the start threshold, output starts at the first of them.  Stop part: while copying, a run of D_stop
// consecutive samples below the stop threshold is discarded; below_periods 1 ends the output there, -1 clears the window and
// runs the leading trim again from the next sample.  Three kernels:
//   (a) flags, batch-wide: every sample's window sum in fp64 from 64-sample prefix sums (a wave scan per 64 samples; the window
//       adds the whole 64-sample totals between its two ends), so rounding is relative to one window's energy.  Squares of fp32
//       samples are exact in fp64 and, on the 16-bit grid (k << 16, k^2 < 2^30), every partial sum is an exact integer times
//       2^32 far below 2^53: the sums, hence the decisions, equal SoX's running double sum bit for bit.  One bit per sample per
//       threshold (__ballot, 64-bit words).
//   (b) walk, one wave per utterance: runs found word by word (count-trailing-zeros over the bit masks); after a restart the
//       W - 1 flags the cleared window changes are recomputed (a wave scan from the restart point) into LDS copies of their words.
//       It writes the kept intervals (source start, output start, length) and the new length.
//   (c) gather: output sample -> its interval (binary search) -> source sample; optionally in reverse order, so that
//       `silence, reverse` is one pass.
// Interval bound: every kept piece but the last ends where a discarded run of D_stop samples starts, so an utterance has at
// most t_max / D_stop + 1 of them (one without a stop part); the workspace holds t_max / D_stop + 2 per utterance.
#include "common.h"

namespace evmi {

constexpr int kSoxTile = 1024;        // samples per flags workgroup: 16 words, 4 waves x 4
constexpr int kSoxMaxWindow = 4096;   // W = rate / 50: rates up to 204.8 kHz
constexpr int kSoxRampWords = kSoxMaxWindow / 64 + 2;

__device__ __forceinline__ long long sox_rms(double sum, int window) {
  const double q = sqrt(fmax(sum, 0.0) / (double)window);
  return q >= 2147483647.0 ? 2147483647LL : (long long)q;  // (int32) truncation, clamped where 2^31 would overflow
}

// inclusive prefix of v over the 64 lanes of a wave
__device__ __forceinline__ double wave_scan(double v, int lane) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const double u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

// (a) grid (ceil(t_max / kSoxTile), items), 256 threads; LDS: 64-sample prefix sums of every 64-sample group a window of the tile touches
__global__ __launch_bounds__(256) void sox_silence_flags_kernel(const float* __restrict__ x, const int* __restrict__ lens, uint64_t* __restrict__ f_start,
                                                                uint64_t* __restrict__ f_stop, int t_max, int words, int window, long long r_start,
                                                                long long r_stop) {
  extern __shared__ double pre[];
  const int item = blockIdx.y;
  const int n = min(lens[item], t_max);
  const int w0 = blockIdx.x * (kSoxTile / 64);
  const int nw = min(kSoxTile / 64, words - w0);
  uint64_t* fs = f_start + (long long)item * words;
  uint64_t* fp = f_stop + (long long)item * words;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (w0 * 64 >= n) {
    for (int w = threadIdx.x; w < nw; w += 256) fs[w0 + w] = fp[w0 + w] = 0ull;
    return;
  }
  const int g_lo = max(0, w0 * 64 - window + 1) >> 6;
  const int g_hi = min(w0 + nw, (n + 63) >> 6);
  const float* xs = x + (long long)item * t_max;
  for (int g = g_lo + wave; g < g_hi; g += 4) {
    const int t = g * 64 + lane;
    const double s = t < n ? (double)xs[t] * 2147483648.0 : 0.0;
    pre[(g - g_lo) * 64 + lane] = wave_scan(s * s, lane);
  }
  __syncthreads();
  for (int g = w0 + wave; g < w0 + nw; g += 4) {
    const int i = g * 64 + lane;
    bool a_start = false, a_stop = false;
    if (i < n) {
      const int j0 = max(0, i - window + 1), g0 = j0 >> 6;
      const double* p = pre;  // (group h's prefix sums start at (h - g_lo) * 64)
      const int b = (g0 - g_lo) * 64;
      double sum = (g0 == g ? p[(g - g_lo) * 64 + (i & 63)] : p[b + 63]) - ((j0 & 63) ? p[b + (j0 & 63) - 1] : 0.0);
      if (g0 != g) {
        for (int h = g0 + 1; h < g; ++h) sum += p[(h - g_lo) * 64 + 63];
        sum += p[(g - g_lo) * 64 + (i & 63)];
      }
      const long long rms = sox_rms(sum, window);
      a_start = rms >= r_start;
      a_stop = rms >= r_stop;
    }
    const uint64_t bs = __ballot(a_start), bp = __ballot(a_stop);
    if (lane == 0) {
      fs[g] = bs;
      fp[g] = bp;
    }
  }
}

__device__ __forceinline__ uint64_t sox_word(const uint64_t* g, const uint64_t* ramp, int k_lo, int k_hi, int k) {
  return (k >= k_lo && k < k_hi) ? ramp[k - k_lo] : g[k];
}

// start of the first run of d consecutive samples in [p, n) whose flag equals `want`, or -1
__device__ int sox_find_run(const uint64_t* g, const uint64_t* ramp, int k_lo, int k_hi, int p, int n, int d, bool want) {
  int run = 0, start = p, q = p;
  while (q < n) {
    const int off = q & 63, avail = min(64 - off, n - q);
    uint64_t w = sox_word(g, ramp, k_lo, k_hi, q >> 6);
    if (!want) w = ~w;
    w >>= off;
    if (avail < 64) w &= (1ull << avail) - 1ull;
    if (w & 1ull) {
      const uint64_t nw = ~w;
      const int ones = min(avail, nw ? (int)__builtin_ctzll(nw) : 64);
      if (run == 0) start = q;
      run += ones;
      q += ones;
      if (run >= d) return start;
    } else {
      run = 0;
      q += w ? min(avail, (int)__builtin_ctzll(w)) : avail;
    }
  }
  return -1;
}

// (b) one wave per utterance.  Every lane runs the same (uniform) walk; lane 0 writes.  iv [items][max_iv][3]: source start, output
// start, length.  lens is rewritten with the kept length.
__global__ __launch_bounds__(64) void sox_silence_walk_kernel(const float* __restrict__ x, int* __restrict__ lens, const uint64_t* __restrict__ f_start,
                                                              const uint64_t* __restrict__ f_stop, int* __restrict__ ivals, int* __restrict__ n_ivals,
                                                              int t_max, int words, int max_iv, int window, int above, int d_start, long long r_start,
                                                              int below, int d_stop, long long r_stop) {
  __shared__ uint64_t ramp[2][kSoxRampWords];
  const int item = blockIdx.x, lane = threadIdx.x;
  const int n = min(lens[item], t_max);
  const uint64_t* fs = f_start + (long long)item * words;
  const uint64_t* fp = f_stop + (long long)item * words;
  const float* xs = x + (long long)item * t_max;
  int* iv = ivals + (long long)item * max_iv * 3;
  int k_lo = 0, k_hi = 0;  // words [k_lo, k_hi) are read from `ramp` (the flags after the last restart)
  int pos = 0, copy_from = 0, out = 0, count = 0;
  bool trimming = above == 1;
  while (pos < n) {
    if (trimming) {
      const int s = sox_find_run(fs, ramp[0], k_lo, k_hi, pos, n, d_start, true);
      if (s < 0) break;
      copy_from = s;
      pos = s + d_start;
      trimming = false;
    }
    const int r = below ? sox_find_run(fp, ramp[1], k_lo, k_hi, pos, n, d_stop, false) : -1;
    const int end = r < 0 ? n : r;
    if (end > copy_from && count < max_iv) {
      if (lane == 0) {
        iv[3 * count] = copy_from;
        iv[3 * count + 1] = out;
        iv[3 * count + 2] = end - copy_from;
      }
      out += end - copy_from;
      ++count;
    }
    if (r < 0 || below == 1) break;
    // restart: the window is cleared after sample r + d_stop - 1; the next W - 1 samples see only what came after it
    pos = r + d_stop;
    copy_from = pos;
    trimming = above == 1;
    if (pos >= n) break;
    const int r_end = min(pos + window - 1, n);
    __syncthreads();  // (every lane is done reading the previous ramp)
    k_lo = pos >> 6;
    k_hi = r_end > pos ? ((r_end - 1) >> 6) + 1 : k_lo;
    for (int k = lane; k < k_hi - k_lo; k += 64) {
      ramp[0][k] = fs[k_lo + k];
      ramp[1][k] = fp[k_lo + k];
    }
    __syncthreads();
    double carry = 0.0;
    for (int c = pos; c < r_end; c += 64) {
      const int i = c + lane;
      const bool valid = i < r_end;
      const double s = valid ? (double)xs[i] * 2147483648.0 : 0.0;
      const double v = wave_scan(s * s, lane) + carry;
      carry = __shfl(v, 63, 64);
      const long long rms = sox_rms(v, window);
      const uint64_t m = __ballot(valid), b0 = __ballot(valid && rms >= r_start), b1 = __ballot(valid && rms >= r_stop);
      if (lane == 0) {
        const int kk = (c >> 6) - k_lo, o = c & 63;
        ramp[0][kk] = (ramp[0][kk] & ~(m << o)) | (b0 << o);
        ramp[1][kk] = (ramp[1][kk] & ~(m << o)) | (b1 << o);
        if (o && kk + 1 < k_hi - k_lo) {
          ramp[0][kk + 1] = (ramp[0][kk + 1] & ~(m >> (64 - o))) | (b0 >> (64 - o));
          ramp[1][kk + 1] = (ramp[1][kk + 1] & ~(m >> (64 - o))) | (b1 >> (64 - o));
        }
      }
    }
    __syncthreads();
  }
  if (lane == 0) {
    lens[item] = out;
    n_ivals[item] = count;
  }
}

// (c) grid (ceil(t_max / 256), items): y[t] = the t-th kept sample (the (len - 1 - t)-th when reverse), zeros behind the new length
__global__ __launch_bounds__(256) void sox_gather_kernel(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ lens,
                                                         const int* __restrict__ ivals, const int* __restrict__ n_ivals, int t_max, int max_iv,
                                                         int reverse) {
  const int item = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= t_max) return;
  const int n = min(lens[item], t_max);
  float v = 0.f;
  if (t < n) {
    const int o = reverse ? n - 1 - t : t;
    const int* iv = ivals + (long long)item * max_iv * 3;
    int lo = 0, hi = n_ivals[item] - 1;  // the last interval whose output start is <= o
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (iv[3 * mid + 1] <= o) lo = mid;
      else hi = mid - 1;
    }
    v = x[(long long)item * t_max + iv[3 * lo] + (o - iv[3 * lo + 1])];
  }
  y[(long long)item * t_max + t] = v;
}

__global__ __launch_bounds__(256) void sox_reverse_kernel(const float* __restrict__ x, float* __restrict__ y, const int* __restrict__ lens, int t_max) {
  const int item = blockIdx.y;
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= t_max) return;
  const int n = min(lens[item], t_max);
  const long long row = (long long)item * t_max;
  y[row + t] = t < n ? x[row + n - 1 - t] : 0.f;
}

struct SoxWorkspace {
  long long words, max_iv, flag_bytes, iv_bytes, total;
};

static SoxWorkspace sox_workspace(int items, int t_max, int stop_duration) {
  SoxWorkspace w;
  w.words = ((long long)t_max + 63) / 64;
  w.max_iv = (stop_duration > 0 ? t_max / stop_duration : 0) + 2;
  w.flag_bytes = (long long)items * w.words * 8;
  w.iv_bytes = ((long long)items * w.max_iv * 3 * 4 + 7) / 8 * 8;
  w.total = 2 * w.flag_bytes + w.iv_bytes + (long long)items * 4;
  return w;
}

}  // namespace evmi

using namespace evmi;

extern "C" {

long long evmi_sox_silence_ws_bytes(int items, int t_max, int window, int stop_duration) {
  if (items <= 0 || t_max <= 0 || window <= 0 || window > kSoxMaxWindow || stop_duration < 0) return 0;
  return sox_workspace(items, t_max, stop_duration).total;
}

int evmi_sox_silence_f32(const float* x_dev, float* y_dev, int* lens_dev, void* ws_dev, long long ws_bytes, int items, int t_max, int window,
                         int above_periods, int start_duration, long long start_rms_min, int below_periods, int stop_duration,
                         long long stop_rms_min, int reverse, void* stream) {
  if (!x_dev || !y_dev || !lens_dev || !ws_dev || x_dev == y_dev) return fail(EVMI_ERR_INVALID_ARG, "sox_silence: pointers (y must not alias x)");
  if (items <= 0 || items > 65535 || t_max <= 0 || window <= 0 || window > kSoxMaxWindow)
    return fail(EVMI_ERR_INVALID_ARG, "sox_silence: shape (items 1..65535, window 1.." + std::to_string(kSoxMaxWindow) + ")");
  if ((above_periods != 0 && above_periods != 1) || (above_periods == 1 && start_duration < 1) ||
      (below_periods != 0 && below_periods != 1 && below_periods != -1) || (below_periods != 0 && stop_duration < 1) ||
      start_rms_min < 0 || stop_rms_min < 0)
    return fail(EVMI_ERR_INVALID_ARG, "sox_silence: periods / durations / thresholds");
  const SoxWorkspace w = sox_workspace(items, t_max, below_periods ? stop_duration : 0);
  if (ws_bytes < w.total) return fail(EVMI_ERR_INVALID_ARG, "sox_silence: workspace smaller than evmi_sox_silence_ws_bytes");
  char* base = (char*)ws_dev;
  uint64_t* f_start = (uint64_t*)base;
  uint64_t* f_stop = (uint64_t*)(base + w.flag_bytes);
  int* ivals = (int*)(base + 2 * w.flag_bytes);
  int* n_ivals = (int*)(base + 2 * w.flag_bytes + w.iv_bytes);
  hipStream_t s = (hipStream_t)stream;
  const int words = (int)w.words;
  const size_t lds = (size_t)(kSoxTile / 64 + (window + 63) / 64 + 1) * 64 * sizeof(double);
  if (int rc = launch_with_lds(sox_silence_flags_kernel, dim3((t_max + kSoxTile - 1) / kSoxTile, items), dim3(256), lds, s, x_dev, (const int*)lens_dev,
                               f_start, f_stop, t_max, words, window, start_rms_min, stop_rms_min))
    return rc;
  hipLaunchKernelGGL(sox_silence_walk_kernel, dim3(items), dim3(64), 0, s, x_dev, lens_dev, (const uint64_t*)f_start, (const uint64_t*)f_stop, ivals,
                     n_ivals, t_max, words, (int)w.max_iv, window, above_periods, start_duration, start_rms_min, below_periods,
                     below_periods ? stop_duration : 0, stop_rms_min);
  hipLaunchKernelGGL(sox_gather_kernel, dim3((t_max + 255) / 256, items), dim3(256), 0, s, x_dev, y_dev, (const int*)lens_dev, (const int*)ivals,
                     (const int*)n_ivals, t_max, (int)w.max_iv, reverse);
  EVMI_LAUNCH_CHECK("sox_silence");
  return EVMI_OK;
}

int evmi_sox_reverse_f32(const float* x_dev, float* y_dev, const int* lens_dev, int items, int t_max, void* stream) {
  if (!x_dev || !y_dev || !lens_dev || x_dev == y_dev || items <= 0 || items > 65535 || t_max <= 0)
    return fail(EVMI_ERR_INVALID_ARG, "sox_reverse: arguments (y must not alias x)");
  hipLaunchKernelGGL(sox_reverse_kernel, dim3((t_max + 255) / 256, items), dim3(256), 0, (hipStream_t)stream, x_dev, y_dev, lens_dev, t_max);
  EVMI_LAUNCH_CHECK("sox_reverse");
  return EVMI_OK;
}

}  // extern "C"
