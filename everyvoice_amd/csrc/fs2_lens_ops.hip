// FastSpeech2 mask_padding: the depthwise convolution and its backward with per-item lengths, channel-major
// x[c][b][t], fp32.  Columns at or beyond lens[b] (int32 on the device, clamped to [0, T] here) are ABSENT: they are read as zero
// whatever they hold (a select, never a multiply: padding may hold NaN) and written as zero.
//   * dwconv_lens_kernel<REV>    forward (REV = false) and input gradient (REV = true: the taps mirrored, no bias, no activation)
//   * dwconv_lens_dw_partial / _final   weight and bias gradient over the valid columns, per-(channel, item) partial sums reduced in
//                                a fixed order (the scheme of fs2_train_ops.hip's kernels, which these stand beside)
// Arithmetic of the forward and of dx: the accumulation order and the activation formulas of dwconv_cbt_kernel (fs2_ops.hip) and
// dwconv_bwd_dx_kernel (fs2_train_ops.hip) -- bias first, taps in ascending j, one fmaf per tap that exists, a tap that does not
// exist leaves the sum untouched -- so with every length equal to T the bits are theirs.
//
// Memory-bound kernels: one WAVE per (c, b) row and 256-column tile, so the row's length, its channel and its k weights are wave-uniform
// (scalar registers, one integer division per wave instead of three per thread); lanes run along t (coalesced 256-byte rows per
// wave instruction); every tap is requested unconditionally from a clamped position and selected afterwards, so the loads of one
// output are in flight together; no LDS, no scratch.
#include <cmath>

#include "common.h"
#include "evmi.h"

namespace evmi {

constexpr int DWL_TILE = 256;  // columns per wave and grid.y step: four outputs per lane
constexpr int DWL_KMAX = 32;   // the backward's tap limit (that of evmi_dwconv1d_bwd_cbt_f32)

__device__ __forceinline__ int clamp_len(int v, int T) { return min(max(v, 0), T); }

// KT: the taps as a compile-time constant (3: variance predictors, 9: the Conformer), 0 = k at run time
template <bool REV, int KT>
__global__ __launch_bounds__(256) void dwconv_lens_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                         const float* __restrict__ bias, const int* __restrict__ lens,
                                                         float* __restrict__ y, long long rows, int B, int T, int k, int pad, int act) {
  const int kk = KT ? KT : k;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + wave;  // = c * B + b, wave-uniform
  if (row >= rows) return;
  const int c = (int)(row / B), b = (int)(row - (long long)c * B);
  const int len = clamp_len(lens[b], T);
  const float* xr = x + row * T;
  float* yr = y + row * T;
  const float* wr = w + (long long)c * kk;
  const float v0 = (!REV && bias) ? bias[c] : 0.f;
  const int t0 = blockIdx.y * DWL_TILE, t1 = min(T, t0 + DWL_TILE);
  if (t0 >= len) {  // the whole tile lies beyond the item: zeros, no load
    for (int t = t0 + lane; t < t1; t += 64) yr[t] = 0.f;
    return;
  }
  for (int t = t0 + lane; t < t1; t += 64) {
    if (t >= len) {  // (only the wave that holds the item's end diverges here)
      yr[t] = 0.f;
      continue;
    }
    float v = v0;
#pragma unroll
    for (int j = 0; j < kk; ++j) {
      const int ti = REV ? t + pad - j : t + j - pad;
      const float xv = xr[min(max(ti, 0), len - 1)];  // len >= 1 here
      v = (ti >= 0 && ti < len) ? fmaf(wr[j], xv, v) : v;
    }
    if (!REV) {
      if (act == 1) v = v / (1.f + expf(-v));
      else if (act == 2) v = fmaxf(v, 0.f);
    }
    yr[t] = v;
  }
}

// part[c][b][j] = sum_{t < len} x[c][b][t + j - pad] * dy[c][b][t] (j < k; x read as zero outside [0, len)), part[c][b][k] = sum_{t < len} dy:
// one workgroup per (c, b) row.  STAGED: the row of x in LDS, zero padded by the kernel's reach and beyond the length; rows longer than
// the LDS take the direct form.  KM: the taps the unrolled loops cover (k <= KM).
template <bool STAGED, int KM>
__global__ __launch_bounds__(256) void dwconv_lens_dw_partial_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                    const int* __restrict__ lens, float* __restrict__ part, int B, int T,
                                                                    int k, int pad) {
  extern __shared__ float xs[];  // STAGED: [T + k - 1], xs[i] = x[i - pad]
  const int b = blockIdx.x, c = blockIdx.y;
  const int len = clamp_len(lens[b], T);
  const float* xr = x + ((long long)c * B + b) * T;
  const float* dr = dy + ((long long)c * B + b) * T;
  float acc[KM];
#pragma unroll
  for (int j = 0; j < KM; ++j) acc[j] = 0.f;
  float sb = 0.f;
  if (STAGED) {
    for (int i = threadIdx.x; i < len + k - 1; i += 256) {  // (t < len reads xs[t .. t + k - 1] only)
      const int ti = i - pad;
      const float v = xr[min(max(ti, 0), T - 1)];  // requested unconditionally, selected afterwards
      xs[i] = (ti >= 0 && ti < len) ? v : 0.f;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < len; t += 256) {
      const float d = dr[t];
      sb += d;
#pragma unroll
      for (int j = 0; j < KM; ++j)
        if (j < k) acc[j] = fmaf(xs[t + j], d, acc[j]);
    }
  } else {
    for (int t = threadIdx.x; t < len; t += 256) {
      const float d = dr[t];
      sb += d;
#pragma unroll
      for (int j = 0; j < KM; ++j) {
        const int ti = t + j - pad;
        if (j < k && ti >= 0 && ti < len) acc[j] = fmaf(xr[ti], d, acc[j]);
      }
    }
  }
  __shared__ double shw[4][DWL_KMAX + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j <= KM; ++j) {
    if (j < k || j == KM) {
      const double v = wave_sum_dpp_f64(j == KM ? (double)sb : (double)acc[j < KM ? j : 0]);
      if (lane == 0) shw[wave][j == KM ? DWL_KMAX : j] = v;
    }
  }
  __syncthreads();
  float* pr = part + ((long long)c * B + b) * (k + 1);
  if (threadIdx.x < k) pr[threadIdx.x] = (float)(shw[0][threadIdx.x] + shw[1][threadIdx.x] + shw[2][threadIdx.x] + shw[3][threadIdx.x]);
  if (threadIdx.x == 0) pr[k] = (float)(shw[0][DWL_KMAX] + shw[1][DWL_KMAX] + shw[2][DWL_KMAX] + shw[3][DWL_KMAX]);
}

// dw[c][j] += sum_b part[c][b][j] ; db[c] += sum_b part[c][b][k]   (fixed order)
__global__ void dwconv_lens_dw_final_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, int C, int B,
                                            int k) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= C * (k + 1)) return;
  const int c = i / (k + 1), j = i - c * (k + 1);
  double acc = 0.0;
  for (int b = 0; b < B; ++b) acc += (double)part[((long long)c * B + b) * (k + 1) + j];
  if (j < k) dw[c * k + j] += (float)acc;
  else if (db) db[c] += (float)acc;
}

template <bool REV>
static void launch_dwconv_lens(const float* x, const float* w, const float* bias, const int* lens, float* y, int C, int B, int T, int k,
                               int pad, int act, hipStream_t s) {
  const long long rows = (long long)C * B;
  const dim3 grid((unsigned)((rows + 3) / 4), (unsigned)((T + DWL_TILE - 1) / DWL_TILE));
  if (k == 3) hipLaunchKernelGGL((dwconv_lens_kernel<REV, 3>), grid, dim3(256), 0, s, x, w, bias, lens, y, rows, B, T, k, pad, act);
  else if (k == 9) hipLaunchKernelGGL((dwconv_lens_kernel<REV, 9>), grid, dim3(256), 0, s, x, w, bias, lens, y, rows, B, T, k, pad, act);
  else hipLaunchKernelGGL((dwconv_lens_kernel<REV, 0>), grid, dim3(256), 0, s, x, w, bias, lens, y, rows, B, T, k, pad, act);
}

}  // namespace evmi

using namespace evmi;

extern "C" {

int evmi_dwconv1d_cbt_lens_f32(const float* x_dev, const float* w_dev, const float* bias_dev, const int* lens_dev, float* y_dev, int C,
                               int B, int T, int k, int pad, int act, void* stream) {
  if (!x_dev || !w_dev || !lens_dev || !y_dev) return fail(EVMI_ERR_INVALID_ARG, "dwconv1d_cbt_lens: null pointer");
  if (C <= 0 || B <= 0 || T <= 0 || k <= 0 || act < 0 || act > 2) return fail(EVMI_ERR_INVALID_ARG, "dwconv1d_cbt_lens: shape");
  if ((T + DWL_TILE - 1) / DWL_TILE > 65535) return fail(EVMI_ERR_UNSUPPORTED, "dwconv1d_cbt_lens: grid limits");
  launch_dwconv_lens<false>(x_dev, w_dev, bias_dev, lens_dev, y_dev, C, B, T, k, pad, act, (hipStream_t)stream);
  EVMI_LAUNCH_CHECK("dwconv1d_cbt_lens");
  return EVMI_OK;
}

int evmi_dwconv1d_bwd_cbt_lens_f32(const float* x, const float* w, const float* dy, const int* lens, float* dx, float* dw, float* db,
                                   float* ws, long long ws_elems, int C, int B, int T, int k, int pad, void* stream) {
  if (!x || !w || !dy || !lens) return fail(EVMI_ERR_INVALID_ARG, "dwconv_bwd_lens: null pointer");
  if (C < 1 || B < 1 || T < 1 || k < 1 || k > DWL_KMAX)
    return fail(EVMI_ERR_INVALID_ARG, "dwconv_bwd_lens: 1 <= k <= 32 and a non-empty input required");
  if ((T + DWL_TILE - 1) / DWL_TILE > 65535 || B > 65535 || C > 65535) return fail(EVMI_ERR_UNSUPPORTED, "dwconv_bwd_lens: grid limits");
  hipStream_t s = (hipStream_t)stream;
  if (dx) {
    launch_dwconv_lens<true>(dy, w, nullptr, lens, dx, C, B, T, k, pad, 0, s);
    EVMI_LAUNCH_CHECK("dwconv_bwd_lens_dx");
  }
  if (dw) {
    if (!ws || ws_elems < evmi_dwconv1d_bwd_cbt_f32_ws_elems(C, B, k))
      return fail(EVMI_ERR_INVALID_ARG, "dwconv_bwd_lens: workspace missing or too small");
    const size_t lds = (size_t)(T + k - 1) * sizeof(float);
#define EVMI_DWL_PARTIAL(KM)                                                                                                             \
  {                                                                                                                                      \
    if (lds <= 40 * 1024)                                                                                                                \
      hipLaunchKernelGGL((dwconv_lens_dw_partial_kernel<true, KM>), dim3(B, C), dim3(256), lds, s, x, dy, lens, ws, B, T, k, pad);      \
    else hipLaunchKernelGGL((dwconv_lens_dw_partial_kernel<false, KM>), dim3(B, C), dim3(256), 0, s, x, dy, lens, ws, B, T, k, pad);    \
  }
    if (k <= 4) EVMI_DWL_PARTIAL(4)
    else if (k <= 12) EVMI_DWL_PARTIAL(12)
    else EVMI_DWL_PARTIAL(DWL_KMAX)
#undef EVMI_DWL_PARTIAL
    EVMI_LAUNCH_CHECK("dwconv_bwd_lens_dw_partial");
    hipLaunchKernelGGL(dwconv_lens_dw_final_kernel, dim3((unsigned)(((long long)C * (k + 1) + 255) / 256)), dim3(256), 0, s, ws, dw, db, C,
                       B, k);
    EVMI_LAUNCH_CHECK("dwconv_bwd_lens_dw_final");
  }
  return EVMI_OK;
}

}  // extern "C"
