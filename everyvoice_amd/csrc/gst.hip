// Global Style Token module of FastSpeech2 (arXiv 1803.09017), fp32, forward and backward:
//   gst_conv_{fwd,dgrad,wgrad}  3 x 3 / stride 2 / padding 1 two-dimensional convolution of the reference encoder on channel-major
//                               tensors x[c][b][h][w] (h = frames, w = mel bins), weights [c_out][c_in][3][3] as torch stores them.
//                               Output o reads inputs 2 o - 1 .. 2 o + 1: the low-side padding is always read, the high-side one only
//                               for an odd input length.  Direct kernels: every thread owns one position and a tile of channels, the
//                               weights are workgroup-uniform (scalar loads).
//   gst_gru_{fwd,bwd}           the recurrence of a single-layer GRU in ONE launch for all steps: a workgroup per item, a thread per
//                               gate row, its row (backward: its column piece) of W_hh in registers for all steps, h in LDS.
//   gst_conv_fwd_rows, gst_gru_{fwd,bwd}_steps  the same with per-item lengths read from device memory: rows / steps beyond an
//                               item's length are absent (never read), what is written there is zero.
//   gst_attention_{fwd,bwd}     one query per item against the style tokens' keys / values, `heads` heads.
// Every sum is taken in a fixed order (no float atomics): the training step is bit-reproducible run to run.
#include "common.h"

namespace evmi {
namespace {

constexpr int kConvThreads = 256;
constexpr int kFwdCoTile = 16;   // output channels per thread (forward)
constexpr int kDgradCiTile = 8;  // input channels per thread (input gradient)
constexpr int kWgCo = 4, kWgCi = 4;  // the weight gradient's channel tile: 4 x 4 x 9 accumulators per thread
constexpr int kWgMaxSplit = 64;

__host__ __device__ inline int conv_out(int n) { return (n - 1) / 2 + 1; }

// ---- forward ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kConvThreads) void gst_conv_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                    const float* __restrict__ bias, float* __restrict__ y, int Cin,
                                                                    int Cout, int B, int H, int W, int OH, int OW, int act) {
  const long long n = (long long)blockIdx.x * kConvThreads + threadIdx.x;
  const long long total = (long long)B * OH * OW;
  if (n >= total) return;
  const int co0 = blockIdx.y * kFwdCoTile;
  const int ow = (int)(n % OW), oh = (int)((n / OW) % OH), b = (int)(n / ((long long)OW * OH));
  int off[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
      ok[kh * 3 + kw] = ih >= 0 && ih < H && iw >= 0 && iw < W;
      off[kh * 3 + kw] = ok[kh * 3 + kw] ? ih * W + iw : 0;
    }
  float acc[kFwdCoTile];
#pragma unroll
  for (int j = 0; j < kFwdCoTile; ++j) acc[j] = (bias && co0 + j < Cout) ? bias[co0 + j] : 0.f;
  const long long plane = (long long)H * W;
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xp = x + ((long long)ci * B + b) * plane;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = ok[t] ? xp[off[t]] : 0.f;
#pragma unroll
    for (int j = 0; j < kFwdCoTile; ++j) {
      if (co0 + j >= Cout) break;
      const float* wp = w + ((long long)(co0 + j) * Cin + ci) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[j] = fmaf(v[t], wp[t], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kFwdCoTile; ++j) {
    if (co0 + j >= Cout) break;
    float r = acc[j];
    if (act == 3) r = fmaxf(r, 0.f);
    y[((long long)(co0 + j) * B + b) * OH * OW + (long long)oh * OW + ow] = r;
  }
}

// ---- forward with per-item row counts: rows at or beyond rows_in[b] are absent (never read), output rows beyond conv_out(rows_in[b])
// are written as zero.  The per-output sum (input channels outer, nine taps inner) is gst_conv_fwd_kernel's: with rows_in[b] == H for
// every item the two are bit-equal.  A thread of an invalid output row stores its zeros and leaves before the channel loop.
__global__ __launch_bounds__(kConvThreads) void gst_conv_fwd_rows_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                                         const float* __restrict__ bias, float* __restrict__ y,
                                                                         const int* __restrict__ rows_in, int Cin, int Cout, int B, int H,
                                                                         int W, int OH, int OW, int act) {
  const long long n = (long long)blockIdx.x * kConvThreads + threadIdx.x;
  const long long total = (long long)B * OH * OW;
  if (n >= total) return;
  const int co0 = blockIdx.y * kFwdCoTile;
  const int ow = (int)(n % OW), oh = (int)((n / OW) % OH), b = (int)(n / ((long long)OW * OH));
  const int rows = min(max(rows_in[b], 0), H);
  if (rows < 1 || oh >= conv_out(rows)) {
#pragma unroll
    for (int j = 0; j < kFwdCoTile; ++j) {
      if (co0 + j >= Cout) break;
      y[((long long)(co0 + j) * B + b) * OH * OW + (long long)oh * OW + ow] = 0.f;
    }
    return;
  }
  int off[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
      ok[kh * 3 + kw] = ih >= 0 && ih < rows && iw >= 0 && iw < W;
      off[kh * 3 + kw] = ok[kh * 3 + kw] ? ih * W + iw : 0;
    }
  float acc[kFwdCoTile];
#pragma unroll
  for (int j = 0; j < kFwdCoTile; ++j) acc[j] = (bias && co0 + j < Cout) ? bias[co0 + j] : 0.f;
  const long long plane = (long long)H * W;
  for (int ci = 0; ci < Cin; ++ci) {
    const float* xp = x + ((long long)ci * B + b) * plane;
    float v[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) v[t] = ok[t] ? xp[off[t]] : 0.f;
#pragma unroll
    for (int j = 0; j < kFwdCoTile; ++j) {
      if (co0 + j >= Cout) break;
      const float* wp = w + ((long long)(co0 + j) * Cin + ci) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[j] = fmaf(v[t], wp[t], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kFwdCoTile; ++j) {
    if (co0 + j >= Cout) break;
    float r = acc[j];
    if (act == 3) r = fmaxf(r, 0.f);
    y[((long long)(co0 + j) * B + b) * OH * OW + (long long)oh * OW + ow] = r;
  }
}

// ---- input gradient: dx[ci][b][ih][iw] = sum over co and the taps with 2 o - 1 + k = i of w[co][ci][kh][kw] dy[co][b][oh][ow] ------
__global__ __launch_bounds__(kConvThreads) void gst_conv_dgrad_kernel(const float* __restrict__ dy, const float* __restrict__ w,
                                                                      float* __restrict__ dx, int Cin, int Cout, int B, int H, int W,
                                                                      int OH, int OW) {
  const long long n = (long long)blockIdx.x * kConvThreads + threadIdx.x;
  const long long total = (long long)B * H * W;
  if (n >= total) return;
  const int ci0 = blockIdx.y * kDgradCiTile;
  const int iw = (int)(n % W), ih = (int)((n / W) % H), b = (int)(n / ((long long)W * H));
  int off[9];
  bool ok[9];
#pragma unroll
  for (int kh = 0; kh < 3; ++kh)
#pragma unroll
    for (int kw = 0; kw < 3; ++kw) {
      const int h2 = ih + 1 - kh, w2 = iw + 1 - kw;  // = 2 oh, 2 ow
      const bool v = h2 >= 0 && w2 >= 0 && !(h2 & 1) && !(w2 & 1) && (h2 >> 1) < OH && (w2 >> 1) < OW;
      ok[kh * 3 + kw] = v;
      off[kh * 3 + kw] = v ? (h2 >> 1) * OW + (w2 >> 1) : 0;
    }
  float acc[kDgradCiTile];
#pragma unroll
  for (int j = 0; j < kDgradCiTile; ++j) acc[j] = 0.f;
  const long long oplane = (long long)OH * OW;
  for (int co = 0; co < Cout; ++co) {
    const float* gp = dy + ((long long)co * B + b) * oplane;
    float g[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) g[t] = ok[t] ? gp[off[t]] : 0.f;
#pragma unroll
    for (int j = 0; j < kDgradCiTile; ++j) {
      if (ci0 + j >= Cin) break;
      const float* wp = w + ((long long)co * Cin + ci0 + j) * 9;
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[j] = fmaf(g[t], wp[t], acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < kDgradCiTile; ++j) {
    if (ci0 + j >= Cin) break;
    dx[((long long)(ci0 + j) * B + b) * H * W + (long long)ih * W + iw] = acc[j];
  }
}

// ---- weight and bias gradient: partials over `split` slices of the B * OH * OW positions, then a fixed-order sum --------------------
inline int wgrad_split(long long positions) {
  const long long s = positions / 2048;
  return (int)(s < 1 ? 1 : (s > kWgMaxSplit ? kWgMaxSplit : s));
}

__global__ __launch_bounds__(kConvThreads) void gst_conv_wgrad_kernel(const float* __restrict__ x, const float* __restrict__ dy,
                                                                      float* __restrict__ part, int Cin, int Cout, int B, int H, int W,
                                                                      int OH, int OW, int split) {
  __shared__ float sh[kConvThreads / 64][kWgCo * kWgCi * 9 + kWgCo];
  const int ci_tiles = (Cin + kWgCi - 1) / kWgCi;
  const int co0 = (blockIdx.x / ci_tiles) * kWgCo, ci0 = (blockIdx.x % ci_tiles) * kWgCi;
  const int s = blockIdx.y;
  const long long total = (long long)B * OH * OW;
  const long long per = (total + split - 1) / split;
  const long long lo = (long long)s * per, hi = lo + per < total ? lo + per : total;
  const long long plane = (long long)H * W, oplane = (long long)OH * OW;
  float acc[kWgCo][kWgCi][9];
  float accb[kWgCo];
#pragma unroll
  for (int a = 0; a < kWgCo; ++a) {
    accb[a] = 0.f;
#pragma unroll
    for (int c = 0; c < kWgCi; ++c)
#pragma unroll
      for (int t = 0; t < 9; ++t) acc[a][c][t] = 0.f;
  }
  for (long long n = lo + threadIdx.x; n < hi; n += kConvThreads) {
    const int ow = (int)(n % OW), oh = (int)((n / OW) % OH), b = (int)(n / oplane);
    float g[kWgCo];
#pragma unroll
    for (int a = 0; a < kWgCo; ++a) {
      g[a] = co0 + a < Cout ? dy[((long long)(co0 + a) * B + b) * oplane + (long long)oh * OW + ow] : 0.f;
      accb[a] += g[a];
    }
#pragma unroll
    for (int c = 0; c < kWgCi; ++c) {
      if (ci0 + c >= Cin) break;
      const float* xp = x + ((long long)(ci0 + c) * B + b) * plane;
#pragma unroll
      for (int kh = 0; kh < 3; ++kh)
#pragma unroll
        for (int kw = 0; kw < 3; ++kw) {
          const int ih = 2 * oh - 1 + kh, iw = 2 * ow - 1 + kw;
          const float v = (ih >= 0 && ih < H && iw >= 0 && iw < W) ? xp[ih * W + iw] : 0.f;
#pragma unroll
          for (int a = 0; a < kWgCo; ++a) acc[a][c][kh * 3 + kw] = fmaf(g[a], v, acc[a][c][kh * 3 + kw]);
        }
    }
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int a = 0; a < kWgCo; ++a) {
#pragma unroll
    for (int c = 0; c < kWgCi; ++c)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const float r = wave_sum_dpp(acc[a][c][t]);
        if (lane == 0) sh[wave][(a * kWgCi + c) * 9 + t] = r;
      }
    const float rb = wave_sum_dpp(accb[a]);
    if (lane == 0) sh[wave][kWgCo * kWgCi * 9 + a] = rb;
  }
  __syncthreads();
  const int i = threadIdx.x;
  if (i >= kWgCo * kWgCi * 9 + kWgCo) return;
  float r = sh[0][i];
#pragma unroll
  for (int q = 1; q < kConvThreads / 64; ++q) r += sh[q][i];  // (wave order: fixed)
  const long long n_w = (long long)Cout * Cin * 9;
  float* ps = part + (long long)s * (n_w + Cout);
  if (i < kWgCo * kWgCi * 9) {
    const int a = i / (kWgCi * 9), c = (i / 9) % kWgCi, t = i % 9;
    if (co0 + a < Cout && ci0 + c < Cin) ps[((long long)(co0 + a) * Cin + ci0 + c) * 9 + t] = r;
  } else {
    const int a = i - kWgCo * kWgCi * 9;
    if (ci0 == 0 && co0 + a < Cout) ps[n_w + co0 + a] = r;
  }
}

__global__ void gst_conv_wgrad_reduce_kernel(const float* __restrict__ part, float* __restrict__ dw, float* __restrict__ db, long long n_w,
                                             int Cout, int split, int accumulate) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_w + Cout) return;
  float* dst = i < n_w ? dw + i : (db ? db + (i - n_w) : nullptr);
  if (!dst) return;
  *dst = ordered_sum_strided(part + i, n_w + Cout, split, accumulate ? *dst : 0.f);
}

// ---- GRU recurrence ---------------------------------------------------------------------------------------------------------------
// gi [3H][B][T]: x W_ih^T + b_ih of every step (gate order r, z, n).  Saved for the backward: rzn [3H][B][T] (the gates behind their
// activations), hn [H][B][T] (W_hn h + b_hn), hprev [H][B][T] (the state each step started from; zero at t = 0).
__device__ __forceinline__ float sigmoid_(float v) { return 1.f / (1.f + expf(-v)); }

template <int H>
__global__ __launch_bounds__(3 * H) void gst_gru_fwd_kernel(const float* __restrict__ gi, const float* __restrict__ whh,
                                                            const float* __restrict__ bhh, float* __restrict__ rzn, float* __restrict__ hn,
                                                            float* __restrict__ hprev, float* __restrict__ hlast, int B, int T) {
  __shared__ __attribute__((aligned(16))) float h[H];
  __shared__ float gate[2 * H];
  const int b = blockIdx.x, j = threadIdx.x;
  float w[H];
#pragma unroll
  for (int k = 0; k < H; ++k) w[k] = whh[(long long)j * H + k];  // (a parameter inside a flat buffer: no 16-byte alignment to rely on)
  const float bj = bhh[j];
  if (j < H) h[j] = 0.f;
  __syncthreads();
  const long long row = ((long long)j * B + b) * T;
  for (int t = 0; t < T; ++t) {
    const float x = gi[row + t];
    float acc = bj;
#pragma unroll
    for (int k = 0; k < H; k += 4) {
      const f32x4 hv = *reinterpret_cast<const f32x4*>(h + k);
      acc = fmaf(w[k], hv[0], acc);
      acc = fmaf(w[k + 1], hv[1], acc);
      acc = fmaf(w[k + 2], hv[2], acc);
      acc = fmaf(w[k + 3], hv[3], acc);
    }
    if (j < 2 * H) {
      const float v = sigmoid_(x + acc);
      gate[j] = v;
      if (rzn) rzn[row + t] = v;
    }
    __syncthreads();  // every product has read h; r and z are in LDS
    if (j >= 2 * H) {
      const int k = j - 2 * H;
      const float r = gate[k], z = gate[H + k], hp = h[k];
      const float n = tanhf(x + r * acc);
      if (rzn) {
        rzn[row + t] = n;
        hn[((long long)k * B + b) * T + t] = acc;
        hprev[((long long)k * B + b) * T + t] = hp;
      }
      h[k] = (1.f - z) * n + z * hp;
    }
    __syncthreads();
  }
  if (j < H) hlast[(long long)j * B + b] = h[j];
}

// dgi [3H][B][T]: gradient of the projected inputs; dgh [3H][B][T]: gradient of W_hh h + b_hh (dW_hh = dgh hprev^T and db_hh = its
// row sums are a dense layer's weight gradient).  Thread (g, k) keeps W_hh[g H .. g H + H - 1][k] for dh_prev = W_hh^T dgh.
template <int H>
__global__ __launch_bounds__(3 * H) void gst_gru_bwd_kernel(const float* __restrict__ rzn, const float* __restrict__ hn,
                                                            const float* __restrict__ hprev, const float* __restrict__ whh,
                                                            const float* __restrict__ dhlast, float* __restrict__ dgi,
                                                            float* __restrict__ dgh, int B, int T) {
  __shared__ __attribute__((aligned(16))) float dg[3 * H];
  __shared__ float part[3 * H];
  __shared__ float dh[H];
  const int b = blockIdx.x, j = threadIdx.x, g = j / H, k = j % H;
  float wt[H];
#pragma unroll
  for (int i = 0; i < H; ++i) wt[i] = whh[((long long)g * H + i) * H + k];
  if (g == 0) dh[k] = dhlast[(long long)k * B + b];
  __syncthreads();
  const long long BT = (long long)B * T;
  const long long col = ((long long)k * B + b) * T;
  for (int t = T - 1; t >= 0; --t) {
    float carry = 0.f;
    if (g == 0) {
      const float r = rzn[col + t], z = rzn[(long long)H * BT + col + t], n = rzn[2ll * H * BT + col + t];
      const float a = hn[col + t], hp = hprev[col + t], d = dh[k];
      const float dn = d * (1.f - z) * (1.f - n * n);
      const float dz = d * (hp - n) * z * (1.f - z);
      const float dr = dn * a * r * (1.f - r);
      dgi[col + t] = dr;
      dgi[(long long)H * BT + col + t] = dz;
      dgi[2ll * H * BT + col + t] = dn;
      dgh[col + t] = dr;
      dgh[(long long)H * BT + col + t] = dz;
      dgh[2ll * H * BT + col + t] = dn * r;
      dg[k] = dr;
      dg[H + k] = dz;
      dg[2 * H + k] = dn * r;
      carry = d * z;
    }
    __syncthreads();
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < H; i += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(dg + g * H + i);
      p = fmaf(wt[i], v[0], p);
      p = fmaf(wt[i + 1], v[1], p);
      p = fmaf(wt[i + 2], v[2], p);
      p = fmaf(wt[i + 3], v[3], p);
    }
    part[j] = p;
    __syncthreads();
    if (g == 0) dh[k] = carry + ((part[k] + part[H + k]) + part[2 * H + k]);
    __syncthreads();
  }
}

// ---- GRU recurrence with per-item step counts --------------------------------------------------------------------------------------
// Item b runs n = clamp(steps[b], 1, T) steps: hlast is the state after step n - 1, the saved tensors and dgi / dgh are zero at later
// steps (so the dense weight gradients over all B * T columns pick up nothing from them) and gi there is never read.  n is read once
// into a workgroup-uniform value: every __syncthreads() is reached by all threads.  With steps[b] == T the loops are those above.
template <int H>
__global__ __launch_bounds__(3 * H) void gst_gru_fwd_steps_kernel(const float* __restrict__ gi, const float* __restrict__ whh,
                                                                  const float* __restrict__ bhh, float* __restrict__ rzn,
                                                                  float* __restrict__ hn, float* __restrict__ hprev,
                                                                  float* __restrict__ hlast, const int* __restrict__ steps, int B, int T) {
  __shared__ __attribute__((aligned(16))) float h[H];
  __shared__ float gate[2 * H];
  const int b = blockIdx.x, j = threadIdx.x;
  const int n_steps = __builtin_amdgcn_readfirstlane(min(max(steps[b], 1), T));
  float w[H];
#pragma unroll
  for (int k = 0; k < H; ++k) w[k] = whh[(long long)j * H + k];
  const float bj = bhh[j];
  if (j < H) h[j] = 0.f;
  __syncthreads();
  const long long row = ((long long)j * B + b) * T;
  for (int t = 0; t < n_steps; ++t) {
    const float x = gi[row + t];
    float acc = bj;
#pragma unroll
    for (int k = 0; k < H; k += 4) {
      const f32x4 hv = *reinterpret_cast<const f32x4*>(h + k);
      acc = fmaf(w[k], hv[0], acc);
      acc = fmaf(w[k + 1], hv[1], acc);
      acc = fmaf(w[k + 2], hv[2], acc);
      acc = fmaf(w[k + 3], hv[3], acc);
    }
    if (j < 2 * H) {
      const float v = sigmoid_(x + acc);
      gate[j] = v;
      if (rzn) rzn[row + t] = v;
    }
    __syncthreads();  // every product has read h; r and z are in LDS
    if (j >= 2 * H) {
      const int k = j - 2 * H;
      const float r = gate[k], z = gate[H + k], hp = h[k];
      const float n = tanhf(x + r * acc);
      if (rzn) {
        rzn[row + t] = n;
        hn[((long long)k * B + b) * T + t] = acc;
        hprev[((long long)k * B + b) * T + t] = hp;
      }
      h[k] = (1.f - z) * n + z * hp;
    }
    __syncthreads();
  }
  if (j < H) hlast[(long long)j * B + b] = h[j];
  if (rzn)
    for (int t = n_steps; t < T; ++t) {
      rzn[row + t] = 0.f;
      if (j < H) {
        hn[row + t] = 0.f;  // (j < H: row is also the [H][B][T] offset of hidden unit j)
        hprev[row + t] = 0.f;
      }
    }
}

template <int H>
__global__ __launch_bounds__(3 * H) void gst_gru_bwd_steps_kernel(const float* __restrict__ rzn, const float* __restrict__ hn,
                                                                  const float* __restrict__ hprev, const float* __restrict__ whh,
                                                                  const float* __restrict__ dhlast, float* __restrict__ dgi,
                                                                  float* __restrict__ dgh, const int* __restrict__ steps, int B, int T) {
  __shared__ __attribute__((aligned(16))) float dg[3 * H];
  __shared__ float part[3 * H];
  __shared__ float dh[H];
  const int b = blockIdx.x, j = threadIdx.x, g = j / H, k = j % H;
  const int n_steps = __builtin_amdgcn_readfirstlane(min(max(steps[b], 1), T));
  float wt[H];
#pragma unroll
  for (int i = 0; i < H; ++i) wt[i] = whh[((long long)g * H + i) * H + k];
  if (g == 0) dh[k] = dhlast[(long long)k * B + b];
  __syncthreads();
  const long long BT = (long long)B * T;
  const long long col = ((long long)k * B + b) * T;
  for (int t = n_steps; t < T; ++t) {  // the absent steps: thread (g, k) zeroes gate row g H + k of both outputs
    dgi[(long long)g * H * BT + col + t] = 0.f;
    dgh[(long long)g * H * BT + col + t] = 0.f;
  }
  for (int t = n_steps - 1; t >= 0; --t) {
    float carry = 0.f;
    if (g == 0) {
      const float r = rzn[col + t], z = rzn[(long long)H * BT + col + t], n = rzn[2ll * H * BT + col + t];
      const float a = hn[col + t], hp = hprev[col + t], d = dh[k];
      const float dn = d * (1.f - z) * (1.f - n * n);
      const float dz = d * (hp - n) * z * (1.f - z);
      const float dr = dn * a * r * (1.f - r);
      dgi[col + t] = dr;
      dgi[(long long)H * BT + col + t] = dz;
      dgi[2ll * H * BT + col + t] = dn;
      dgh[col + t] = dr;
      dgh[(long long)H * BT + col + t] = dz;
      dgh[2ll * H * BT + col + t] = dn * r;
      dg[k] = dr;
      dg[H + k] = dz;
      dg[2 * H + k] = dn * r;
      carry = d * z;
    }
    __syncthreads();
    float p = 0.f;
#pragma unroll
    for (int i = 0; i < H; i += 4) {
      const f32x4 v = *reinterpret_cast<const f32x4*>(dg + g * H + i);
      p = fmaf(wt[i], v[0], p);
      p = fmaf(wt[i + 1], v[1], p);
      p = fmaf(wt[i + 2], v[2], p);
      p = fmaf(wt[i + 3], v[3], p);
    }
    part[j] = p;
    __syncthreads();
    if (g == 0) dh[k] = carry + ((part[k] + part[H + k]) + part[2 * H + k]);
    __syncthreads();
  }
}

// ---- style-token attention ---------------------------------------------------------------------------------------------------------
// q [E][B], keys / values [E][N] (channel-major, as the dense layers write them); style [B][E]; probs [B][heads][N]
constexpr int kMaxTokens = 16;

__global__ void gst_attention_fwd_kernel(const float* __restrict__ q, const float* __restrict__ keys, const float* __restrict__ values,
                                         float* __restrict__ style, float* __restrict__ probs, int B, int N, int E, int heads) {
  extern __shared__ float lds[];
  float* prod = lds;                   // [N][E]
  float* sc = lds + (long long)N * E;  // [heads][N]
  const int b = blockIdx.x, e = threadIdx.x, dh = E / heads, hd = e / dh;
  const float qe = q[(long long)e * B + b];
  for (int n = 0; n < N; ++n) prod[n * E + e] = qe * keys[(long long)e * N + n];
  __syncthreads();
  for (int i = e; i < heads * N; i += E) {
    const int h2 = i / N, n = i % N;
    float s = 0.f;
    for (int d = 0; d < dh; ++d) s += prod[n * E + h2 * dh + d];
    sc[h2 * N + n] = s / sqrtf((float)dh);
  }
  __syncthreads();
  if (e < heads) {
    float m = sc[e * N];
    for (int n = 1; n < N; ++n) m = fmaxf(m, sc[e * N + n]);
    float sum = 0.f;
    for (int n = 0; n < N; ++n) sum += expf(sc[e * N + n] - m);
    for (int n = 0; n < N; ++n) {
      const float p = expf(sc[e * N + n] - m) / sum;
      sc[e * N + n] = p;
      if (probs) probs[((long long)b * heads + e) * N + n] = p;
    }
  }
  __syncthreads();
  float o = 0.f;
  for (int n = 0; n < N; ++n) o = fmaf(sc[hd * N + n], values[(long long)e * N + n], o);
  style[(long long)b * E + e] = o;
}

// One workgroup walks the items in order: dK and dV are sums over the items, kept in registers (dq [E][B], dkeys / dvalues [E][N]).
__global__ void gst_attention_bwd_kernel(const float* __restrict__ dstyle, const float* __restrict__ q, const float* __restrict__ keys,
                                         const float* __restrict__ values, const float* __restrict__ probs, float* __restrict__ dq,
                                         float* __restrict__ dkeys, float* __restrict__ dvalues, int B, int N, int E, int heads) {
  extern __shared__ float lds[];
  float* prod = lds;                   // [N][E]
  float* dsc = lds + (long long)N * E;  // [heads][N]: gradient of the scaled scores
  float* pr = dsc + heads * N;          // [heads][N]: the probabilities
  const int e = threadIdx.x, dh = E / heads, hd = e / dh;
  const float scale = 1.f / sqrtf((float)dh);
  float kr[kMaxTokens], vr[kMaxTokens], dk[kMaxTokens], dv[kMaxTokens];
#pragma unroll
  for (int n = 0; n < kMaxTokens; ++n) {
    kr[n] = n < N ? keys[(long long)e * N + n] : 0.f;
    vr[n] = n < N ? values[(long long)e * N + n] : 0.f;
    dk[n] = 0.f;
    dv[n] = 0.f;
  }
  for (int b = 0; b < B; ++b) {
    const float ds = dstyle[(long long)b * E + e], qe = q[(long long)e * B + b];
#pragma unroll
    for (int n = 0; n < kMaxTokens; ++n)
      if (n < N) prod[n * E + e] = ds * vr[n];
    __syncthreads();
    for (int i = e; i < heads * N; i += E) {
      const int h2 = i / N, n = i % N;
      float s = 0.f;
      for (int d = 0; d < dh; ++d) s += prod[n * E + h2 * dh + d];
      dsc[h2 * N + n] = s;  // dP for now
      pr[h2 * N + n] = probs[((long long)b * heads + h2) * N + n];
    }
    __syncthreads();
    if (e < heads) {
      float dot = 0.f;
      for (int n = 0; n < N; ++n) dot = fmaf(pr[e * N + n], dsc[e * N + n], dot);
      for (int n = 0; n < N; ++n) dsc[e * N + n] = pr[e * N + n] * (dsc[e * N + n] - dot) * scale;
    }
    __syncthreads();
    float a = 0.f;
#pragma unroll
    for (int n = 0; n < kMaxTokens; ++n)
      if (n < N) {
        const float g = dsc[hd * N + n];
        a = fmaf(g, kr[n], a);
        dk[n] = fmaf(g, qe, dk[n]);
        dv[n] = fmaf(pr[hd * N + n], ds, dv[n]);
      }
    dq[(long long)e * B + b] = a;
    __syncthreads();
  }
#pragma unroll
  for (int n = 0; n < kMaxTokens; ++n)
    if (n < N) {
      dkeys[(long long)e * N + n] = dk[n];
      dvalues[(long long)e * N + n] = dv[n];
    }
}

bool conv_shape_ok(int Cin, int Cout, int B, int H, int W) {
  return Cin >= 1 && Cout >= 1 && B >= 1 && H >= 1 && W >= 1 && (long long)(Cin > Cout ? Cin : Cout) * B * H * W < (1ll << 31);
}

bool attention_shape_ok(int B, int N, int E, int heads) {
  return B >= 1 && N >= 1 && N <= kMaxTokens && heads >= 1 && E >= heads && E % heads == 0 && E % 64 == 0 && E <= 1024;
}

}  // namespace
}  // namespace evmi

using namespace evmi;

extern "C" {

int evmi_gst_conv2d_fwd_f32(const float* x, const float* w, const float* bias, float* y, int Cin, int Cout, int B, int H, int W, int act,
                            void* stream) {
  if (!x || !w || !y || !conv_shape_ok(Cin, Cout, B, H, W)) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_fwd: bad arguments");
  if (act != 0 && act != 3) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_fwd: act must be 0 (none) or 3 (ReLU)");
  const int OH = conv_out(H), OW = conv_out(W);
  const long long total = (long long)B * OH * OW;
  const dim3 grid((unsigned)((total + kConvThreads - 1) / kConvThreads), (unsigned)((Cout + kFwdCoTile - 1) / kFwdCoTile));
  hipLaunchKernelGGL(gst_conv_fwd_kernel, grid, dim3(kConvThreads), 0, (hipStream_t)stream, x, w, bias, y, Cin, Cout, B, H, W, OH, OW, act);
  EVMI_LAUNCH_CHECK("gst_conv2d_fwd");
  return EVMI_OK;
}

int evmi_gst_conv2d_fwd_rows_f32(const float* x, const float* w, const float* bias, float* y, const int* rows_in_dev, int Cin, int Cout, int B,
                                 int H, int W, int act, void* stream) {
  if (!x || !w || !y || !rows_in_dev || !conv_shape_ok(Cin, Cout, B, H, W)) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_fwd_rows: bad arguments");
  if (act != 0 && act != 3) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_fwd_rows: act must be 0 (none) or 3 (ReLU)");
  const int OH = conv_out(H), OW = conv_out(W);
  const long long total = (long long)B * OH * OW;
  const dim3 grid((unsigned)((total + kConvThreads - 1) / kConvThreads), (unsigned)((Cout + kFwdCoTile - 1) / kFwdCoTile));
  hipLaunchKernelGGL(gst_conv_fwd_rows_kernel, grid, dim3(kConvThreads), 0, (hipStream_t)stream, x, w, bias, y, rows_in_dev, Cin, Cout, B, H, W,
                     OH, OW, act);
  EVMI_LAUNCH_CHECK("gst_conv2d_fwd_rows");
  return EVMI_OK;
}

int evmi_gst_conv2d_dgrad_f32(const float* dy, const float* w, float* dx, int Cin, int Cout, int B, int H, int W, void* stream) {
  if (!dy || !w || !dx || !conv_shape_ok(Cin, Cout, B, H, W)) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_dgrad: bad arguments");
  const int OH = conv_out(H), OW = conv_out(W);
  const long long total = (long long)B * H * W;
  const dim3 grid((unsigned)((total + kConvThreads - 1) / kConvThreads), (unsigned)((Cin + kDgradCiTile - 1) / kDgradCiTile));
  hipLaunchKernelGGL(gst_conv_dgrad_kernel, grid, dim3(kConvThreads), 0, (hipStream_t)stream, dy, w, dx, Cin, Cout, B, H, W, OH, OW);
  EVMI_LAUNCH_CHECK("gst_conv2d_dgrad");
  return EVMI_OK;
}

long long evmi_gst_conv2d_wgrad_ws_elems(int Cin, int Cout, int B, int H, int W) {
  if (!conv_shape_ok(Cin, Cout, B, H, W)) return 0;
  const long long positions = (long long)B * conv_out(H) * conv_out(W);
  return (long long)wgrad_split(positions) * ((long long)Cout * Cin * 9 + Cout);
}

int evmi_gst_conv2d_wgrad_f32(const float* x, const float* dy, float* dw, float* db, float* ws, long long ws_elems, int Cin, int Cout,
                              int B, int H, int W, int accumulate, void* stream) {
  if (!x || !dy || !dw || !ws || !conv_shape_ok(Cin, Cout, B, H, W)) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_wgrad: bad arguments");
  if (ws_elems < evmi_gst_conv2d_wgrad_ws_elems(Cin, Cout, B, H, W)) return fail(EVMI_ERR_INVALID_ARG, "gst_conv2d_wgrad: workspace too small");
  const int OH = conv_out(H), OW = conv_out(W);
  const int split = wgrad_split((long long)B * OH * OW);
  const int tiles = ((Cout + kWgCo - 1) / kWgCo) * ((Cin + kWgCi - 1) / kWgCi);
  hipLaunchKernelGGL(gst_conv_wgrad_kernel, dim3((unsigned)tiles, (unsigned)split), dim3(kConvThreads), 0, (hipStream_t)stream, x, dy, ws,
                     Cin, Cout, B, H, W, OH, OW, split);
  EVMI_LAUNCH_CHECK("gst_conv2d_wgrad");
  const long long n_w = (long long)Cout * Cin * 9;
  hipLaunchKernelGGL(gst_conv_wgrad_reduce_kernel, dim3((unsigned)((n_w + Cout + 255) / 256)), dim3(256), 0, (hipStream_t)stream, ws, dw, db,
                     n_w, Cout, split, accumulate);
  EVMI_LAUNCH_CHECK("gst_conv2d_wgrad_reduce");
  return EVMI_OK;
}

int evmi_gst_gru_fwd_f32(const float* gi, const float* whh, const float* bhh, float* rzn, float* hn, float* hprev, float* hlast, int B, int T,
                         int H, void* stream) {
  if (!gi || !whh || !bhh || !hlast || B < 1 || T < 1) return fail(EVMI_ERR_INVALID_ARG, "gst_gru_fwd: bad arguments");
  if ((rzn != nullptr) != (hn != nullptr) || (rzn != nullptr) != (hprev != nullptr))
    return fail(EVMI_ERR_INVALID_ARG, "gst_gru_fwd: the saved tensors (gates, hn, hprev) go together");
  if (H == 128)
    hipLaunchKernelGGL(gst_gru_fwd_kernel<128>, dim3(B), dim3(384), 0, (hipStream_t)stream, gi, whh, bhh, rzn, hn, hprev, hlast, B, T);
  else if (H == 64)
    hipLaunchKernelGGL(gst_gru_fwd_kernel<64>, dim3(B), dim3(192), 0, (hipStream_t)stream, gi, whh, bhh, rzn, hn, hprev, hlast, B, T);
  else if (H == 32)
    hipLaunchKernelGGL(gst_gru_fwd_kernel<32>, dim3(B), dim3(96), 0, (hipStream_t)stream, gi, whh, bhh, rzn, hn, hprev, hlast, B, T);
  else
    return fail(EVMI_ERR_UNSUPPORTED, "gst_gru_fwd: hidden size 32, 64 or 128 (encoder.input_dim 64, 128 or 256)");
  EVMI_LAUNCH_CHECK("gst_gru_fwd");
  return EVMI_OK;
}

int evmi_gst_gru_bwd_f32(const float* rzn, const float* hn, const float* hprev, const float* whh, const float* dhlast, float* dgi, float* dgh,
                         int B, int T, int H, void* stream) {
  if (!rzn || !hn || !hprev || !whh || !dhlast || !dgi || !dgh || B < 1 || T < 1) return fail(EVMI_ERR_INVALID_ARG, "gst_gru_bwd: bad arguments");
  if (H == 128)
    hipLaunchKernelGGL(gst_gru_bwd_kernel<128>, dim3(B), dim3(384), 0, (hipStream_t)stream, rzn, hn, hprev, whh, dhlast, dgi, dgh, B, T);
  else if (H == 64)
    hipLaunchKernelGGL(gst_gru_bwd_kernel<64>, dim3(B), dim3(192), 0, (hipStream_t)stream, rzn, hn, hprev, whh, dhlast, dgi, dgh, B, T);
  else if (H == 32)
    hipLaunchKernelGGL(gst_gru_bwd_kernel<32>, dim3(B), dim3(96), 0, (hipStream_t)stream, rzn, hn, hprev, whh, dhlast, dgi, dgh, B, T);
  else
    return fail(EVMI_ERR_UNSUPPORTED, "gst_gru_bwd: hidden size 32, 64 or 128 (encoder.input_dim 64, 128 or 256)");
  EVMI_LAUNCH_CHECK("gst_gru_bwd");
  return EVMI_OK;
}

int evmi_gst_gru_fwd_steps_f32(const float* gi, const float* whh, const float* bhh, float* rzn, float* hn, float* hprev, float* hlast,
                               const int* steps_dev, int B, int T, int H, void* stream) {
  if (!gi || !whh || !bhh || !hlast || !steps_dev || B < 1 || T < 1) return fail(EVMI_ERR_INVALID_ARG, "gst_gru_fwd_steps: bad arguments");
  if ((rzn != nullptr) != (hn != nullptr) || (rzn != nullptr) != (hprev != nullptr))
    return fail(EVMI_ERR_INVALID_ARG, "gst_gru_fwd_steps: the saved tensors (gates, hn, hprev) go together");
  if (H == 128)
    hipLaunchKernelGGL(gst_gru_fwd_steps_kernel<128>, dim3(B), dim3(384), 0, (hipStream_t)stream, gi, whh, bhh, rzn, hn, hprev, hlast, steps_dev, B, T);
  else if (H == 64)
    hipLaunchKernelGGL(gst_gru_fwd_steps_kernel<64>, dim3(B), dim3(192), 0, (hipStream_t)stream, gi, whh, bhh, rzn, hn, hprev, hlast, steps_dev, B, T);
  else if (H == 32)
    hipLaunchKernelGGL(gst_gru_fwd_steps_kernel<32>, dim3(B), dim3(96), 0, (hipStream_t)stream, gi, whh, bhh, rzn, hn, hprev, hlast, steps_dev, B, T);
  else
    return fail(EVMI_ERR_UNSUPPORTED, "gst_gru_fwd_steps: hidden size 32, 64 or 128 (encoder.input_dim 64, 128 or 256)");
  EVMI_LAUNCH_CHECK("gst_gru_fwd_steps");
  return EVMI_OK;
}

int evmi_gst_gru_bwd_steps_f32(const float* rzn, const float* hn, const float* hprev, const float* whh, const float* dhlast, float* dgi,
                               float* dgh, const int* steps_dev, int B, int T, int H, void* stream) {
  if (!rzn || !hn || !hprev || !whh || !dhlast || !dgi || !dgh || !steps_dev || B < 1 || T < 1)
    return fail(EVMI_ERR_INVALID_ARG, "gst_gru_bwd_steps: bad arguments");
  if (H == 128)
    hipLaunchKernelGGL(gst_gru_bwd_steps_kernel<128>, dim3(B), dim3(384), 0, (hipStream_t)stream, rzn, hn, hprev, whh, dhlast, dgi, dgh, steps_dev, B, T);
  else if (H == 64)
    hipLaunchKernelGGL(gst_gru_bwd_steps_kernel<64>, dim3(B), dim3(192), 0, (hipStream_t)stream, rzn, hn, hprev, whh, dhlast, dgi, dgh, steps_dev, B, T);
  else if (H == 32)
    hipLaunchKernelGGL(gst_gru_bwd_steps_kernel<32>, dim3(B), dim3(96), 0, (hipStream_t)stream, rzn, hn, hprev, whh, dhlast, dgi, dgh, steps_dev, B, T);
  else
    return fail(EVMI_ERR_UNSUPPORTED, "gst_gru_bwd_steps: hidden size 32, 64 or 128 (encoder.input_dim 64, 128 or 256)");
  EVMI_LAUNCH_CHECK("gst_gru_bwd_steps");
  return EVMI_OK;
}

int evmi_gst_attention_fwd_f32(const float* q, const float* keys, const float* values, float* style, float* probs, int B, int N, int E,
                               int heads, void* stream) {
  if (!q || !keys || !values || !style || !attention_shape_ok(B, N, E, heads))
    return fail(EVMI_ERR_INVALID_ARG, "gst_attention_fwd: bad arguments (at most 16 tokens, E a multiple of 64 and of heads, E <= 1024)");
  const size_t lds = ((size_t)N * E + (size_t)heads * N) * sizeof(float);
  if (int rc = launch_with_lds(gst_attention_fwd_kernel, dim3(B), dim3(E), lds, (hipStream_t)stream, q, keys, values, style, probs, B, N, E, heads))
    return rc;
  EVMI_LAUNCH_CHECK("gst_attention_fwd");
  return EVMI_OK;
}

int evmi_gst_attention_bwd_f32(const float* dstyle, const float* q, const float* keys, const float* values, const float* probs, float* dq,
                               float* dkeys, float* dvalues, int B, int N, int E, int heads, void* stream) {
  if (!dstyle || !q || !keys || !values || !probs || !dq || !dkeys || !dvalues || !attention_shape_ok(B, N, E, heads))
    return fail(EVMI_ERR_INVALID_ARG, "gst_attention_bwd: bad arguments (at most 16 tokens, E a multiple of 64 and of heads, E <= 1024)");
  const size_t lds = ((size_t)N * E + 2 * (size_t)heads * N) * sizeof(float);
  if (int rc = launch_with_lds(gst_attention_bwd_kernel, dim3(1), dim3(E), lds, (hipStream_t)stream, dstyle, q, keys, values, probs, dq, dkeys,
                               dvalues, B, N, E, heads))
    return rc;
  EVMI_LAUNCH_CHECK("gst_attention_bwd");
  return EVMI_OK;
}

}  // extern "C"
