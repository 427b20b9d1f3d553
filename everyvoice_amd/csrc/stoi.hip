// Short-time objective intelligibility (Taal, Hendriks, Heusdens, Jensen 2011) of a synthesis against its recording:
// ref [B][S_ref] and deg [B][S_deg] fp32 waveforms at 10 kHz, one workgroup per item over its own n = min(len_ref, len_deg) samples.
// All arithmetic fp32, every sum in a fixed order, nothing per frame outside LDS and registers:
//
//   w      = hanning(258)[1:-1];  frame i = w . x[128 i : 128 i + 256] for every i with 128 i < n - 256:  F = ceil((n - 256) / 128)
//   e_i    = 20 log10(||frame i of ref|| + eps);  frame i is kept iff max_i e_i - 40 - e_i < 0;  K kept frames, k(.) their indices
//   the kept frames overlap-added at hop 128 and framed again are K - 1 frames:
//            new j = w . [tail(frame k(j-1)) + head(frame k(j)), tail(frame k(j)) + head(frame k(j+1))]      (no k(-1): zeros)
//   X_b[j] = sqrt(sum over the bins of band b of |DFT_512(new j)|^2), 15 one-third-octave bands over bins 7 .. 218
//   segment m = 30 .. K - 1 over columns m - 30 .. m - 1 (J = K - 30), per band with x, y the 30 values of ref and deg:
//            c = ||x|| / (||y|| + eps);  y' = min(c y, x (1 + 10^(15/20)));  both minus their mean, over (their norm + eps);  rho = sum x^ y'^
//   segment[s] = mean of rho over the bands;  stoi = mean of rho over all 15 J values
//
// The schedule (512 threads, 8 waves):
//   0. tables: the window and the 256 twiddles of the 512-point transform, made in double from short series, rounded once to fp32;
//   1. energies: a wave per frame of ref, four samples a lane, the wave's sum through DPP (wave_sum_dpp: a fixed order);
//   2. wave 0: the maximum, then the compaction 64 frames at a time (ballot + popcount): klist[k] = i.  K <= F is the only
//      data-dependent count of the kernel and every index made from it stays below F;
//   3. a wave per new frame, ref then deg: the 256 samples go into the wave's own 512 complex LDS slots with the first butterfly
//      stage applied (the upper half of the zero-padded input is zero: slot t = v, slot t + 256 = v W^t), eight more in-place
//      radix-2 stages (decimation in frequency, four butterflies a lane, the twiddle product compensated: stoi_diff_of_products;
//      bin k ends in slot bitreverse(k)), |X|^2 of bins 0 .. 255
//      back into the same slots, four lanes a band sum it (every fourth bin ascending, then (s0 + s1) + (s2 + s3)), sqrt -> LDS;
//   4. a thread per segment: the 15 bands one after the other, 30 + 30 values in registers, rho summed band 0 .. 14; the item's
//      value is the segment sums added by wave 0, lane l taking segments l, l + 64, .., then wave_sum_dpp.
// Every barrier sits outside the branches; the trip counts that hold one come from n and K alone.  An fmaxf skips a NaN energy and
// the comparison with a NaN is false, so a NaN frame is dropped; an Inf drops every frame.  No value moves an index.
#include <cmath>

#include "common.h"
#include "evmi.h"

namespace evmi {

constexpr int STOI_THREADS = 512;
constexpr int STOI_WAVES = STOI_THREADS / 64;
constexpr int STOI_FRAME = 256, STOI_HOP = 128, STOI_NFFT = 512, STOI_BANDS = 15, STOI_N = 30;
constexpr int STOI_LDS_BUDGET = 152 * 1024;  // of the 160 KiB of a compute unit
// LDS of a launch, in this order: fft [8 waves][512] float2 | tw [256] float2 | win [256] float | misc 64 bytes |
// energy [Fc] float (after phase 2: the segments' sums) | klist [Fc] int | xb [Fc][15] float | yb [Fc][15] float
constexpr int STOI_FIXED_BYTES = STOI_WAVES * STOI_NFFT * 8 + 256 * 8 + 256 * 4 + 64;
constexpr int STOI_FRAME_BYTES = 4 + 4 + 2 * STOI_BANDS * 4;
constexpr int STOI_MAX_FRAMES = (STOI_LDS_BUDGET - STOI_FIXED_BYTES) / STOI_FRAME_BYTES;
constexpr int STOI_MAX_N = STOI_FRAME + STOI_HOP * STOI_MAX_FRAMES;
static_assert(STOI_MAX_N >= 110000, "11 s at 10 kHz must fit");

__host__ __device__ inline int stoi_frames(int n) { return n > STOI_FRAME ? (n - STOI_FRAME + STOI_HOP - 1) / STOI_HOP : 0; }
// row strides of frame_of and segment at a padded length S (never below 1: the outputs are never empty)
inline int stoi_f_cap(int S) { return stoi_frames(S) > 1 ? stoi_frames(S) : 1; }
inline int stoi_j_cap(int S) { return stoi_frames(S) - STOI_N > 1 ? stoi_frames(S) - STOI_N : 1; }

// bins [edge[b], edge[b + 1]) of band b: centre 150 x 2^(b/3) Hz, edges x 2^(+-1/6), on the 257 bins of a 512-point transform at 10 kHz
__device__ const int stoi_band_edge[STOI_BANDS + 1] = {7, 9, 11, 14, 17, 22, 27, 34, 43, 55, 69, 87, 109, 138, 174, 219};

// cos and sin of 2 pi r, 0 <= r < 1, in double: the nearest quarter turn taken out, then the series on |angle| <= pi / 4 (error below
// 1e-16: the fp32 tables are these values rounded once)
__device__ inline void cos_sin_turn(double r, double& c, double& s) {
  const int quarter = (int)(r * 4.0 + 0.5);
  const double a = (r - 0.25 * quarter) * 6.283185307179586476925286766559;
  const double a2 = a * a;
  double cp = 1.0, sp = 1.0;
  for (int k = 18; k >= 2; k -= 2) {  // Horner from the far end: cos to a^18 / 18!, sin to a^19 / 19!
    cp = 1.0 - cp * a2 / (double)((k - 1) * k);
    sp = 1.0 - sp * a2 / (double)(k * (k + 1));
  }
  sp *= a;
  switch (quarter & 3) {
    case 0: c = cp; s = sp; break;
    case 1: c = -sp; s = cp; break;
    case 2: c = -cp; s = -sp; break;
    default: c = sp; s = -cp; break;
  }
}

// every LDS operation of this wave is complete and none is moved across (a wave's slots are its own: no workgroup barrier)
__device__ __forceinline__ void wave_lds_fence() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

// a b - c d with the rounding error of the product c d taken back out (two fmaf: c d = p + e exactly): the error is relative to the
// result, not to the products.  A bin that holds only a tone's leakage is a difference of products of its strong components; on such
// inputs the kernel's deviation from float64 fell by a quarter with this form.
__device__ __forceinline__ float stoi_diff_of_products(float a, float b, float c, float d) {
  const float p = c * d;
  const float e = fmaf(c, d, -p);
  return fmaf(a, b, -p) - e;
}

// stages 1 .. 8 of the 512-point decimation-in-frequency transform on the wave's slots (stage 0 is applied as the frame is stored)
__device__ __forceinline__ void stoi_fft_stages(float2* z, const float2* __restrict__ tw, int lane) {
#pragma unroll
  for (int s = 1; s < 9; ++s) {
    const int hb = 8 - s, half = 1 << hb;
    float2 a[4], c[4], w[4];
    int i0[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = lane + 64 * q, pos = b & (half - 1);
      i0[q] = ((b >> hb) << (hb + 1)) + pos;
      a[q] = z[i0[q]];
      c[q] = z[i0[q] + half];
      w[q] = tw[pos << s];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float dx = a[q].x - c[q].x, dy = a[q].y - c[q].y;
      z[i0[q]] = make_float2(a[q].x + c[q].x, a[q].y + c[q].y);
      z[i0[q] + half] = make_float2(stoi_diff_of_products(dx, w[q].x, dy, w[q].y), stoi_diff_of_products(dx, w[q].y, -dy, w[q].x));
    }
    wave_lds_fence();
  }
}

__global__ __launch_bounds__(STOI_THREADS) void stoi_kernel(const float* __restrict__ ref, const float* __restrict__ deg,
                                                            const int* __restrict__ ref_lens, const int* __restrict__ deg_lens,
                                                            float* __restrict__ stoi, int* __restrict__ counts, float* __restrict__ segment,
                                                            int* __restrict__ frame_of, int S_ref, int S_deg, int F_cap, int J_cap) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float2* fft = reinterpret_cast<float2*>(smem);
  float2* tw = fft + STOI_WAVES * STOI_NFFT;
  float* win = reinterpret_cast<float*>(tw + 256);
  int* misc = reinterpret_cast<int*>(win + 256);
  float* energy = reinterpret_cast<float*>(misc + 16);
  int* klist = reinterpret_cast<int*>(energy + F_cap);
  float* xb = reinterpret_cast<float*>(klist + F_cap);
  float* yb = xb + F_cap * STOI_BANDS;

  const int item = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int n = min(min(max(ref_lens[item], 0), S_ref), min(max(deg_lens[item], 0), S_deg));
  const int F = stoi_frames(n);  // <= F_cap: n <= min(S_ref, S_deg)
  const float* xr = ref + (long long)item * S_ref;
  const float* xd = deg + (long long)item * S_deg;
  const float eps = 2.220446049250313e-16f;

  // 0. tables
  if (tid < 256) {
    double c, s;
    cos_sin_turn((double)(tid + 1) / 257.0, c, s);
    win[tid] = (float)(0.5 - 0.5 * c);
    cos_sin_turn((double)tid / 512.0, c, s);
    tw[tid] = make_float2((float)c, (float)-s);
  }
  __syncthreads();

  // 1. energies of the reference's frames
  for (int i = wave; i < F; i += STOI_WAVES) {
    float acc = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = lane + 64 * q;
      const float v = win[t] * xr[i * STOI_HOP + t];
      acc = fmaf(v, v, acc);
    }
    acc = wave_sum_dpp(acc);
    if (lane == 0) energy[i] = 20.f * log10f(sqrtf(acc) + eps);
  }
  __syncthreads();

  // 2. the loudest frame, then the frames within 40 dB of it, in order
  if (wave == 0) {
    float emax = -INFINITY;
    for (int i = lane; i < F; i += 64) emax = fmaxf(emax, energy[i]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) emax = fmaxf(emax, __shfl_xor(emax, o));
    int K = 0;
    for (int i0 = 0; i0 < F; i0 += 64) {
      const int i = i0 + lane;
      const bool keep = i < F && (emax - 40.f - energy[i] < 0.f);
      const unsigned long long mask = __ballot(keep);
      if (keep) klist[K + __popcll(mask & ((1ull << lane) - 1ull))] = i;
      K += __popcll(mask);
    }
    if (lane == 0) misc[0] = K;
  }
  __syncthreads();
  const int K = min(misc[0], F);
  const int J = K > STOI_N ? K - STOI_N : 0;
  for (int k = tid; k < F_cap; k += STOI_THREADS) frame_of[(long long)item * F_cap + k] = k < K ? klist[k] : -1;
  if (tid == 0) {
    counts[3 * item] = F;
    counts[3 * item + 1] = K;
    counts[3 * item + 2] = J;
  }

  // 3. the band values of the K - 1 frames of the kept signal
  float2* z = fft + wave * STOI_NFFT;
  float* pw = reinterpret_cast<float*>(z);
  for (int j = wave; j < K - 1; j += STOI_WAVES) {
    const int k0 = j > 0 ? klist[j - 1] : -1, k1 = klist[j], k2 = klist[j + 1];
#pragma unroll
    for (int sig = 0; sig < 2; ++sig) {
      const float* x = sig ? xd : xr;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = lane + 64 * q;
        float a, b;
        if (q < 2) {  // t < 128: the tail of the frame before (zeros in front of the first) + the head of this one
          a = k0 >= 0 ? win[t + STOI_HOP] * x[k0 * STOI_HOP + STOI_HOP + t] : 0.f;
          b = win[t] * x[k1 * STOI_HOP + t];
        } else {  // the tail of this one + the head of the next
          a = win[t] * x[k1 * STOI_HOP + t];
          b = win[t - STOI_HOP] * x[k2 * STOI_HOP + t - STOI_HOP];
        }
        const float v = win[t] * (a + b);
        const float2 w = tw[t];
        z[t] = make_float2(v, 0.f);
        z[t + 256] = make_float2(v * w.x, v * w.y);
      }
      wave_lds_fence();
      stoi_fft_stages(z, tw, lane);
      float p[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const float2 v = z[__brev((unsigned)(lane + 64 * q)) >> 23];
        p[q] = v.x * v.x + v.y * v.y;
      }
      wave_lds_fence();
#pragma unroll
      for (int q = 0; q < 4; ++q) pw[lane + 64 * q] = p[q];
      wave_lds_fence();
      const int band = min(lane >> 2, STOI_BANDS - 1), part = lane & 3;
      float sum = 0.f;
      for (int bin = stoi_band_edge[band] + part; bin < stoi_band_edge[band + 1]; bin += 4) sum += pw[bin];
      sum += __shfl_xor(sum, 1);
      sum += __shfl_xor(sum, 2);
      if (lane < 4 * STOI_BANDS && part == 0) (sig ? yb : xb)[j * STOI_BANDS + band] = sqrtf(sum);
      wave_lds_fence();  // the slots are read before the next frame lands in them
    }
  }
  __syncthreads();

  // 4. the segments
  float* seg_sum = energy;
  const float clip = 6.623413251903491f;  // 1 + 10^(15 / 20)
  for (int s = tid; s < J; s += STOI_THREADS) {
    float total = 0.f;
    for (int band = 0; band < STOI_BANDS; ++band) {
      float x[STOI_N], y[STOI_N];
      float sxx = 0.f, syy = 0.f;
#pragma unroll
      for (int i = 0; i < STOI_N; ++i) {
        x[i] = xb[(s + i) * STOI_BANDS + band];
        y[i] = yb[(s + i) * STOI_BANDS + band];
        sxx = fmaf(x[i], x[i], sxx);
        syy = fmaf(y[i], y[i], syy);
      }
      const float c = sqrtf(sxx) / (sqrtf(syy) + eps);
      float mx = 0.f, my = 0.f;
#pragma unroll
      for (int i = 0; i < STOI_N; ++i) {
        y[i] = fminf(c * y[i], x[i] * clip);
        mx += x[i];
        my += y[i];
      }
      mx /= (float)STOI_N;
      my /= (float)STOI_N;
      sxx = 0.f, syy = 0.f;
#pragma unroll
      for (int i = 0; i < STOI_N; ++i) {
        x[i] -= mx;
        y[i] -= my;
        sxx = fmaf(x[i], x[i], sxx);
        syy = fmaf(y[i], y[i], syy);
      }
      const float nx = sqrtf(sxx) + eps, ny = sqrtf(syy) + eps;
      float rho = 0.f;
#pragma unroll
      for (int i = 0; i < STOI_N; ++i) rho = fmaf(x[i] / nx, y[i] / ny, rho);
      total += rho;
    }
    seg_sum[s] = total;
    segment[(long long)item * J_cap + s] = total / (float)STOI_BANDS;
  }
  for (int s = J + tid; s < J_cap; s += STOI_THREADS) segment[(long long)item * J_cap + s] = 0.f;
  __syncthreads();
  if (wave == 0) {
    float acc = 0.f;
    for (int s = lane; s < J; s += 64) acc += seg_sum[s];
    acc = wave_sum_dpp(acc);
    if (lane == 0) stoi[item] = J > 0 ? acc / (float)(STOI_BANDS * J) : NAN;
  }
}

}  // namespace evmi

using namespace evmi;

extern "C" {

int evmi_stoi_plan(int S, int* max_n, int* f_cap, int* j_cap) {
  if (!max_n || !f_cap || !j_cap) return fail(EVMI_ERR_INVALID_ARG, "stoi_plan: null pointer");
  if (S <= 0) return fail(EVMI_ERR_INVALID_ARG, "stoi_plan: shape");
  *max_n = STOI_MAX_N;
  *f_cap = stoi_f_cap(S < STOI_MAX_N ? S : STOI_MAX_N);
  *j_cap = stoi_j_cap(S < STOI_MAX_N ? S : STOI_MAX_N);
  return EVMI_OK;
}

int evmi_stoi_f32(const float* ref_dev, const float* deg_dev, const int* ref_lens_dev, const int* deg_lens_dev, float* stoi_dev,
                  int* counts_dev, float* segment_dev, int* frame_of_dev, int B, int S_ref, int S_deg, void* stream) {
  if (!ref_dev || !deg_dev || !ref_lens_dev || !deg_lens_dev || !stoi_dev || !counts_dev || !segment_dev || !frame_of_dev)
    return fail(EVMI_ERR_INVALID_ARG, "stoi: null pointer");
  if (B <= 0 || S_ref <= 0 || S_deg <= 0) return fail(EVMI_ERR_INVALID_ARG, "stoi: shape");
  const int S = S_ref < S_deg ? S_ref : S_deg;
  if (S > STOI_MAX_N)
    return fail(EVMI_ERR_UNSUPPORTED, "stoi: more than " + std::to_string(STOI_MAX_N) + " samples in the shorter row (" + std::to_string(S) +
                                          "): one workgroup's LDS holds " + std::to_string(STOI_MAX_FRAMES) + " frames");
  const int F_cap = stoi_f_cap(S), J_cap = stoi_j_cap(S);
  const size_t lds = STOI_FIXED_BYTES + (size_t)F_cap * STOI_FRAME_BYTES;
  if (int rc = launch_with_lds(stoi_kernel, dim3(B), dim3(STOI_THREADS), lds, (hipStream_t)stream, ref_dev, deg_dev, ref_lens_dev, deg_lens_dev,
                               stoi_dev, counts_dev, segment_dev, frame_of_dev, S_ref, S_deg, F_cap, J_cap))
    return rc;
  EVMI_LAUNCH_CHECK("stoi");
  return EVMI_OK;
}

}  // extern "C"
