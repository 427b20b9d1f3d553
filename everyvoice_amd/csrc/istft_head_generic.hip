// Generic-size iSTFTNet output head, gfx950: one fused launch (see istft_head_generic.h for the domain and the tiling, istft_head.hip
// for the arithmetic it restates).
//
//   z[f][c]  = b[c] + sum_{j<7} sum_ci W[c][ci][j] * xpad[f + j - 3][ci],   xpad[0] = x[1], xpad[q] = x[q-1],   c < n_fft + 2
//   re, im   = exp(z[f][b]) * (cos, sin)(sin(z[f][H + b])),   H = n_fft/2 + 1; interior bins doubled, im of bins 0 and H-1 dropped
//   y_f[k]   = w[k] / n_fft * sum_b ( re_b cos(2 pi b k / n_fft) - im_b sin(2 pi b k / n_fft) )
//   wav[t]   = sum_f y_f[t + n_fft/2 - hop f] / sum_f w^2[t + n_fft/2 - hop f]      (frames f in [0, L] that hold the sample)
//
// The contraction walks (64-channel group of the logits, 32-channel chunk of the input) the way conv_tc_generic_kernel does, on
// v_mfma_f32_16x16x32_bf16 with the lane maps of mfma16_layout.h; the accumulators go to an fp32 LDS tile [F][n_fft + 2] with the
// bias added and stay fp32 through exp / sin, the inverse DFT and the overlap-add.  16-channel tiles past n_fft + 2 are neither
// staged nor multiplied.
#include "istft_head_generic.h"

#include "mfma16_layout.h"

namespace evmi {

namespace {

struct H {
  static constexpr int NTHREADS = 256;  // four waves
  static constexpr int BM = kGenericBM, KC = kGenericKC, KS = kIstftKs;
  static constexpr int MT = BM / 16;
  static constexpr int XS = KC + 8, AS = KC + 8;  // LDS row strides (elements): odd multiples of 16 bytes
  static constexpr int VPT = KC / 8;              // 16-byte vectors per 32-channel row
  static constexpr int A_ELEMS = KS * BM * AS;
  static int polar_stride(int n_fft) { return n_fft + 2; }  // a frame's bins as (re, im) pairs: 8-byte aligned rows
  static size_t lds_bytes(int frames, int n_fft) {
    return (size_t)frames * polar_stride(n_fft) * 4 + (size_t)((frames + KS - 1) * XS + A_ELEMS) * 2;
  }
};

}  // namespace

// NT: 16-frame tiles per wave; the workgroup holds F = 64 NT frames.  lo = (n_fft/2 - 1) / hop halo frames in front, G = F - 2 lo - 1
// frames' worth of samples per workgroup.
template <int NT>
__global__ __launch_bounds__(H::NTHREADS) void istft_head_generic_kernel(const bf16_t* __restrict__ x,     // [B][L][C], activation applied
                                                                         const bf16_t* __restrict__ w,     // conv_tc_generic image
                                                                         const float* __restrict__ bias,   // [n_fft + 2]
                                                                         float* __restrict__ wav,          // [B][hop L]
                                                                         int Ls, int C, int n_fft, int hop,  // Ls: frames per item, the stride
                                                                         ItemLens lens) {  // ragged batch: item b holds item_rows(lens, b, Ls) frames
  constexpr int F = 64 * NT;
  constexpr int XROWS = F + H::KS - 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int co = n_fft + 2, bins = n_fft / 2 + 1, PS = n_fft + 2;
  float* Ps = reinterpret_cast<float*>(smem);                  // [F][bins][2]: logits (magnitude, angle) per bin, then (re, im)
  bf16_t* Xs = reinterpret_cast<bf16_t*>(Ps + F * PS);         // [XROWS][XS]
  bf16_t* As = Xs + XROWS * H::XS;                             // [7][64][AS]
  float2* tw = reinterpret_cast<float2*>(Xs);                  // after the contraction: (cos, sin)(2 pi i / n_fft) and the window
  float* win = reinterpret_cast<float*>(tw + n_fft);

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int b = blockIdx.y;
  const int lo = (n_fft / 2 - 1) / hop;
  const int G = F - 2 * lo - 1;
  const int F0 = blockIdx.x * G - lo;   // first frame of the tile
  const int T0 = blockIdx.x * G * hop;  // first output sample
  const int L = item_rows(lens, b, Ls);  // this item's frames: L + 1 spectral frames, the envelope of a sequence of L
  if (T0 >= hop * L) return;             // wholly at or beyond the item: before the first load
  const int n_frames = L + 1;
  const int nchunk = (C + H::KC - 1) / H::KC;
  const int ngroups = (co + H::BM - 1) / H::BM;
  const bf16_t* __restrict__ xb = x + (long long)b * Ls * C;

#pragma unroll 1
  for (int grp = 0; grp < ngroups; ++grp) {
    const int m0 = grp * H::BM;
    const int mt_active = (co - m0 + 15) / 16 < H::MT ? (co - m0 + 15) / 16 : H::MT;  // workgroup-uniform
    f32x4 acc[H::MT][NT];
#pragma unroll
    for (int i = 0; i < H::MT; ++i)
#pragma unroll
      for (int j = 0; j < NT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

#pragma unroll 1
    for (int chunk = 0; chunk < nchunk; ++chunk) {
      __syncthreads();  // everyone is done reading the previous operand tiles
      // activation rows: frame F0 + n reads padded rows F0 + n - 3 .. + 3; padded row q in [0, L] is x[q - 1] (q = 0: x[1]), zero outside
      for (int v = tid; v < XROWS * H::VPT; v += H::NTHREADS) {
        const int i = v / H::VPT, c = chunk * H::KC + (v % H::VPT) * 8;
        const int q = F0 - 3 + i;
        bf16x8 val;
#pragma unroll
        for (int e = 0; e < 8; ++e) val[e] = (bf16_t)0.f;
        if (q >= 0 && q <= L && c < C) {
          const int src = q == 0 ? (L > 1 ? 1 : 0) : q - 1;
          val = *reinterpret_cast<const bf16x8*>(xb + (long long)src * C + c);
        }
        *reinterpret_cast<bf16x8*>(Xs + i * H::XS + (v % H::VPT) * 8) = val;
      }
      // weights: the rows of the active 16-channel tiles of every tap of this (group, chunk)
      const bf16_t* wsrc = w + ((long long)grp * nchunk + chunk) * H::KS * H::BM * H::KC;
      const int a_rows = mt_active * 16;
      for (int v = tid; v < H::KS * a_rows * H::VPT; v += H::NTHREADS) {
        const int j = v / (a_rows * H::VPT), r = v % (a_rows * H::VPT);  // r: vector within the tap's active rows
        *reinterpret_cast<bf16x8*>(As + (j * H::BM + r / H::VPT) * H::AS + (r % H::VPT) * 8) =
            *reinterpret_cast<const bf16x8*>(wsrc + (long long)j * H::BM * H::KC + r * 8);
      }
      __syncthreads();
      // lane l: row (l & 15) of a 16-row tile, channel vector (l >> 4) of the 32-deep k-step, for both operands
      const bf16_t* Arow = As + mfma16::acc_row(lane) * H::AS + mfma16::frag_vec(lane, 0) * 8;
      const bf16_t* Brow = Xs + (wave * NT * 16 + mfma16::acc_row(lane)) * H::XS + mfma16::frag_vec(lane, 0) * 8;
#pragma unroll 1
      for (int j = 0; j < H::KS; ++j) {
        bf16x8 bfr[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) bfr[nt] = *reinterpret_cast<const bf16x8*>(Brow + (j + nt * 16) * H::XS);
#pragma unroll
        for (int mt = 0; mt < H::MT; ++mt) {
          if (mt < mt_active) {
            const bf16x8 af = *reinterpret_cast<const bf16x8*>(Arow + (j * H::BM + mt * 16) * H::AS);
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bfr[nt], acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
    // logits of this group, fp32, bias added: register i of a lane is channel m0 + 16 mt + 4 (l >> 4) + i of frame row (l & 15)
#pragma unroll
    for (int mt = 0; mt < H::MT; ++mt) {
      if (mt < mt_active) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int c = m0 + mt * 16 + mfma16::acc_channel(lane, i);
          if (c < co) {
            const float bv = bias[c];
            const int slot = c < bins ? 2 * c : 2 * (c - bins) + 1;  // magnitude logit of bin c | angle logit of bin c - bins
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) Ps[(wave * NT * 16 + nt * 16 + mfma16::acc_row(lane)) * PS + slot] = acc[mt][nt][i] + bv;
          }
        }
      }
    }
  }
  __syncthreads();  // logits complete; operand tiles dead: the tables alias them

  for (int i = tid; i < n_fft; i += H::NTHREADS) {
    const float th = 6.283185307179586f * i / n_fft;
    const float cs = cosf(th);
    tw[i] = make_float2(cs, sinf(th));
    win[i] = 0.5f - 0.5f * cs;
  }
  // z -> (re, im) in place; interior bins carry their factor 2, frames that do not exist are never read
  for (int v = tid; v < F * bins; v += H::NTHREADS) {
    const int n = v / bins, bb = v % bins;
    const int f = F0 + n;
    if (f < 0 || f >= n_frames) continue;
    float2* zp = reinterpret_cast<float2*>(Ps + n * PS) + bb;
    const float2 z = *zp;
    const float m = expf(z.x);
    const float phi = sinf(z.y);
    const bool edge = bb == 0 || bb == bins - 1;
    *zp = edge ? make_float2(m * cosf(phi), 0.f) : make_float2(2.f * (m * cosf(phi)), 2.f * (m * sinf(phi)));
  }
  __syncthreads();

  // inverse DFT sample by sample + overlap-add + envelope normalisation
  const int n_out = hop * L;
  const float inv_n = 1.f / n_fft;
  for (int v = tid; v < G * hop; v += H::NTHREADS) {
    const int t = T0 + v;
    if (t >= n_out) break;
    const int p = t + n_fft / 2;
    float s = 0.f, env = 0.f;
    for (int f = p / hop, k = p - hop * f; k < n_fft && f >= 0; --f, k += hop) {
      if (f >= n_frames) continue;
      const float2* zr = reinterpret_cast<const float2*>(Ps + (f - F0) * PS);
      // four bins per trip with their LDS reads independent of one another (the loop is latency-bound otherwise); i*: (bb * k) mod n_fft
      float a0 = 0.f, a1 = 0.f;
      int i0 = 0, bb = 0;
      for (; bb + 4 <= bins; bb += 4) {
        int i1 = i0 + k; i1 -= i1 >= n_fft ? n_fft : 0;
        int i2 = i1 + k; i2 -= i2 >= n_fft ? n_fft : 0;
        int i3 = i2 + k; i3 -= i3 >= n_fft ? n_fft : 0;
        const float2 z0 = zr[bb], z1 = zr[bb + 1], z2 = zr[bb + 2], z3 = zr[bb + 3];
        const float2 t0 = tw[i0], t1 = tw[i1], t2 = tw[i2], t3 = tw[i3];
        a0 += z0.x * t0.x - z0.y * t0.y;
        a1 += z1.x * t1.x - z1.y * t1.y;
        a0 += z2.x * t2.x - z2.y * t2.y;
        a1 += z3.x * t3.x - z3.y * t3.y;
        i0 = i3 + k; i0 -= i0 >= n_fft ? n_fft : 0;
      }
      for (; bb < bins; ++bb) {
        const float2 z0 = zr[bb], t0 = tw[i0];
        a0 += z0.x * t0.x - z0.y * t0.y;
        i0 += k; i0 -= i0 >= n_fft ? n_fft : 0;
      }
      const float wk = win[k];
      s += (a0 + a1) * wk * inv_n;
      env += wk * wk;
    }
    wav[(long long)b * hop * Ls + t] = s / env;
  }
}

int launch_istft_head_generic(const bf16_t* x, const bf16_t* w_img, const float* bias, float* wav, int B, int L, int C, int n_fft, int hop,
                              ItemLens lens, hipStream_t s) {
  if (!istft_head_channels_ok(C)) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_generic: C must be a multiple of 8 in [8, 512]");
  if (!istft_head_nfft_ok(n_fft)) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_generic: n_fft must be even in [4, 128]");
  if (!istft_head_hop_ok(n_fft, hop)) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_generic: hop must be in [1, n_fft / 2]");
  if (B < 1 || L < 1) return fail(EVMI_ERR_INVALID_ARG, "istft_head_generic: B and L must be positive");
  if (B > 65535 || (long long)hop * L > 0x7fffffffll - 2 * kIstftMaxNfft)
    return fail(EVMI_ERR_INVALID_ARG, "istft_head_generic: more than 65535 items or 2^31 samples per item");
  const int F = istft_head_frame_tile(n_fft, hop);
  const int G = F - istft_head_halo(n_fft, hop);
  const size_t lds = H::lds_bytes(F, n_fft);
  if (G < 1 || lds > 160 * 1024) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_generic: tile does not fit");
  dim3 grid((unsigned)((L + G - 1) / G), B);
  const auto kernel = F == 64 ? istft_head_generic_kernel<1> : F == 128 ? istft_head_generic_kernel<2> : istft_head_generic_kernel<3>;
  if (int rc = launch_with_lds(kernel, grid, dim3(H::NTHREADS), lds, s, x, w_img, bias, wav, L, C, n_fft, hop, lens)) return rc;
  EVMI_LAUNCH_CHECK("istft_head_generic");
  return EVMI_OK;
}

int launch_istft_head(const bf16_t*, const bf16_t*, const float*, float*, int, int, int, ItemLens, hipStream_t);  // istft_head.hip

namespace {

// w fp32 [co][C][7] (torch) -> the zero-padded generic image; one thread per image element
__global__ void istft_relayout_generic_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst, int co, int C, long long n) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int ci = (int)(r % H::KC); r /= H::KC;
  const int mi = (int)(r % H::BM); r /= H::BM;
  const int j = (int)(r % H::KS); r /= H::KS;
  const int nch = (C + H::KC - 1) / H::KC;
  const int chn = (int)(r % nch); r /= nch;
  const int m = (int)r * H::BM + mi, c = chn * H::KC + ci;
  dst[idx] = (bf16_t)((m < co && c < C) ? w[((long long)m * C + c) * H::KS + j] : 0.f);
}

// ... -> the specialised kernel's [7][32][C] image (rows >= 18 zero) and its bias padded to 32
__global__ void istft_relayout_specialised_kernel(const float* __restrict__ w, const float* __restrict__ bias, bf16_t* __restrict__ dst,
                                                  float* __restrict__ bias32, int C) {
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx < 32) bias32[idx] = idx < 18 ? bias[idx] : 0.f;
  if (idx >= H::KS * 32 * C) return;
  const int ci = idx % C, m = (idx / C) % 32, j = idx / (32 * C);
  dst[idx] = (bf16_t)(m < 18 ? w[((long long)m * C + ci) * H::KS + j] : 0.f);
}

long long head_weight_elems(int C, int n_fft) {
  const long long gen = conv_generic_weight_elems(C, n_fft + 2, H::KS), spec = (long long)H::KS * 32 * C;
  return (gen > spec ? gen : spec) + 64;  // + the specialised kernel's padded bias (32 floats)
}

}  // namespace

}  // namespace evmi

using namespace evmi;

extern "C" {

long long evmi_istft_head_weight_elems(int C, int n_fft) {
  if (!istft_head_channels_ok(C) || !istft_head_nfft_ok(n_fft)) return 0;
  return head_weight_elems(C, n_fft);
}

int evmi_istft_head_frame_tile(int n_fft, int hop) {
  if (!istft_head_nfft_ok(n_fft) || !istft_head_hop_ok(n_fft, hop)) return 0;
  return istft_head_frame_tile(n_fft, hop);
}

int evmi_istft_head_bf16(const void* x_dev, const float* w_dev, const float* bias_dev, void* w_laid_dev, float* wav_dev, int B, int L,
                         int C, int n_fft, int hop, int variant, void* stream) {
  if (!x_dev || !w_dev || !bias_dev || !w_laid_dev || !wav_dev) return fail(EVMI_ERR_INVALID_ARG, "istft_head_bf16: null pointer");
  if (B < 1 || L < 1) return fail(EVMI_ERR_INVALID_ARG, "istft_head_bf16: B and L must be positive");
  if (variant != 0 && variant != 1) return fail(EVMI_ERR_INVALID_ARG, "istft_head_bf16: variant must be 0 (the generator's choice) or 1 (generic)");
  if (!istft_head_channels_ok(C)) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_bf16: C must be a multiple of 8 in [8, 512]");
  if (!istft_head_nfft_ok(n_fft)) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_bf16: n_fft must be even in [4, 128]");
  if (!istft_head_hop_ok(n_fft, hop)) return fail(EVMI_ERR_UNSUPPORTED, "istft_head_bf16: hop must be in [1, n_fft / 2]");
  if (B > 65535 || (long long)hop * L > 0x7fffffffll - 2 * kIstftMaxNfft)
    return fail(EVMI_ERR_INVALID_ARG, "istft_head_bf16: more than 65535 items or 2^31 samples per item");
  hipStream_t s = (hipStream_t)stream;
  const bf16_t* x = reinterpret_cast<const bf16_t*>(x_dev);
  bf16_t* img = reinterpret_cast<bf16_t*>(w_laid_dev);
  if (variant == 0 && istft_head_specialised(C, n_fft, hop)) {
    float* bias32 = reinterpret_cast<float*>(img + (size_t)H::KS * 32 * C);
    const int n = H::KS * 32 * C;
    hipLaunchKernelGGL(istft_relayout_specialised_kernel, dim3((n + 255) / 256), dim3(256), 0, s, w_dev, bias_dev, img, bias32, C);
    EVMI_LAUNCH_CHECK("istft_relayout_specialised");
    return launch_istft_head(x, img, bias32, wav_dev, B, L, C, ItemLens{}, s);
  }
  const long long n = conv_generic_weight_elems(C, n_fft + 2, H::KS);
  hipLaunchKernelGGL(istft_relayout_generic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, w_dev, img, n_fft + 2, C, n);
  EVMI_LAUNCH_CHECK("istft_relayout_generic");
  return launch_istft_head_generic(x, img, bias_dev, wav_dev, B, L, C, n_fft, hop, ItemLens{}, s);
}

}  // extern "C"
