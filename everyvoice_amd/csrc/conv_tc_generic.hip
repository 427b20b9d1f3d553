// Generic-shape bf16 MFMA implicit-GEMM convolution, gfx950.  See conv_tc_generic.h for the tiling and the limits, conv_tc_mfma.h
// for the contract.  Register-staged like conv_tc_kernel.h (global -> registers -> LDS for both operands: per-vector guards are
// cheap there), on the lane maps of mfma16_layout.h.
#include "conv_tc_generic.h"

#include <type_traits>

#include "mfma16_layout.h"

namespace evmi {

namespace {

struct G {
  static constexpr int BM = kGenericBM, BN = kGenericBN, KC = kGenericKC, HALO = kGenericMaxHalo;
  static constexpr int NTHREADS = 256, NWAVES = 4;
  static constexpr int MT = BM / 16, NT = BN / (NWAVES * 16);  // 16 x 16 tiles per wave: 4 x 4
  static constexpr int TAPS = 4;                               // taps per weight stage (one barrier per stage)
  static constexpr int XS = KC + 8, AS = KC + 8, OS = BM + 8;  // LDS row strides (elements): odd multiples of 16 bytes
  static constexpr int R_MAX = BN + HALO;
  static constexpr int A_TILE = TAPS * BM * AS;
  static constexpr int VPT = KC / 8;  // 16-byte vectors per 32-channel row
  static constexpr size_t LDS_MAIN = size_t(R_MAX * XS + 2 * A_TILE) * 2;
  static constexpr size_t LDS_OUT = size_t(BN) * OS * 2;
  static constexpr size_t LDS = LDS_MAIN > LDS_OUT ? LDS_MAIN : LDS_OUT;
  static_assert(BM * VPT == NTHREADS, "one weight vector per thread and tap");
  static_assert(2 * LDS <= 160 * 1024, "two workgroups per CU");
};

}  // namespace

__global__ __launch_bounds__(G::NTHREADS, 2) void conv_tc_generic_kernel(ConvTcArgs a, int c_in, int ks) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* Xs = reinterpret_cast<bf16_t*>(smem);
  bf16_t* As = Xs + G::R_MAX * G::XS;

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int r0 = blockIdx.x * G::BN;
  const int b = blockIdx.y;
  const int mtile = blockIdx.z;
  const int m0 = mtile * G::BM;
  int t_in, n_rows;  // of this item (ragged batch: its own, conv_tc_mfma.h)
  long long out_limit;
  if (!conv_item_extents(a, b, r0, t_in, n_rows, out_limit)) return;
  const int nchunk = (c_in + G::KC - 1) / G::KC;
  const int ngroup = (ks + G::TAPS - 1) / G::TAPS;
  const int nstep = nchunk * ngroup;
  // 16-channel tiles of this workgroup that hold a real output channel (workgroup-uniform): the others issue no MFMA
  const int mt_active = (a.c_out - m0 + 15) / 16 < G::MT ? (a.c_out - m0 + 15) / 16 : G::MT;

  const bf16_t* __restrict__ xb = a.x + (long long)b * a.x_batch_stride;
  const bf16_t* __restrict__ wb = a.w + (long long)mtile * nchunk * ks * G::BM * G::KC;

  f32x4 acc[G::MT][G::NT];
#pragma unroll
  for (int i = 0; i < G::MT; ++i)
#pragma unroll
    for (int j = 0; j < G::NT; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) acc[i][j][r] = 0.f;

  // weights of one stage (up to TAPS taps of one chunk): thread t holds vector (t % 4) of row (t / 4) of every tap
  bf16x8 areg[G::TAPS];
  auto taps_of = [&](int grp) { return ks - grp * G::TAPS < G::TAPS ? ks - grp * G::TAPS : G::TAPS; };
  auto a_prefetch = [&](int step) {
    const int chunk = step / ngroup, grp = step % ngroup;
    const bf16_t* src = wb + ((long long)chunk * ks + grp * G::TAPS) * G::BM * G::KC + tid * 8;
    const int ntaps = taps_of(grp);
#pragma unroll
    for (int i = 0; i < G::TAPS; ++i)
      if (i < ntaps) areg[i] = *reinterpret_cast<const bf16x8*>(src + (long long)i * G::BM * G::KC);
  };
  auto a_commit = [&](int step) {
    bf16_t* dst = As + (step & 1) * G::A_TILE + (tid / G::VPT) * G::AS + (tid % G::VPT) * 8;
    const int ntaps = taps_of(step % ngroup);
#pragma unroll
    for (int i = 0; i < G::TAPS; ++i)
      if (i < ntaps) *reinterpret_cast<bf16x8*>(dst + i * G::BM * G::AS) = areg[i];
  };

  const int rows_needed = G::BN + (ks - 1) * a.dil;  // <= R_MAX: checked by the launcher
  const int x_nvec = rows_needed * G::VPT;
  const float pre = a.pre_slope;

  a_prefetch(0);
#pragma unroll 1
  for (int chunk = 0; chunk < nchunk; ++chunk) {
    if (chunk > 0) __syncthreads();  // everyone is done reading the previous chunk's rows
    // ---- activation tile: rows [r0 - pad, r0 - pad + rows_needed) x channels [32 chunk, 32 chunk + 32), zero outside the tensor
#pragma unroll 1
    for (int v0 = 0; v0 < x_nvec; v0 += 4 * G::NTHREADS) {
      bf16x8 xv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {  // four requests in flight per round trip
        const int v = v0 + tid + i * G::NTHREADS;
        const int row = v / G::VPT, c = chunk * G::KC + (v % G::VPT) * 8;
        const int rr = r0 - a.pad + row;
        bf16x8 val;
#pragma unroll
        for (int e = 0; e < 8; ++e) val[e] = (bf16_t)0.f;
        if (v < x_nvec && c < c_in && rr >= 0 && rr < t_in) val = *reinterpret_cast<const bf16x8*>(xb + (long long)rr * c_in + c);
        xv[i] = val;
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int v = v0 + tid + i * G::NTHREADS;
        if (v >= x_nvec) continue;
        bf16x8 val = xv[i];
        if (pre != 1.f) {  // slope in [0, 1]: lrelu(x) = max(x, slope * x)
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            const float f = (float)val[e];
            val[e] = (bf16_t)fmaxf(f, f * pre);
          }
        }
        *reinterpret_cast<bf16x8*>(Xs + (v / G::VPT) * G::XS + (v % G::VPT) * 8) = val;
      }
    }
#pragma unroll 1
    for (int grp = 0; grp < ngroup; ++grp) {
      const int step = chunk * ngroup + grp;
      a_commit(step);
      __syncthreads();
      if (step + 1 < nstep) a_prefetch(step + 1);
      const int ntaps = taps_of(grp);
      // lane l: row (l & 15) of a 16-row tile, channel vector (l >> 4) of the 32-deep k-step, for both operands
      const bf16_t* Arow = As + (step & 1) * G::A_TILE + mfma16::acc_row(lane) * G::AS + mfma16::frag_vec(lane, 0) * 8;
      const bf16_t* Brow = Xs + (wave * G::NT * 16 + mfma16::acc_row(lane) + grp * G::TAPS * a.dil) * G::XS + mfma16::frag_vec(lane, 0) * 8;
#pragma unroll 1
      for (int j = 0; j < ntaps; ++j) {
        bf16x8 af[G::MT], bfr[G::NT];
#pragma unroll
        for (int mt = 0; mt < G::MT; ++mt) af[mt] = *reinterpret_cast<const bf16x8*>(Arow + (j * G::BM + mt * 16) * G::AS);
#pragma unroll
        for (int nt = 0; nt < G::NT; ++nt) bfr[nt] = *reinterpret_cast<const bf16x8*>(Brow + (j * a.dil + nt * 16) * G::XS);
#pragma unroll
        for (int mt = 0; mt < G::MT; ++mt) {
          if (mt < mt_active) {
#pragma unroll
            for (int nt = 0; nt < G::NT; ++nt)
              acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[mt], bfr[nt], acc[mt][nt], 0, 0, 0);
          }
        }
      }
    }
  }

  // ---- epilogue: acc + bias -> bf16 -> LDS [BN][BM + 8] -> coalesced fused store (the arithmetic of conv_tc_kernel.h) ----------
  __syncthreads();
  bf16_t* Os = reinterpret_cast<bf16_t*>(smem);
#pragma unroll
  for (int mt = 0; mt < G::MT; ++mt) {
    const int c = mt * 16 + mfma16::acc_channel(lane, 0);  // four consecutive channels per lane
    f32x4 bv;
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = 0.f;
    if (m0 + c < a.c_out) bv = *reinterpret_cast<const f32x4*>(a.bias + m0 + c);  // c_out is a multiple of 8: all four or none
#pragma unroll
    for (int nt = 0; nt < G::NT; ++nt) {
      const int n = wave * G::NT * 16 + nt * 16 + mfma16::acc_row(lane);
      bf16x4 pk;
#pragma unroll
      for (int i = 0; i < 4; ++i) pk[i] = (bf16_t)(acc[mt][nt][i] + bv[i]);
      *reinterpret_cast<bf16x4*>(Os + n * G::OS + c) = pk;
    }
  }
  __syncthreads();
  {
    const long long ob = (long long)b * a.out_batch_stride;
    const float scale = a.out_scale, post = a.post_slope;
    constexpr int VPR = G::BM / 8;
    constexpr int OPT = G::BN * VPR / G::NTHREADS;  // output vectors per thread
    constexpr int EB = 4;                           // vectors per batch of residual / running-sum loads
    static_assert(OPT % EB == 0, "epilogue batches");
    auto flat_index = [&](int v) -> long long {
      const int n = v / VPR, c8 = v % VPR;
      const int r = r0 + n;
      const long long flat = (long long)r * a.out_row_stride + m0 + c8 * 8 + a.out_shift;
      return (r >= n_rows || m0 + c8 * 8 >= a.c_out || flat < 0 || flat >= out_limit) ? -1 : flat;
    };
    const float mslope = a.mask_slope;
    auto body = [&](auto has_res, auto has_acc, auto has_mask) {
      constexpr bool RES = decltype(has_res)::value, ACC = decltype(has_acc)::value, MSK = decltype(has_mask)::value;
#pragma unroll
      for (int i0 = 0; i0 < OPT; i0 += EB) {
        bf16x8 rv[EB], pv[EB], mv[EB];
#pragma unroll
        for (int i = 0; i < EB; ++i) {
          // unconditional loads (vectors that are not stored read element 0 of the item), as in conv_tc_kernel.h
          const long long flat = flat_index(tid + (i0 + i) * G::NTHREADS);
          const long long safe = flat < 0 ? 0 : flat;
          if (RES) rv[i] = *reinterpret_cast<const bf16x8*>(a.res + ob + safe);
          if (ACC) pv[i] = *reinterpret_cast<const bf16x8*>(a.out + ob + safe);
          if (MSK) mv[i] = *reinterpret_cast<const bf16x8*>(a.mask + ob + safe);
        }
#pragma unroll
        for (int i = 0; i < EB; ++i) {
          const int v = tid + (i0 + i) * G::NTHREADS;
          const long long flat = flat_index(v);
          const bf16x8 o = *reinterpret_cast<const bf16x8*>(Os + (v / VPR) * G::OS + (v % VPR) * 8);
          float f[8];
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] = (float)o[e];
          if (MSK) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] = (float)mv[i][e] > 0.f ? f[e] : f[e] * mslope;
          }
          if (RES) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += (float)rv[i][e];
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] *= scale;
          if (ACC) {
#pragma unroll
            for (int e = 0; e < 8; ++e) f[e] += (float)pv[i][e];
          }
          bf16x8 res;
#pragma unroll
          for (int e = 0; e < 8; ++e) res[e] = (bf16_t)(post != 1.f ? lrelu(f[e], post) : f[e]);
          if (flat >= 0) *reinterpret_cast<bf16x8*>(a.out + ob + flat) = res;
        }
      }
    };
    using T_ = std::integral_constant<bool, true>;
    using F_ = std::integral_constant<bool, false>;
    if (a.mask) {  // (training launches: never with a running sum)
      if (a.res) body(T_{}, F_{}, T_{});
      else body(F_{}, F_{}, T_{});
    } else if (a.res) {
      if (a.accumulate) body(T_{}, T_{}, F_{});
      else body(T_{}, F_{}, F_{});
    } else {
      if (a.accumulate) body(F_{}, T_{}, F_{});
      else body(F_{}, F_{}, F_{});
    }
  }
}

const char* conv_generic_refusal(int c_in, int c_out, int ks, int dil) {
  if (c_in <= 0 || c_out <= 0 || (c_in & 7) || (c_out & 7)) return "channel counts must be positive multiples of 8";
  if (ks < 1 || dil < 1) return "kernel size and dilation must be at least 1";
  if ((long long)(ks - 1) * dil > kGenericMaxHalo) return "(ks - 1) * dil exceeds the halo limit of 256 rows";
  return nullptr;
}

int launch_conv_generic(const ConvTcArgs& a, int c_in, int ks, int B, hipStream_t stream) {
  if (const char* why = conv_generic_refusal(c_in, a.c_out, ks, a.dil)) return fail(EVMI_ERR_UNSUPPORTED, std::string("conv_tc_generic: ") + why);
  if (B <= 0 || a.n_rows <= 0 || a.t_in <= 0) return fail(EVMI_ERR_INVALID_ARG, "conv_tc_generic: B, n_rows and t_in must be positive");
  const long long mtiles = (a.c_out + G::BM - 1) / G::BM;
  if (B > 65535 || mtiles > 65535) return fail(EVMI_ERR_INVALID_ARG, "conv_tc_generic: more than 65535 items or channel tiles");
  dim3 grid((a.n_rows + G::BN - 1) / G::BN, B, (unsigned)mtiles);
  ConvTcArgs args = a;
  args.n_items = B;
  if (int rc = launch_with_lds(conv_tc_generic_kernel, grid, dim3(G::NTHREADS), G::LDS, stream, args, c_in, ks)) return rc;
  EVMI_LAUNCH_CHECK("conv_tc_generic");
  return EVMI_OK;
}

// w fp32 [c_out][c_in][ks] (torch) -> the zero-padded image; one thread per image element
__global__ void relayout_generic_kernel(const float* __restrict__ w, bf16_t* __restrict__ dst, int c_out, int c_in, int ks, long long n) {
  const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= n) return;
  long long r = idx;
  const int ci = (int)(r % G::KC); r /= G::KC;
  const int mi = (int)(r % G::BM); r /= G::BM;
  const int j = (int)(r % ks); r /= ks;
  const int nch = (c_in + G::KC - 1) / G::KC;
  const int chn = (int)(r % nch); r /= nch;
  const int m = (int)r * G::BM + mi, c = chn * G::KC + ci;
  dst[idx] = (bf16_t)((m < c_out && c < c_in) ? w[((long long)m * c_in + c) * ks + j] : 0.f);
}

}  // namespace evmi

using namespace evmi;

extern "C" {

long long evmi_conv_generic_weight_elems(int c_in, int c_out, int ks) {
  if (c_in <= 0 || c_out <= 0 || ks <= 0) return 0;
  return conv_generic_weight_elems(c_in, c_out, ks);
}

int evmi_conv_generic_relayout_f32(const float* w_dev, void* dst_bf16_dev, int c_in, int c_out, int ks, void* stream) {
  if (!w_dev || !dst_bf16_dev) return fail(EVMI_ERR_INVALID_ARG, "conv_generic_relayout: null pointer");
  if (const char* why = conv_generic_refusal(c_in, c_out, ks, 1)) return fail(EVMI_ERR_UNSUPPORTED, std::string("conv_generic_relayout: ") + why);
  const long long n = conv_generic_weight_elems(c_in, c_out, ks);
  hipLaunchKernelGGL(relayout_generic_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w_dev,
                     reinterpret_cast<bf16_t*>(dst_bf16_dev), c_out, c_in, ks, n);
  EVMI_LAUNCH_CHECK("relayout_generic");
  return EVMI_OK;
}

int evmi_conv_generic_bf16(const void* x, const void* w_laid, const float* bias_dev, const void* res, void* out, int B, int t_in, int n_rows,
                           int c_in, int c_out, int ks, int dil, int pad, long long out_row_stride, long long out_shift, long long out_limit,
                           float pre_slope, float post_slope, float out_scale, int accumulate, void* stream) {
  if (!x || !w_laid || !bias_dev || !out) return fail(EVMI_ERR_INVALID_ARG, "conv_generic: null pointer");
  if (B <= 0 || t_in <= 0 || n_rows <= 0 || pad < 0) return fail(EVMI_ERR_INVALID_ARG, "conv_generic: shape");
  if (out_row_stride <= 0 || out_limit <= 0 || (out_row_stride & 7) || (out_shift & 7) || (out_limit & 7))
    return fail(EVMI_ERR_INVALID_ARG, "conv_generic: out_row_stride, out_shift and out_limit must be multiples of 8 elements (row stride and limit positive)");
  ConvTcArgs a = {};
  a.x = reinterpret_cast<const bf16_t*>(x);
  a.w = reinterpret_cast<const bf16_t*>(w_laid);
  a.bias = bias_dev;
  a.res = reinterpret_cast<const bf16_t*>(res);
  a.out = reinterpret_cast<bf16_t*>(out);
  a.t_in = t_in; a.n_rows = n_rows; a.c_out = c_out; a.dil = dil; a.pad = pad;
  a.x_batch_stride = (long long)t_in * c_in;
  a.out_batch_stride = out_limit;
  a.out_row_stride = out_row_stride; a.out_shift = out_shift; a.out_limit = out_limit;
  a.pre_slope = pre_slope; a.post_slope = post_slope; a.out_scale = out_scale; a.accumulate = accumulate ? 1 : 0;
  a.mask_slope = 1.f;
  return launch_conv_generic(a, c_in, ks, B, (hipStream_t)stream);
}

}  // extern "C"
