// Alignment at inference: the projected mel q [A][B][T] and text k [A][B][L] of the aligner straight to the
// integer durations [B][L] of the monotonic search, one workgroup per item over that item's own T_b frames and L_b tokens.
//
//   value[y][x] = -temperature * sum_a (q[a][y] - k[a][x])^2  (+ logf((float)prior[y][x] + 1e-8f))     fp32, a ascending, fmaf
//   Q[y][x]     = value[y][x] + max(Q[y-1][x-1], Q[y-1][x])    over the band max(0, L_b + y - T_b) <= x < min(L_b, y + 1)
//   read back from (T_b - 1, L_b - 1): move to x - 1 when x == y or Q[y-1][x] < Q[y-1][x-1]            (mas_kernel, fs2_ops.hip)
//
// The two softmax normalisers of the training chain (log_softmax over the tokens in front of the prior, softmax behind it) are
// constants of a frame; every monotonic path visits each frame exactly once, so they shift all paths alike and are not computed.
//
// The frames go through the workgroup (1024 threads) in tiles of TY frames, as many as the LDS holds at the launch's L and A (24 .. 64):
//   1. the tile's q columns are staged in LDS (t is the contiguous axis of q: a frame at a time would be a strided read);
//   2. value pass: the tile is cut into units of 64 tokens x 8 consecutive frames, dealt round-robin to the 16 waves.  A lane owns a
//      token of its unit: the 8 q values of a channel are two broadcast 16-byte LDS reads, the key value comes from the item's k image
//      in LDS (where A * L fits beside the rest) or from global memory, differences and fmaf run two frames an instruction (packed
//      fp32).  Cells outside the band are not computed;
//   3. search: frames in sequence, thread x holds token x: Q[y-1][x] in a register, Q[y-1][x-1] through two LDS rows, one LDS-only
//      barrier per frame; the decision of each cell (one byte) is collected in LDS and leaves for the workspace once per tile.
// The read-back pulls the decisions back through LDS in chunks of whole rows and one thread walks them there.
#include <cmath>

#include "common.h"
#include "evmi.h"

namespace evmi {

constexpr int AD_THREADS = 1024;
constexpr int AD_WAVES = AD_THREADS / 64;
constexpr int AD_FPT = 8;  // frames of one unit of the value pass
constexpr int AD_MAX_A = 128;
constexpr int AD_MAX_L = AD_THREADS;
constexpr int AD_MAX_TY = 64;
constexpr int AD_LDS_BUDGET = 152 * 1024;  // of the 160 KiB of a compute unit
typedef float f32x2 __attribute__((ext_vector_type(2)));

__host__ __device__ inline int ad_row_stride(int L) { return (L + 15) & ~15; }  // bytes of a workspace row: 16-byte vectors

// LDS of a launch, in this order: vals [TY][VS] floats | rows [2][VS] floats | qs [A][TY] floats | (ks [A][VS] floats) | dec [TY][VS] bytes
struct AdPlan {
  int ty, vs;
  bool k_in_lds;
  size_t bytes;
};
inline AdPlan ad_plan(int A, int L) {
  AdPlan p;
  p.vs = (L + 63) & ~63;
  const size_t rows = (size_t)2 * p.vs * 4, per_frame = (size_t)5 * p.vs + 4 * A, ks = (size_t)A * p.vs * 4;
  auto frames = [&](size_t fixed) { return fixed >= (size_t)AD_LDS_BUDGET ? 0 : (int)min((size_t)AD_MAX_TY, (AD_LDS_BUDGET - fixed) / per_frame) & ~7; };
  p.k_in_lds = frames(rows + ks) >= 32;  // (a smaller tile costs more than reading k through the caches)
  p.ty = frames(rows + (p.k_in_lds ? ks : 0));
  p.bytes = rows + (p.k_in_lds ? ks : 0) + (size_t)p.ty * per_frame;
  return p;
}

template <bool KLDS>
__global__ __launch_bounds__(AD_THREADS) void align_durations_kernel(const float* __restrict__ q, const float* __restrict__ k,
                                                                     const double* __restrict__ prior, const int* __restrict__ text_lens,
                                                                     const int* __restrict__ mel_lens, int* __restrict__ dur,
                                                                     unsigned char* __restrict__ ws, int A, int B, int T, int L, int TY,
                                                                     int VS, float temperature) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  float* vals = reinterpret_cast<float*>(smem);
  float* rows = vals + TY * VS;
  float* qs = rows + 2 * VS;
  float* ks = qs + A * TY;
  unsigned char* dec = reinterpret_cast<unsigned char*>(KLDS ? ks + A * VS : ks);

  const int b = blockIdx.x, tid = threadIdx.x;
  const int Lb = min(max(text_lens[b], 0), L), Tb = min(max(mel_lens[b], 0), T);
  int* drow = dur + (long long)b * L;
  for (int l = tid; l < L; l += AD_THREADS) drow[l] = 0;
  if (Lb == 0 || Tb == 0 || Tb < Lb) return;  // no path uses every token: the row of zeros

  const int WX = (Lb + 63) >> 6;  // waves across the item's tokens
  const int lane = tid & 63, wave = tid >> 6;
  const int Lp = ad_row_stride(L);
  unsigned char* wsb = ws + (long long)b * T * Lp;
  const float* kb = k + (long long)b * L;
  const float MAX_NEG = -1e9f;

  if (KLDS) {
    for (int i = tid; i < A * VS; i += AD_THREADS) {
      const int a = i / VS, x = i - a * VS;
      ks[i] = x < Lb ? kb[(long long)a * B * L + x] : 0.f;
    }
  }
  __syncthreads();  // (also: the zeroed duration row has landed before the read-back stores into it)

  float own = MAX_NEG;  // Q[y - 1][x] of this thread's token x = tid in the search

  for (int y0 = 0; y0 < Tb; y0 += TY) {
    const int ny = min(TY, Tb - y0);
    // 1. q columns of the tile: qs[a][yy]
    for (int i = tid; i < A * TY; i += AD_THREADS) {
      const int a = i / TY, yy = i - a * TY;
      qs[i] = yy < ny ? q[((long long)a * B + b) * T + y0 + yy] : 0.f;
    }
    __syncthreads();
    // 2. values of the band cells of the tile: unit u = (frame group g, token wave) -> wave u % 16
    const int units = ((ny + AD_FPT - 1) / AD_FPT) * WX;
    for (int u = wave; u < units; u += AD_WAVES) {
      const int g = u / WX, x = (u - g * WX) * 64 + lane;
      const int ya = y0 + g * AD_FPT, yb = min(ya + AD_FPT, Tb) - 1;  // this unit's frames [ya, yb]
      if (!(x < Lb && x <= yb && x >= Lb + ya - Tb)) continue;        // no cell of this token's 8 is inside the band
      double pr[AD_FPT];  // (asked for here, used behind the channel loop)
      if (prior) {
#pragma unroll
        for (int f = 0; f < AD_FPT; ++f) pr[f] = prior[((long long)b * T + min(ya + f, Tb - 1)) * L + x];
      }
      f32x2 acc[AD_FPT / 2];
#pragma unroll
      for (int f = 0; f < AD_FPT / 2; ++f) acc[f] = f32x2{0.f, 0.f};
      const float* qrow = qs + g * AD_FPT;
#pragma unroll 4
      for (int a = 0; a < A; ++a) {
        const f32x4 q0 = *reinterpret_cast<const f32x4*>(qrow + a * TY), q1 = *reinterpret_cast<const f32x4*>(qrow + a * TY + 4);
        const f32x2 qp[4] = {f32x2{q0[0], q0[1]}, f32x2{q0[2], q0[3]}, f32x2{q1[0], q1[1]}, f32x2{q1[2], q1[3]}};
        const float kv = KLDS ? ks[a * VS + x] : kb[(long long)a * B * L + x];
#pragma unroll
        for (int f = 0; f < 4; ++f) {
          const f32x2 d = qp[f] - kv;
          acc[f] = __builtin_elementwise_fma(d, d, acc[f]);  // per element fmaf(d, d, acc): two frames an instruction
        }
      }
#pragma unroll
      for (int f = 0; f < AD_FPT; ++f) {
        const int y = ya + f;
        if (y <= yb && x <= y && x >= Lb + y - Tb) {
#pragma clang fp contract(off)
          float v = -temperature * acc[f >> 1][f & 1];
          if (prior) v = v + logf((float)pr[f] + 1e-8f);
          vals[(y - y0) * VS + x] = v;
        }
      }
    }
    __syncthreads();
    // 3. the search over the tile's frames
    for (int yy = 0; yy < ny; ++yy) {
      const int y = y0 + yy, x = tid;
      float* cur = rows + (y & 1) * VS;
      const float* prev = rows + ((y & 1) ^ 1) * VS;
      if (x >= max(0, Lb + y - Tb) && x < min(Lb, y + 1)) {
        const float v_cur = x == y ? MAX_NEG : own;
        const float v_prev = x == 0 ? (y == 0 ? 0.f : MAX_NEG) : prev[x - 1];
        own = vals[yy * VS + x] + fmaxf(v_prev, v_cur);
        cur[x] = own;
        dec[yy * VS + x] = (x != 0 && (x == y || v_cur < v_prev)) ? 1 : 0;
      }
      lds_barrier();
    }
    // the tile's decisions -> workspace rows (4 bytes a store; columns outside the band hold whatever the LDS held)
    {
      const int words = min(VS, Lp) >> 2;
      for (int i = tid; i < ny * words; i += AD_THREADS) {
        const int yy = i / words, w = i - yy * words;
        *reinterpret_cast<unsigned*>(wsb + (long long)(y0 + yy) * Lp + 4 * w) = *reinterpret_cast<const unsigned*>(dec + yy * VS + 4 * w);
      }
    }
  }
  __syncthreads();  // every decision is in the workspace and visible to this workgroup

  // read-back: chunks of whole rows through LDS (the vals region), walked by one thread
  unsigned char* chunk = smem;
  const int RC = TY * VS * 4 / Lp;  // rows of a chunk: at least 3 TY (Lp < L + 16 <= VS + 16)
  int index = Lb - 1, run = 0;
  for (int y1 = Tb; y1 > 0;) {
    const int nr = min(RC, y1), yc = y1 - nr;
    const uint4* src = reinterpret_cast<const uint4*>(wsb + (long long)yc * Lp);
    for (int i = tid; i < (nr * Lp) >> 4; i += AD_THREADS) reinterpret_cast<uint4*>(chunk)[i] = src[i];
    __syncthreads();
    if (tid == 0) {
      for (int y = y1 - 1; y >= yc; --y) {
        ++run;
        if (index != 0 && chunk[(y - yc) * Lp + index]) {
          drow[index] = run;
          run = 0;
          --index;
        }
      }
    }
    __syncthreads();
    y1 = yc;
  }
  if (tid == 0) drow[index] = run;
}

}  // namespace evmi

using namespace evmi;

extern "C" {

long long evmi_align_durations_ws_bytes(int B, int T, int L) {
  if (B <= 0 || T <= 0 || L <= 0) return 0;
  return (long long)B * T * ad_row_stride(L);
}

int evmi_align_durations_f32(const float* q_dev, const float* k_dev, const double* prior_dev, const int* text_lens_dev, const int* mel_lens_dev,
                             int* dur_dev, unsigned char* ws_dev, long long ws_bytes, int A, int B, int T, int L, float temperature,
                             void* stream) {
  if (!q_dev || !k_dev || !text_lens_dev || !mel_lens_dev || !dur_dev || !ws_dev) return fail(EVMI_ERR_INVALID_ARG, "align_durations: null pointer");
  if (A <= 0 || B <= 0 || T <= 0 || L <= 0) return fail(EVMI_ERR_INVALID_ARG, "align_durations: shape");
  if (A > AD_MAX_A) return fail(EVMI_ERR_UNSUPPORTED, "align_durations: more than 128 attention channels");
  if (L > AD_MAX_L) return fail(EVMI_ERR_UNSUPPORTED, "align_durations: more than 1024 tokens");
  if (ws_bytes < evmi_align_durations_ws_bytes(B, T, L)) return fail(EVMI_ERR_INVALID_ARG, "align_durations: workspace too small");
  if ((uintptr_t)ws_dev & 15) return fail(EVMI_ERR_INVALID_ARG, "align_durations: workspace not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  const AdPlan p = ad_plan(A, L);
  int rc;
#define EVMI_AD(KL)                                                                                                                 \
  rc = launch_with_lds(align_durations_kernel<KL>, dim3(B), dim3(AD_THREADS), p.bytes, s, q_dev, k_dev, prior_dev, text_lens_dev, \
                       mel_lens_dev, dur_dev, ws_dev, A, B, T, L, p.ty, p.vs, temperature)
  if (p.k_in_lds) EVMI_AD(true);
  else EVMI_AD(false);
#undef EVMI_AD
  if (rc) return rc;
  EVMI_LAUNCH_CHECK("align_durations");
  return EVMI_OK;
}

}  // extern "C"
