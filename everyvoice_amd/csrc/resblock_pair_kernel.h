// Fused residual pair of a HiFiGAN ResBlock1 on MFMA, persistent over row tiles:
//
//   out = post( [accumulate ? out : 0] + out_scale * ( x + b2 + conv2( lrelu( b1 + conv1_dil( lrelu(x) ) ) ) ) )
//
// Both convolutions (C -> C channels, KS taps; conv1 dilated, conv2 dense) run back to back on one
// row tile with the intermediate kept in LDS, so per pair the residual stream is read once and
// written once (the unfused path moves five tensors).  Only used where the per-tile working set
// fits LDS (C <= 64).
//
// Per tile of BN rows computed per convolution (TT = BN - (KS-1) of them valid after conv2):
//   XA [BN + (KS-1)*dil][C+8]  lrelu(x), zero outside [0, T)      (B operand of conv1)
//   RS [BN][C+8]               raw x of the output rows            (residual, no second HBM read)
//   T1 [BN + KS-1][C+8]        lrelu(conv1 + b1), zero outside [0, T)  (B operand of conv2)
//   WS 2 x [TAPS][C][C+8]      weight tap groups, streamed global -> regs -> LDS one group ahead
// The workgroup is persistent: it walks tiles tile0, tile0 + grid, ... and keeps the NEXT tile's
// activation rows in flight in registers while the current tile computes, so the only exposed
// HBM latency is the first tile's.  The blocks this kernel shares with the branch and chunked kernels are in resblock_tiles.h.
#pragma once

#include "resblock_tiles.h"

namespace evmi {

struct PairArgs {
  const bf16_t* x;   // [B][T][C] residual stream (raw)
  const bf16_t* w1;  // [KS][C][C] bf16, tap-major (kernel layout)
  const bf16_t* w2;
  const float* b1;
  const float* b2;
  bf16_t* out;       // [B][T][C]
  int T;
  int dil1;
  int tiles_per_item;
  int n_tiles;       // B * tiles_per_item
  float slope;       // leaky-relu slope on x (load) and on conv1's output
  float post_slope;
  float out_scale;
  int accumulate;
  long long* timeline;  // debug builds only (PairCfg::DBG): cycle stamps of workgroup 0, else nullptr
  // ragged batch: T stays the item stride and the upper bound, item b is valid for item_rows(lens, b, T) rows (common.h)
  ItemLens lens = {};
};

struct PairLaunch {
  void (*kernel)(PairArgs);
  void (*kernel_ragged)(PairArgs) = nullptr;  // the same kernel reading PairArgs::lens: an instantiation of its own, so the uniform one keeps its registers
  int c, ks, bn, tt, threads, max_dil;
  int wg_per_cu = 1;  // persistent workgroups per CU (LDS-bound residency)
  int kc;  // channel chunk of the weight layout [chunk][tap][C][kc] (== c when the layer is not chunked)
  size_t lds_bytes;
  const char* name;
};

// WRES_: the weights of both convolutions stay in registers for the life of the persistent workgroup (NSTEP x W_PER_THREAD vectors,
// loaded once) and are committed to the LDS from there: a two-tap step at 64 channels is 16 MFMAs per wave, shorter than the L2 round
// trip of the next step's weights that the one-step-ahead prefetch has to cover.
// WM_: waves along the output channels (the others along the rows): 64 channels on sixteen waves = 2 x 8 of 32 x 32 tiles
template <int C_, int KS_, int BN_, int TAPS_, int MAXDIL_, int WAVES_, int DBG_ = 0, int NWBUF_ = 2, int WRES_ = 0, int WM_ = 1>
struct PairCfg {
  static constexpr int C = C_, KS = KS_, BN = BN_, TAPS = TAPS_, MAXDIL = MAXDIL_, WAVES = WAVES_, DBG = DBG_, WRES = WRES_;
  static constexpr int WM = WM_, WN = WAVES / WM;
  // weight tap-group buffers in LDS: 2 = commit the next group while the current one is read; 1 = one
  // buffer (lets a whole convolution's taps sit in LDS at once) at the price of a barrier before each commit
  static constexpr int NWBUF = NWBUF_;
  static constexpr int NTHREADS = WAVES * 64;
  static constexpr int MT = C / (WM * 32), NT = BN / (WN * 32);
  static constexpr int S = C + 8;  // LDS row stride (elements): odd multiple of 16 B -> conflict-free b128 reads
  static constexpr int TT = BN - (KS - 1);
  static constexpr int RA_MAX = BN + (KS - 1) * MAXDIL;
  static constexpr int T1_ROWS = BN + KS - 1;
  static constexpr int NG = (KS + TAPS - 1) / TAPS;  // tap groups per convolution
  static constexpr int LAST_TAPS = KS - (NG - 1) * TAPS;  // taps in the final (possibly short) group
  static constexpr int NSTEP = 2 * NG;
  static constexpr int W_TILE = TAPS * C * S;
  static constexpr int W_VECS = TAPS * C * (C / 8);
  static constexpr int W_PER_THREAD = (W_VECS + NTHREADS - 1) / NTHREADS;
  static constexpr bool W_EXACT = (KS % TAPS == 0) && (W_VECS % NTHREADS == 0);
  static constexpr int X_VECS_MAX = RA_MAX * (C / 8);
  static constexpr int X_PER_THREAD = (X_VECS_MAX + NTHREADS - 1) / NTHREADS;
  static constexpr size_t OFF_XA = 0;
  static constexpr size_t OFF_RS = OFF_XA + size_t(RA_MAX) * S;
  static constexpr size_t OFF_T1 = OFF_RS + size_t(BN) * S;
  static constexpr size_t OFF_WS = OFF_T1 + size_t(T1_ROWS) * S;
  static constexpr size_t OFF_BIAS = OFF_WS + NWBUF * size_t(W_TILE);  // 2 copies x 2 x C floats (in bf16 units: 8 C)
  static constexpr size_t LDS = (OFF_BIAS + 8 * size_t(C)) * 2;
  static constexpr int WG_PER_CU = (2 * LDS <= 160 * 1024 && WAVES <= 4) ? 2 : 1;
  static_assert(BN % (WN * 32) == 0 && C % (WM * 32) == 0 && WAVES % WM == 0, "tiling");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

// RAGGED: item lengths from a.lens (item_rows); false: a.lens is not looked at and every item holds a.T rows
template <class P, bool RAGGED = false>
__global__ __launch_bounds__(P::NTHREADS) void resblock_pair_kernel(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* XA = reinterpret_cast<bf16_t*>(smem) + P::OFF_XA;
  bf16_t* RS = reinterpret_cast<bf16_t*>(smem) + P::OFF_RS;
  bf16_t* T1 = reinterpret_cast<bf16_t*>(smem) + P::OFF_T1;
  bf16_t* WS = reinterpret_cast<bf16_t*>(smem) + P::OFF_WS;
  float* BIAS = reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(smem) + P::OFF_BIAS);

  constexpr int C = P::C, KS = P::KS, H2 = (KS - 1) / 2;
  const Lane ln = lane_coords<P>();
  const int tid = ln.tid;
  const int h1 = a.dil1 * (KS - 1) / 2;
  // XA row 0 is global row r0 - H2 - h1; BN + (KS-1) * dil1 rows of XA are actually needed
  const XLoad xl = {a.x, a.lens, a.T, a.tiles_per_item, P::TT, H2 + h1, (P::BN + (KS - 1) * a.dil1) * (C / 8)};
  const bf16_t* const w[2] = {a.w1, a.w2};
  const TileWalk walk = tile_walk(a.n_tiles);

  u32x4 xreg[P::X_PER_THREAD];
  u32x4 wreg[P::WRES ? P::NSTEP : 1][P::W_PER_THREAD];

  int n_stamp = 0;
  auto stamp = [&]() {
    if (P::DBG && a.timeline && blockIdx.x == 0 && tid == 0 && n_stamp < 256)
      a.timeline[n_stamp++] = (long long)__builtin_readcyclecounter();
  };
  int tile = walk.first;
  if (tile >= walk.end) return;
  // both bias vectors sit in LDS, twice, for the life of the (persistent) workgroup (acc_from_bias)
  for (int i = tid; i < 4 * C; i += P::NTHREADS) BIAS[i] = (i % (2 * C)) < C ? a.b1[i % (2 * C)] : a.b2[i % (2 * C) - C];
  lds_barrier();  // (the first tile's accumulators are initialised from it before the first step's barrier)
  x_issue<P, RAGGED>(xreg, xl, tile, tid);
  w_preload<P>(wreg, w, tid);

  for (; tile < walk.end; tile += walk.stride) {
    const int item = tile / a.tiles_per_item, rt = tile % a.tiles_per_item;
    const int r0 = rt * P::TT;  // first output row of this tile
    const int next = tile + walk.stride < walk.end ? tile + walk.stride : -1;
    const int Tb = RAGGED ? item_rows(a.lens, item, a.T) : a.T;  // valid rows of this item (wave-uniform)
    if (RAGGED && r0 >= Tb) {  // this slot of the walk lies at or beyond its item's length: no load, no store
      if (next >= 0) x_issue<P, RAGGED>(xreg, xl, next, tid);
      continue;
    }
    stamp();  // tile start
    x_commit<P>(xreg, XA, RS, a.slope, xl.nvec, H2 + h1, P::BN, tid);  // RS: raw x of the output rows
    stamp();  // x committed

    f32x16 acc[P::MT][P::NT];
#pragma unroll
    for (int conv = 0; conv < 2; ++conv) {
      acc_from_bias<P>(acc, BIAS, conv, ln);
      // tap groups are fully unrolled so that the (possibly shorter) last group is static too
#pragma unroll
      for (int grp = 0; grp < P::NG; ++grp) {
        tap_group_step<P, RAGGED>(acc, wreg, xreg, WS, conv ? T1 : XA, 0, conv ? 1 : a.dil1, conv * P::NG + grp, w, xl, next, ln);
        stamp();  // step done
      }
      if (conv == 0) {  // T1[n] is global row r0 - H2 + n
        const bool edge = r0 - H2 < 0 || r0 - H2 + P::BN > Tb;  // (wave-uniform) rows outside the sequence in this tile
        t1_epilogue<P>(acc, T1, 0, r0 - H2, edge, Tb, a.slope, ln);
        zero_t1_tail<P, P::S>(T1, tid);
      }
    }
    stamp();  // conv loops done (includes the T1 epilogue of conv1)
    final_epilogue<P>(acc, RS, 0, a.out + (long long)item * a.T * C, r0, P::TT, Tb, a.out_scale, a.post_slope, a.accumulate, ln);
    stamp();  // stores issued
    lds_barrier();  // staging / residual tiles are free again for the next tile's commit
  }
}

template <class P>
static PairLaunch make_pair_launch(const char* name) {
  PairLaunch l;
  l.kernel = resblock_pair_kernel<P>;
  l.kernel_ragged = resblock_pair_kernel<P, true>;
  l.c = P::C;
  l.ks = P::KS;
  l.bn = P::BN;
  l.tt = P::TT;
  l.threads = P::NTHREADS;
  l.max_dil = P::MAXDIL;
  l.lds_bytes = P::LDS;
  l.name = name;
  l.kc = P::C;
  l.wg_per_cu = P::WG_PER_CU;
  return l;
}

const PairLaunch* find_resblock_pair(int c, int ks, int dil);
// w fp32 [c][c][ks] (torch: [out][in][tap]) -> the bf16 image [chunk][tap][c][kc] both pair kernels and the branch kernel stream
// (kc = PairLaunch::kc; kc == c: the plain tap-major [ks][c][c]).  Host memory on both sides; dst holds c * c * ks elements.
void relayout_resblock_pair(const float* w, int c, int ks, int kc, uint16_t* dst);
int launch_resblock_pair(const PairLaunch* L, PairArgs a, int B, int n_cu, hipStream_t stream);

}  // namespace evmi
