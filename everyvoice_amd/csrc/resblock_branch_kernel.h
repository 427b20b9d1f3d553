// One whole branch of a HiFiGAN multi-receptive-field stage -- up to three residual pairs of ResBlock1, dilations (d0, d1, d2) -- on
// one row tile, the running value of the branch kept in LDS between the pairs:
//
//   y0 = x;   y(p+1) = y(p) + b2p + conv2p( lrelu( b1p + conv1p_dil(dp)( lrelu(y(p)) ) ) );   out = post([out +] scale * y(np))
//
// The pair kernel (resblock_pair_kernel.h) reads and writes the residual stream once per pair: three round trips of a 403 MB tensor per
// branch, and the k = 3 / k = 7 pairs of the 32- and 64-channel stages are bound by exactly that (0.8 GB in 216 us).  Here HBM sees the
// branch input once and the branch output once.  Arithmetic and rounding points are those of the pair kernel (y(p) is rounded to bf16
// where the pair kernel stores it): the two paths give the same bits.
//
// Geometry.  All LDS tiles share ONE row coordinate: LDS row i is global row g0 + i.  H = (KS-1)/2, h1p = dp * H, M0 = 0,
// M(p+1) = Mp + h1p + H, Mtot = M(np).  The tile loads R0 = BN + 2 h1_0 rows of x from g0 = r0 - Mtot; every convolution computes BN rows:
//   conv1 of pair p: rows Mp + h1p + n  (n < BN)  <-  XA rows Mp + n + j dp
//   conv2 of pair p: rows M(p+1) + n              <-  T1 rows Mp + h1p + n + j
// and what lies outside the shrinking valid range [M(p+1), R0 - M(p+1)) is finite garbage that only ever feeds garbage rows (a row of the
// B operand touches one output row).  TT = R0 - 2 Mtot rows are stored per tile (dilations 1, 3, 5: BN - 22 H).  Rows outside the
// sequence are forced to zero at every stage (each convolution of the unfused chain zero-pads ITS input).
//   XA [RB][C+8]  lrelu(y(p))      RS [RB][C+8]  y(p) (the residual; updated in place)      T1 [RB][C+8]  lrelu(conv1 + b1)
//   RB = BN + 16 H rows (the reach of pair 2 of a (1, 3, 5) branch); WS / BIAS as in the pair kernel.
// Every block but the update of y between two pairs is the pair kernel's own, from resblock_tiles.h.
#pragma once

#include "resblock_pair_kernel.h"

namespace evmi {

struct BranchArgs {
  const bf16_t* x;    // [B][T][C]
  bf16_t* out;        // [B][T][C]
  const bf16_t* w[6];  // conv1, conv2 of pair 0, 1, 2: [KS][C][C] bf16, tap-major (the pair kernel's layout)
  const float* b[6];
  int T;
  int np;             // pairs (1..3)
  int dil[3];
  int tt;             // valid rows per tile (host: BN + 2 h1_0 - 2 Mtot)
  int tiles_per_item;
  int n_tiles;
  float slope, post_slope, out_scale;
  int accumulate;
  ItemLens lens = {};  // ragged batch: as PairArgs::lens
};

struct BranchLaunch {
  void (*kernel)(BranchArgs);
  void (*kernel_ragged)(BranchArgs) = nullptr;  // as PairLaunch::kernel_ragged
  int c, ks, bn, rb, threads;
  size_t lds_bytes;
  const char* name;
};

// WRES_: the weights of all 2 NP convolutions stay in registers for the life of the persistent workgroup (loaded once) and are committed to
// the LDS from there every step -- a k = 3 step is 12 MFMAs per wave, far shorter than the L2 round trip of the next step's weights that
// the pair kernel's one-step-ahead prefetch has to cover
// WM_: waves along the output channels (the others along the rows)
template <int C_, int KS_, int BN_, int TAPS_, int WAVES_, int NWBUF_, int NP_ = 3, int WRES_ = 1, int WM_ = 1>
struct BranchCfg {
  static constexpr int C = C_, KS = KS_, BN = BN_, TAPS = TAPS_, WAVES = WAVES_, NWBUF = NWBUF_, NP = NP_, WRES = WRES_;
  static constexpr int WM = WM_, WN = WAVES / WM;
  static constexpr int NTHREADS = WAVES * 64;
  static constexpr int MT = C / (WM * 32), NT = BN / (WN * 32);
  static constexpr int S = C + 8;
  static constexpr int H = (KS - 1) / 2;
  static constexpr int RB = BN + 16 * H;
  static constexpr int NG = (KS + TAPS - 1) / TAPS;
  static constexpr int LAST_TAPS = KS - (NG - 1) * TAPS;
  static constexpr int NSTEP = 2 * NP * NG;  // weight steps per tile: convolution s / NG (conv1, conv2 of pair 0, conv1 of pair 1, ...)
  static constexpr int W_TILE = TAPS * C * S;
  static constexpr int W_VECS = TAPS * C * (C / 8);
  static constexpr int W_PER_THREAD = (W_VECS + NTHREADS - 1) / NTHREADS;
  static constexpr bool W_EXACT = (KS % TAPS == 0) && (W_VECS % NTHREADS == 0);
  static constexpr int X_PER_THREAD = (RB * (C / 8) + NTHREADS - 1) / NTHREADS;
  static constexpr size_t OFF_XA = 0;
  static constexpr size_t OFF_RS = OFF_XA + size_t(RB) * S;
  static constexpr size_t OFF_T1 = OFF_RS + size_t(RB) * S;
  static constexpr size_t OFF_WS = OFF_T1 + size_t(RB) * S;
  static constexpr size_t OFF_BIAS = OFF_WS + NWBUF * size_t(W_TILE);  // 2 copies x 6 x C floats (in bf16 units: 24 C)
  static constexpr size_t LDS = (OFF_BIAS + 24 * size_t(C)) * 2;
  static_assert(BN % (WN * 32) == 0 && C % (WM * 32) == 0 && WAVES % WM == 0, "tiling");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

template <class P, bool RAGGED = false>  // RAGGED: as in resblock_pair_kernel
__global__ __launch_bounds__(P::NTHREADS) void resblock_branch_kernel(BranchArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* XA = reinterpret_cast<bf16_t*>(smem) + P::OFF_XA;
  bf16_t* RS = reinterpret_cast<bf16_t*>(smem) + P::OFF_RS;
  bf16_t* T1 = reinterpret_cast<bf16_t*>(smem) + P::OFF_T1;
  bf16_t* WS = reinterpret_cast<bf16_t*>(smem) + P::OFF_WS;
  float* BIAS = reinterpret_cast<float*>(reinterpret_cast<bf16_t*>(smem) + P::OFF_BIAS);

  constexpr int C = P::C, S = P::S, H = P::H;
  const Lane ln = lane_coords<P>();
  const int tid = ln.tid, lane = ln.lane;
  constexpr int np = P::NP;
  int mtot = 0;
#pragma unroll
  for (int p = 0; p < np; ++p) mtot += a.dil[p] * H + H;
  // LDS row 0 is global row r0 - Mtot; a tile loads BN + 2 h1_0 rows of x
  const XLoad xl = {a.x, a.lens, a.T, a.tiles_per_item, a.tt, mtot, (P::BN + 2 * a.dil[0] * H) * (C / 8)};
  const TileWalk walk = tile_walk(a.n_tiles);

  u32x4 xreg[P::X_PER_THREAD];
  u32x4 wreg[P::WRES ? P::NSTEP : 1][P::W_PER_THREAD];

  int tile = walk.first;
  if (tile >= walk.end) return;
  // the three activation tiles start finite (what a tile never writes is read by garbage rows only, but must not be a NaN pattern
  // that another row's MFMA could not survive -- it cannot: a B row feeds one output row -- nor trap the activation arithmetic).
  // One flat fill of XA, RS and T1, pad columns included: whatever the layout inside a tile, every byte of the three is written
  for (int v = tid; v < 3 * P::RB * S / 8; v += P::NTHREADS) *reinterpret_cast<bf16x8*>(XA + v * 8) = zero_bf16x8();
  for (int i = tid; i < 4 * np * C; i += P::NTHREADS) BIAS[i] = a.b[(i % (2 * np * C)) / C][i % C];  // (two copies: acc_from_bias)
  lds_barrier();
  x_issue<P, RAGGED>(xreg, xl, tile, tid);
  w_preload<P>(wreg, a.w, tid);

  for (; tile < walk.end; tile += walk.stride) {
    const int item = tile / a.tiles_per_item, rt = tile % a.tiles_per_item;
    const int r0 = rt * a.tt;       // first output row of this tile
    const int g0 = r0 - mtot;       // global row of LDS row 0
    const int next = tile + walk.stride < walk.end ? tile + walk.stride : -1;
    const int Tb = RAGGED ? item_rows(a.lens, item, a.T) : a.T;  // valid rows of this item (wave-uniform)
    if (RAGGED && r0 >= Tb) {  // this slot of the walk lies at or beyond its item's length: no load, no store
      if (next >= 0) x_issue<P, RAGGED>(xreg, xl, next, tid);
      continue;
    }
    const bool edge = g0 < 0 || g0 + P::RB > Tb;  // (wave-uniform) the tile holds rows outside the sequence
    x_commit<P>(xreg, XA, RS, a.slope, xl.nvec, 0, P::RB, tid);  // RS: every row, y(0) = x

    f32x16 acc[P::MT][P::NT];
    int mp = 0;  // Mp
#pragma unroll
    for (int p = 0; p < np; ++p) {
      const int dil = a.dil[p];
      const int h1 = dil * H;
#pragma unroll
      for (int conv = 0; conv < 2; ++conv) {
        acc_from_bias<P>(acc, BIAS, 2 * p + conv, ln);
        // conv1: XA rows Mp + n + j d;  conv2: T1 rows Mp + h1 + n + j
#pragma unroll
        for (int grp = 0; grp < P::NG; ++grp)
          tap_group_step<P, RAGGED>(acc, wreg, xreg, WS, conv ? T1 : XA, conv ? mp + h1 : mp, conv ? 1 : dil, (2 * p + conv) * P::NG + grp, a.w, xl,
                                    next, ln);
        // T1[Mp + h1 + n] (only a tile at an end of the sequence has rows outside it)
        if (conv == 0) t1_epilogue<P>(acc, T1, mp + h1, g0, edge, Tb, a.slope, ln);
      }
      const int mnext = mp + h1 + H;  // M(p+1): LDS row of conv2's output row 0
      if (p + 1 < np) {
        // y(p+1) = y(p) + b2 + conv2, rounded to bf16 as the pair kernel stores it; raw into RS (in place: a lane reads and writes
        // its own elements), its activation into XA (dead since conv1 of this pair); zero outside the sequence
        const float sl = a.slope;
#pragma unroll
        for (int mt = 0; mt < P::MT; ++mt) {
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const int c = ln.cb + mt * 32 + 8 * q + 4 * (lane >> 5);
#pragma unroll
            for (int nt = 0; nt < P::NT; ++nt) {
              const int n = ln.nb + nt * 32 + (lane & 31);
              const int row = mnext + n;
              const bf16x4 rv = *reinterpret_cast<const bf16x4*>(RS + lds_at_channel<S>(row, c));
              bf16x4 raw, act;
#pragma unroll
              for (int i = 0; i < 4; ++i) raw[i] = (bf16_t)(acc[mt][nt][4 * q + i] + (float)rv[i]);
              if (edge) {
                const int g = g0 + row;
                if (g < 0 || g >= Tb) {
#pragma unroll
                  for (int i = 0; i < 4; ++i) raw[i] = (bf16_t)0.f;
                }
              }
              act = lrelu4_bf16(f32x4{(float)raw[0], (float)raw[1], (float)raw[2], (float)raw[3]}, sl);
              *reinterpret_cast<bf16x4*>(RS + lds_at_channel<S>(row, c)) = raw;
              *reinterpret_cast<bf16x4*>(XA + lds_at_channel<S>(row, c)) = act;
            }
          }
        }
      } else {
        final_epilogue<P>(acc, RS, mnext, a.out + (long long)item * a.T * C, r0, a.tt, Tb, a.out_scale, a.post_slope, a.accumulate, ln);
      }
      mp = mnext;
    }
    lds_barrier();  // the activation tiles are free again for the next tile's commit
  }
}

template <class P>
static BranchLaunch make_branch_launch(const char* name) {
  BranchLaunch l;
  l.kernel = resblock_branch_kernel<P>;
  l.kernel_ragged = resblock_branch_kernel<P, true>;
  l.c = P::C;
  l.ks = P::KS;
  l.bn = P::BN;
  l.rb = P::RB;
  l.threads = P::NTHREADS;
  l.lds_bytes = P::LDS;
  l.name = name;
  return l;
}

// nullptr when no instantiation takes this branch (channels, kernel size, the dilations' reach inside the LDS tiles)
const BranchLaunch* find_resblock_branch(int c, int ks, int np, const int* dil);
int launch_resblock_branch(const BranchLaunch* L, BranchArgs a, int B, int n_cu, hipStream_t stream);

}  // namespace evmi
