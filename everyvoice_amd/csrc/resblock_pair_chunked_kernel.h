// Fused residual pair for wide layers (C = 128): same contract as resblock_pair_kernel.h, but the
// conv1 operand tile holds one 64-channel chunk at a time (the whole-C tile does not fit next to the
// intermediate), the intermediate T1 holds all C channels, and the waves tile the output 2 (channels) x
// 4 (rows) with 64 x 64 per wave.  Per tile: 2*NCH*KS weight steps, one activation load per chunk, one
// epilogue — twice the K depth per tile of the unfused convolutions, and no T1 round trip through HBM.
// The tile walk, the LDS addressing (three pitches: SX / ST / SW) and the T1 tail rows come from resblock_tiles.h; the loads through
// buffer descriptors, the three-deep weight ring, the bias added in the epilogues and the staged stores are this kernel's own.
#pragma once

#include "resblock_pair_kernel.h"

namespace evmi {

template <int C_, int KC_, int KS_, int BN_, int MAXDIL_, int WM_, int WN_>
struct PairChunkedCfg {
  static constexpr int C = C_, KC = KC_, KS = KS_, BN = BN_, MAXDIL = MAXDIL_, WM = WM_, WN = WN_;
  static constexpr int NTHREADS = WM * WN * 64;
  static constexpr int NCH = C / KC;
  static constexpr int MT = C / (WM * 32), NT = BN / (WN * 32);
  static constexpr int SX = KC + 8, ST = C + 8, SW = KC + 8;
  static constexpr int TT = BN - (KS - 1);
  static constexpr int RA_MAX = BN + (KS - 1) * MAXDIL;
  static constexpr int T1_ROWS = BN + KS - 1;
  static constexpr int STEPS_PER_CONV = NCH * KS;
  static constexpr int NSTEP = 2 * STEPS_PER_CONV;
  static constexpr int W_TILE = C * SW;
  static constexpr int W_VECS = C * (KC / 8);
  static constexpr int W_PER_THREAD = W_VECS / NTHREADS;
  static constexpr int XV = (RA_MAX * (KC / 8) + NTHREADS - 1) / NTHREADS;
  static constexpr int RV = (BN * (C / 8)) / NTHREADS;  // epilogue vectors per thread (over all BN rows)
  static constexpr size_t OFF_XA = 0;
  static constexpr size_t OFF_T1 = OFF_XA + size_t(RA_MAX) * SX;
  static constexpr size_t OFF_WS = OFF_T1 + size_t(T1_ROWS) * ST;
  static constexpr size_t LDS = (OFF_WS + 2 * size_t(W_TILE)) * 2;
  static_assert(W_VECS % NTHREADS == 0 && (BN * (C / 8)) % NTHREADS == 0, "even split over the threads");
  static_assert(C % (WM * 32) == 0 && BN % (WN * 32) == 0 && C % KC == 0, "tiling");
  static_assert(LDS <= 160 * 1024, "LDS budget");
};

template <class P, bool RAGGED = false>  // RAGGED: as in resblock_pair_kernel
// (one workgroup per CU by its LDS: the register budget is the full 256 per wave at two waves per SIMD)
__global__ __launch_bounds__(P::NTHREADS) void resblock_pair_chunked_kernel(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16_t* XA = reinterpret_cast<bf16_t*>(smem) + P::OFF_XA;
  bf16_t* T1 = reinterpret_cast<bf16_t*>(smem) + P::OFF_T1;
  bf16_t* WS = reinterpret_cast<bf16_t*>(smem) + P::OFF_WS;
  bf16_t* OS = T1;  // epilogue staging [BN][ST] reuses the intermediate once conv2 has consumed it

  constexpr int C = P::C, KC = P::KC, KS = P::KS, H2 = (KS - 1) / 2;
  const Lane ln = lane_coords<P>();
  const int tid = ln.tid, lane = ln.lane;
  const int h1 = a.dil1 * (KS - 1) / 2;
  const int ra = P::BN + (KS - 1) * a.dil1;
  const int x_nvec = ra * (KC / 8);

  const TileWalk walk = tile_walk(a.n_tiles);
  int tile = walk.first;
  if (tile >= walk.end) return;

  bf16x8 xreg[P::XV];
  // weight images are requested TWO steps ahead (a ring of three register sets): a step is 16 MFMAs per wave, far shorter than the
  // L2 round trip that a one-step-ahead prefetch had to cover
  constexpr int WRING = 3;
  bf16x8 wreg[WRING][P::W_PER_THREAD];
  bf16x8 rreg[P::RV];

  auto x_issue = [&](int t, int chunk) {
    const int item = t / a.tiles_per_item, rt = t % a.tiles_per_item;
    const int g0 = rt * P::TT - H2 - h1;
    // the descriptor holds the item's own byte extent (ragged batch: item_rows); none at all for a tile at or beyond it, which is skipped
    const int Tb = RAGGED ? item_rows(a.lens, item, a.T) : a.T;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(a.x + (long long)item * a.T * C), 0,
                                                        (!RAGGED || rt * P::TT < Tb) ? Tb * C * 2 : 0, 0x00020000);
#pragma unroll
    for (int i = 0; i < P::XV; ++i) {
      const int v = tid + i * P::NTHREADS;
      const int row = v / (KC / 8), c8 = v % (KC / 8);
      const int g = g0 + row;
      // rows outside [0, T_item) fall outside the descriptor and read as zero (the convolution's zero padding)
      const unsigned voff = g < 0 ? 0xfffffff0u : (unsigned)((g * C + chunk * KC + c8 * 8) * 2);
      xreg[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff, 0, 0));
    }
  };
  auto x_commit = [&]() {
    const float sl = a.slope;
#pragma unroll
    for (int i = 0; i < P::XV; ++i) {
      const int v = tid + i * P::NTHREADS;
      if (v < x_nvec) {
        const int row = v / (KC / 8), c8 = v % (KC / 8);
        bf16x8 val = xreg[i];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const float f = (float)val[e];
          val[e] = (bf16_t)fmaxf(f, f * sl);
        }
        *reinterpret_cast<bf16x8*>(XA + lds_at<P::SX>(row, c8)) = val;
      }
    }
  };
  // step s: conv = s / STEPS_PER_CONV; within a conv: chunk-major, tap-minor.  Global layout per conv:
  // [chunk][tap][C][KC] (the conv_tc layout with BM = C)
  auto w_prefetch = [&](int s, int slot) {
    const int conv = s / P::STEPS_PER_CONV, rem = s % P::STEPS_PER_CONV;
    const bf16_t* src = (conv ? a.w2 : a.w1) + (long long)rem * C * KC;
#pragma unroll
    for (int i = 0; i < P::W_PER_THREAD; ++i)
      wreg[slot][i] = *reinterpret_cast<const bf16x8*>(src + (long long)(tid + i * P::NTHREADS) * 8);
  };
  auto w_commit = [&](int s, int slot) {
    bf16_t* dst = WS + (s & 1) * P::W_TILE;
#pragma unroll
    for (int i = 0; i < P::W_PER_THREAD; ++i) {
      const int v = tid + i * P::NTHREADS;
      *reinterpret_cast<bf16x8*>(dst + lds_at<P::SW>(v / (KC / 8), v % (KC / 8))) = wreg[slot][i];
    }
  };
  auto out_offset = [&](int r0, int Tb, int i) -> unsigned {
    const int v = tid + i * P::NTHREADS;
    const int n = v / (C / 8), c8 = v % (C / 8);
    const int r = r0 + n;
    return (n < P::TT && r < Tb) ? (unsigned)((r * C + c8 * 8) * 2) : 0xfffffff0u;
  };

  x_issue(tile, 0);
#pragma unroll
  for (int s = 0; s < WRING - 1; ++s) w_prefetch(s, s);
  static_assert(P::NSTEP % WRING == 0, "the ring position of a step is the same in every tile");

  for (; tile < walk.end; tile += walk.stride) {
    const int item = tile / a.tiles_per_item, rt = tile % a.tiles_per_item;
    const int r0 = rt * P::TT;
    const int next = tile + walk.stride < walk.end ? tile + walk.stride : tile;  // last tile: a harmless repeat
    const int Tb = RAGGED ? item_rows(a.lens, item, a.T) : a.T;  // valid rows of this item (wave-uniform)
    if (RAGGED && r0 >= Tb) {  // this slot of the walk lies at or beyond its item's length: no load, no store (the weight ring keeps its place)
      if (next != tile) x_issue(next, 0);
      continue;
    }

    f32x16 acc[P::MT][P::NT];
    auto zero_acc = [&]() {
#pragma unroll
      for (int i = 0; i < P::MT; ++i)
#pragma unroll
        for (int j = 0; j < P::NT; ++j)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    };

    // ---------------- conv1 (dilated) over the activated residual stream ----------------
    zero_acc();
    static_assert(KS % WRING == 0, "the ring slot of a step is its tap: static under the unrolled tap loop");
#pragma unroll 1
    for (int chunk = 0; chunk < P::NCH; ++chunk) {
      if (chunk > 0) lds_barrier();  // done reading the previous chunk's rows (chunk 0: barrier at the loop end)
      x_commit();
#pragma unroll
      for (int tap = 0; tap < KS; ++tap) {
        const int s = chunk * KS + tap;
        w_commit(s, tap % WRING);
        lds_barrier();
        w_prefetch((s + WRING - 1) % P::NSTEP, (tap + WRING - 1) % WRING);
        if (tap == 0) {
          if (chunk + 1 < P::NCH) x_issue(tile, chunk + 1);
          else x_issue(next, 0);
        }
        const bf16_t* Arow = WS + (s & 1) * P::W_TILE + frag_base<P::SW>(ln.cb, lane);
        const bf16_t* Brow = XA + frag_base<P::SX>(ln.nb + tap * a.dil1, lane);
        mma_tap_group<P::MT, P::NT, KC / 16, 1, 0, lds_at<P::SW>(32, 0), lds_at<P::SX>(32, 0)>(Arow, Brow, 0, acc);
      }
    }
    {  // T1[n][c] = lrelu(conv1 + b1) for global row r0 - H2 + n, zero outside the sequence
      const float sl = a.slope;
#pragma unroll
      for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int c = ln.cb + mt * 32 + 8 * q + 4 * (lane >> 5);
          const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b1 + c);
#pragma unroll
          for (int nt = 0; nt < P::NT; ++nt) {
            const int n = ln.nb + nt * 32 + (lane & 31);
            const int g = r0 - H2 + n;
            const float mask = (g >= 0 && g < Tb) ? 1.f : 0.f;
            bf16x4 pk;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              const float f = acc[mt][nt][4 * q + i] + bv[i];
              pk[i] = (bf16_t)(fmaxf(f, f * sl) * mask);
            }
            *reinterpret_cast<bf16x4*>(T1 + lds_at_channel<P::ST>(n, c)) = pk;
          }
        }
      zero_t1_tail<P, P::ST>(T1, tid);
    }
    // ---------------- conv2 (dense) over the intermediate in LDS ----------------
    zero_acc();
#pragma unroll 1
    for (int chunk = 0; chunk < P::NCH; ++chunk) {
#pragma unroll
      for (int tap = 0; tap < KS; ++tap) {
        const int s = P::STEPS_PER_CONV + chunk * KS + tap;
        w_commit(s, tap % WRING);
        lds_barrier();
        w_prefetch((s + WRING - 1) % P::NSTEP, (tap + WRING - 1) % WRING);  // (wraps to the next tile's first images)
        const bf16_t* Arow = WS + (s & 1) * P::W_TILE + frag_base<P::SW>(ln.cb, lane);
        const bf16_t* Brow = T1 + frag_base<P::ST>(ln.nb + tap, lane, chunk * (KC / 8));
        mma_tap_group<P::MT, P::NT, KC / 16, 1, 0, lds_at<P::SW>(32, 0), lds_at<P::ST>(32, 0)>(Arow, Brow, 0, acc);
      }
    }
    // ---------------- epilogue ----------------
    const auto xrsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16_t*>(a.x + (long long)item * a.T * C), 0,
                                                         Tb * C * 2, 0x00020000);
    const auto orsrc = __builtin_amdgcn_make_buffer_rsrc(a.out + (long long)item * a.T * C, 0, Tb * C * 2, 0x00020000);
#pragma unroll
    for (int i = 0; i < P::RV; ++i)  // residual rows (raw x): L2-resident, issued before the staging pass
      rreg[i] = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(xrsrc, out_offset(r0, Tb, i), 0, 0));
    lds_barrier();  // every wave is done reading T1: it becomes the staging tile
#pragma unroll
    for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = ln.cb + mt * 32 + 8 * q + 4 * (lane >> 5);
        const f32x4 bv = *reinterpret_cast<const f32x4*>(a.b2 + c);
#pragma unroll
        for (int nt = 0; nt < P::NT; ++nt) {
          const int n = ln.nb + nt * 32 + (lane & 31);
          bf16x4 pk;
#pragma unroll
          for (int i = 0; i < 4; ++i) pk[i] = (bf16_t)(acc[mt][nt][4 * q + i] + bv[i]);
          *reinterpret_cast<bf16x4*>(OS + lds_at_channel<P::ST>(n, c)) = pk;
        }
      }
    lds_barrier();
    {
      const float scale = a.out_scale, post = a.post_slope;
#pragma unroll
      for (int i = 0; i < P::RV; ++i) {
        const int v = tid + i * P::NTHREADS;
        const unsigned off = out_offset(r0, Tb, i);
        const bf16x8 o = *reinterpret_cast<const bf16x8*>(OS + lds_at<P::ST>(v / (C / 8), v % (C / 8)));
        float f[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) f[e] = ((float)o[e] + (float)rreg[i][e]) * scale;
        if (a.accumulate) {
          const bf16x8 pv = __builtin_bit_cast(bf16x8, __builtin_amdgcn_raw_buffer_load_b128(orsrc, off, 0, 0));
#pragma unroll
          for (int e = 0; e < 8; ++e) f[e] += (float)pv[e];
        }
        bf16x8 res;
#pragma unroll
        for (int e = 0; e < 8; ++e) res[e] = (bf16_t)fmaxf(f[e], f[e] * post);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, res), orsrc, off, 0, 0);
      }
    }
    lds_barrier();  // staging consumed: the next tile may overwrite T1 / XA
  }
}

template <class P>
static PairLaunch make_pair_chunked_launch(const char* name) {
  PairLaunch l;
  l.kernel = resblock_pair_chunked_kernel<P>;
  l.kernel_ragged = resblock_pair_chunked_kernel<P, true>;
  l.c = P::C;
  l.ks = P::KS;
  l.bn = P::BN;
  l.tt = P::TT;
  l.threads = P::NTHREADS;
  l.max_dil = P::MAXDIL;
  l.lds_bytes = P::LDS;
  l.name = name;
  l.kc = P::KC;
  return l;
}

}  // namespace evmi
