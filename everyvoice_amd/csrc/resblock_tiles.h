// Device-side toolkit of the fused residual kernels (resblock_pair_kernel.h, resblock_pair_chunked_kernel.h, resblock_branch_kernel.h):
// the persistent tile walk, the LDS tile addressing, and the blocks the pair and branch kernels run in the same form -- activation
// load / commit, weight streaming, accumulator initialisation, the weight step, the T1 epilogue and the final epilogue.  Plain
// function templates on the kernel's config type P; every one is inlined into its caller.  The three kernels must keep identical
// bits (the branch is three chained pairs): a change of the LDS layout or of the arithmetic is made here, once.
//
// Two conventions here are for the register allocator (DESIGN.md §31 has the figures), not for taste (a third, the two bodies of the
// final epilogue, is explained there):
//  * the small structs (Lane, XLoad) are passed BY VALUE.  By reference the compiler keeps them as memory objects until after its
//    early inlining, and the kernels that run at their register cap then spill (the 32-channel branch kernels: 36 bytes of scratch);
//  * the register arrays that cross a tile (activation rows, resident weights) are four-dword vectors, not bf16x8.  Their loops are
//    still rolled when these functions are inlined, the compiler then turns such an array into ONE long vector, and of 16-bit
//    elements that costs a v_perm_b32 per dword on the way out (40 per tile in the pair kernels).
#pragma once

#include "common.h"

namespace evmi {

// ---- tile walk -----------------------------------------------------------------------------------------------------------------------
// XCD-aware: workgroup b runs on XCD b % 8; each XCD gets one contiguous range of tiles so that neighbouring tiles (which share halo
// rows) meet in the same L2.  A workgroup runs tiles first, first + stride, ... below end (the grid is a multiple of 8).
struct TileWalk {
  int first, end, stride;
};
__device__ __forceinline__ TileWalk tile_walk(int n_tiles) {
  const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per_xcd_wg = ((int)gridDim.x + 7) >> 3;
  const int tiles_per_xcd = (n_tiles + 7) >> 3;
  const int tile_lo = xcd * tiles_per_xcd;
  return {tile_lo + slot, min(n_tiles, tile_lo + tiles_per_xcd), per_xcd_wg};
}

// ---- LDS addressing ------------------------------------------------------------------------------------------------------------------
// Where channel octet c8 (channels 8 c8 .. 8 c8 + 7) of row `row` lives in an activation or weight tile of pitch S elements
// (S = channels + 8: an odd multiple of 16 B, conflict-free b128 reads).  Every LDS access of the three kernels goes through here.
template <int S>
__host__ __device__ __forceinline__ constexpr int lds_at(int row, int c8) {
  return row * S + c8 * 8;
}
// the same for the accumulator layout's channel quads (c a multiple of 4)
template <int S>
__host__ __device__ __forceinline__ constexpr int lds_at_channel(int row, int c) {
  return lds_at<S>(row, c >> 3) + (c & 7);
}
// a lane's fragment base for mma_tap_group (common.h): lane (n, h) reads octet c8_0 + h (+ 2 per k-step) of row row0 + n -- of the
// weight tile (A: rows are output channels) and of the activation tile (B: rows are sequence rows) alike
template <int S>
__device__ __forceinline__ int frag_base(int row0, int lane, int c8_0 = 0) {
  return lds_at<S>(row0 + (lane & 31), c8_0 + (lane >> 5));
}

// this thread's place: cb = first output channel of its wave, nb = first row of its wave within the BN rows of a convolution
struct Lane {
  int tid, lane, cb, nb;
};
template <class P>
__device__ __forceinline__ Lane lane_coords() {
  const int tid = threadIdx.x, wave = tid >> 6;
  return {tid, tid & 63, (wave / P::WN) * P::MT * 32, (wave % P::WN) * P::NT * 32};
}

__device__ __forceinline__ bf16x8 zero_bf16x8() {
  bf16x8 z;
#pragma unroll
  for (int e = 0; e < 8; ++e) z[e] = (bf16_t)0.f;
  return z;
}

// rows BN .. BN + KS - 2 of T1 (pitch S, all P::C channels) only feed discarded outputs; keep them finite
template <class P, int S>
__device__ __forceinline__ void zero_t1_tail(bf16_t* T1, int tid) {
  constexpr int C8 = P::C / 8;
  for (int v = tid; v < (P::KS - 1) * C8; v += P::NTHREADS) *reinterpret_cast<bf16x8*>(T1 + lds_at<S>(P::BN + v / C8, v % C8)) = zero_bf16x8();
}

// ---- activation load and commit (pair, branch) ---------------------------------------------------------------------------------------
// Where a tile's rows come from: LDS row 0 of tile (item, rt) is global row rt * tt - halo of the item; nvec 16-byte vectors are needed.
struct XLoad {
  const bf16_t* x;  // [B][T][C]
  ItemLens lens;    // looked at by the RAGGED instantiations only
  int T, tiles_per_item, tt, halo, nvec;
};
// global -> registers; rows outside [0, T_item) are not requested and commit as zero (each convolution's zero padding)
template <class P, bool RAGGED>
__device__ __forceinline__ void x_issue(u32x4 (&xreg)[P::X_PER_THREAD], const XLoad xl, int tile, int tid) {
  constexpr int C = P::C;
  const int item = tile / xl.tiles_per_item, rt = tile % xl.tiles_per_item;
  const int g0 = rt * xl.tt - xl.halo;
  const bf16_t* xb = xl.x + (long long)item * xl.T * C;
  const int Tb = RAGGED ? item_rows(xl.lens, item, xl.T) : xl.T;
  if (RAGGED && rt * xl.tt >= Tb) return;  // a tile at or beyond its item's length is skipped: nothing to load
#pragma unroll
  for (int i = 0; i < P::X_PER_THREAD; ++i) {
    const int v = tid + i * P::NTHREADS;
    const int row = v / (C / 8), c8 = v % (C / 8);
    const int g = g0 + row;
    bf16x8 val = zero_bf16x8();
    if (v < xl.nvec && g >= 0 && g < Tb) val = *reinterpret_cast<const bf16x8*>(xb + (long long)g * C + c8 * 8);
    xreg[i] = __builtin_bit_cast(u32x4, val);
  }
}
// registers -> LDS: lrelu(x) into XA; the raw rows rs_row0 .. rs_row0 + rs_rows - 1 also into RS (rows 0 ..), the residual
template <class P>
__device__ __forceinline__ void x_commit(const u32x4 (&xreg)[P::X_PER_THREAD], bf16_t* XA, bf16_t* RS, float slope, int nvec, int rs_row0,
                                         int rs_rows, int tid) {
  constexpr int C = P::C, S = P::S;
#pragma unroll
  for (int i = 0; i < P::X_PER_THREAD; ++i) {
    const int v = tid + i * P::NTHREADS;
    if (v < nvec) {
      const int row = v / (C / 8), c8 = v % (C / 8);
      const bf16x8 raw = __builtin_bit_cast(bf16x8, xreg[i]);
      const bf16x8 act = lrelu8_bf16(raw, slope);
      *reinterpret_cast<bf16x8*>(XA + lds_at<S>(row, c8)) = act;
      const int n = row - rs_row0;
      if (n >= 0 && n < rs_rows) *reinterpret_cast<bf16x8*>(RS + lds_at<S>(n, c8)) = raw;
    }
  }
}

// ---- weight streaming (pair, branch) -------------------------------------------------------------------------------------------------
// Step s in [0, P::NSTEP): convolution s / NG, tap group s % NG.  w_conv: that convolution's image [KS][C][C], tap-major.
template <class P>
__device__ __forceinline__ constexpr int w_group_vecs(int grp) {
  return ((P::KS - grp * P::TAPS) < P::TAPS ? (P::KS - grp * P::TAPS) : P::TAPS) * P::C * (P::C / 8);
}
template <class P>
__device__ __forceinline__ void w_prefetch(u32x4 (&wr)[P::W_PER_THREAD], const bf16_t* w_conv, int grp, int tid) {
  const bf16_t* src = w_conv + (long long)grp * P::TAPS * P::C * P::C;
#pragma unroll
  for (int i = 0; i < P::W_PER_THREAD; ++i) {
    const int v = tid + i * P::NTHREADS;
    if (P::W_EXACT || v < w_group_vecs<P>(grp)) wr[i] = *reinterpret_cast<const u32x4*>(src + (long long)v * 8);
  }
}
template <class P>
__device__ __forceinline__ void w_commit(const u32x4 (&wr)[P::W_PER_THREAD], bf16_t* WS, int s, int tid) {
  bf16_t* dst = WS + (s & (P::NWBUF - 1)) * P::W_TILE;
#pragma unroll
  for (int i = 0; i < P::W_PER_THREAD; ++i) {
    const int v = tid + i * P::NTHREADS;
    if (P::W_EXACT || v < w_group_vecs<P>(s % P::NG)) *reinterpret_cast<u32x4*>(dst + lds_at<P::S>(v / (P::C / 8), v % (P::C / 8))) = wr[i];
  }
}
// before the first tile: every step's weights where they stay in registers (P::WRES), else step 0's.  w: the P::NSTEP / NG weight images
template <class P>
__device__ __forceinline__ void w_preload(u32x4 (&wreg)[P::WRES ? P::NSTEP : 1][P::W_PER_THREAD], const bf16_t* const* w, int tid) {
#pragma unroll
  for (int s = 0; s < (P::WRES ? P::NSTEP : 1); ++s) w_prefetch<P>(wreg[s], w[s / P::NG], s % P::NG, tid);
}

// ---- accumulators start at the bias (pair, branch) -----------------------------------------------------------------------------------
// BIAS holds two copies of the P::NSTEP / NG bias vectors, read in the accumulator layout (channels 8q + 4h .. + 3 per register quad)
// under the first weight commit of the convolution: the epilogues, VALU-bound at these channel counts, only activate / add the
// residual.  (Two copies: the accumulators of the second row tile are initialised by loads of their own -- from one copy the compiler
// shares the loads and pays a v_mov per accumulator register.)
template <class P>
__device__ __forceinline__ void acc_from_bias(f32x16 (&acc)[P::MT][P::NT], const float* BIAS, int conv, const Lane ln) {
  const float* bias = BIAS + conv * P::C;
#pragma unroll
  for (int i = 0; i < P::MT; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int j = 0; j < P::NT; ++j) {
        const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + (j & 1) * (P::NSTEP / P::NG) * P::C + ln.cb + i * 32 + 8 * q + 4 * (ln.lane >> 5));
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[i][j][4 * q + r] = bv[r];
      }
}

// ---- one weight step (pair, branch) --------------------------------------------------------------------------------------------------
// Commits step s's weights, requests the next step's (w: the P::NSTEP / NG weight images; wraps to the next tile's first group) and,
// in step 0, the next tile's rows (next_tile < 0: none) -- after the weight loads, so those stay in flight -- then runs the step's
// taps: output row n of the convolution reads rows b_row0 + n + j * dil of the activation tile B.
template <class P, bool RAGGED>
__device__ __forceinline__ void tap_group_step(f32x16 (&acc)[P::MT][P::NT], u32x4 (&wreg)[P::WRES ? P::NSTEP : 1][P::W_PER_THREAD],
                                               u32x4 (&xreg)[P::X_PER_THREAD], bf16_t* WS, const bf16_t* B, int b_row0, int dil, int s,
                                               const bf16_t* const* w, const XLoad xl, int next_tile, const Lane ln) {
  constexpr int S = P::S;
  const int grp = s % P::NG;
  if (P::NWBUF == 1 && s > 0) lds_barrier();  // everyone is done reading the single weight buffer (s = 0: the barrier that ends a tile)
  w_commit<P>(wreg[P::WRES ? s : 0], WS, s, ln.tid);
  lds_barrier();
  if (!P::WRES) {
    const int sn = s + 1 == P::NSTEP ? 0 : s + 1;
    w_prefetch<P>(wreg[0], w[sn / P::NG], sn % P::NG, ln.tid);
  }
  if (s == 0 && next_tile >= 0) x_issue<P, RAGGED>(xreg, xl, next_tile, ln.tid);
  const bf16_t* Arow = WS + (s & (P::NWBUF - 1)) * P::W_TILE + frag_base<S>(ln.cb, ln.lane);
  // (the wave-uniform row offset apart from the lane's own, which does not change from step to step)
  const bf16_t* Brow = B + lds_at<S>(b_row0 + grp * P::TAPS * dil, 0) + frag_base<S>(ln.nb, ln.lane);
  // (the possibly shorter last group is static too: the callers unroll their step loops)
  if (grp + 1 < P::NG || P::LAST_TAPS == P::TAPS)
    mma_tap_group<P::MT, P::NT, P::C / 16, P::TAPS, lds_at<S>(P::C, 0), lds_at<S>(32, 0), lds_at<S>(32, 0)>(Arow, Brow, lds_at<S>(dil, 0), acc);
  else
    mma_tap_group<P::MT, P::NT, P::C / 16, P::LAST_TAPS, lds_at<S>(P::C, 0), lds_at<S>(32, 0), lds_at<S>(32, 0)>(Arow, Brow, lds_at<S>(dil, 0), acc);
}

// ---- T1 epilogue (pair, branch) ------------------------------------------------------------------------------------------------------
// T1[t_row0 + n] = lrelu(conv1 + b1) (the bias is in the accumulators), zero where global row g0 + t_row0 + n lies outside [0, Tb);
// edge (wave-uniform): this tile holds such rows at all
template <class P>
__device__ __forceinline__ void t1_epilogue(const f32x16 (&acc)[P::MT][P::NT], bf16_t* T1, int t_row0, int g0, bool edge, int Tb, float slope,
                                            const Lane ln) {
#pragma unroll
  for (int mt = 0; mt < P::MT; ++mt) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = ln.cb + mt * 32 + 8 * q + 4 * (ln.lane >> 5);
#pragma unroll
      for (int nt = 0; nt < P::NT; ++nt) {
        const int n = ln.nb + nt * 32 + (ln.lane & 31);
        const int row = t_row0 + n;
        bf16x4 pk = lrelu4_bf16(f32x4{acc[mt][nt][4 * q], acc[mt][nt][4 * q + 1], acc[mt][nt][4 * q + 2], acc[mt][nt][4 * q + 3]}, slope);
        if (edge) {
          const int g = g0 + row;
          if (g < 0 || g >= Tb) {
#pragma unroll
            for (int i = 0; i < 4; ++i) pk[i] = (bf16_t)0.f;
          }
        }
        *reinterpret_cast<bf16x4*>(T1 + lds_at_channel<P::S>(row, c)) = pk;
      }
    }
  }
}

// ---- final epilogue (pair, branch) ---------------------------------------------------------------------------------------------------
// out = post([out +] scale * (conv2 + b2 + residual)): accumulators + RS rows rs_row0 + n (accumulator layout) -> registers -> 16-byte
// stores of rows r0 + n, n < tt, below Tb.  No staging pass and no barrier: every wave retires its rows on its own.  Lane (n, h)
// holds channels 8q + 4h .. + 3 of row n per register quad q; swap_quads_bf16 turns the packed quads (2p, 2p + 1) into 16
// contiguous bytes per lane.  ob: the item's [T][C] output.
// ACC (accumulate) is a template argument of the body and the run-time flag picks the instantiation: with the flag tested twice in
// one body (request the old values, later add them) the compiler cannot see that the second test follows the first, holds the
// requested registers pending on the path that skips their use, and drains the next tile's activation loads (s_waitcnt vmcnt(0))
// as soon as the allocator reuses one of them there -- which costs the pair kernels up to 14 %.
template <class P, bool ACC>
__device__ __forceinline__ void final_epilogue_rows(const f32x16 (&acc)[P::MT][P::NT], const bf16_t* RS, int rs_row0, bf16_t* ob, int r0, int tt,
                                                    int Tb, float scale, float post, const Lane ln) {
  // the scaled sum is rounded BEFORE the old value is added (one of the kernels' rounding points): no fused multiply-add here
#pragma clang fp contract(off)
  constexpr int C = P::C;
  constexpr bool accumulate = ACC;
  const int cb = ln.cb, hh = ln.lane >> 5;
#pragma unroll
  for (int nt = 0; nt < P::NT; ++nt) {
    const int n = ln.nb + nt * 32 + (ln.lane & 31);
    const int r = r0 + n;
    const bool ok = n < tt && r < Tb;
    bf16_t* dst = ob + (long long)(ok ? r : 0) * C + 8 * hh;
    u32x4 pv[P::MT][2];
    if (accumulate) {  // all of the lane's vectors are requested before the first is consumed
#pragma unroll
      for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
        for (int p2 = 0; p2 < 2; ++p2) pv[mt][p2] = *reinterpret_cast<const u32x4*>(dst + cb + mt * 32 + 16 * p2);
    }
#pragma unroll
    for (int mt = 0; mt < P::MT; ++mt)
#pragma unroll
      for (int p2 = 0; p2 < 2; ++p2) {
        float f[8];
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
          const int c = cb + mt * 32 + 8 * (2 * p2 + qq) + 4 * hh;
          const bf16x4 rv = *reinterpret_cast<const bf16x4*>(RS + lds_at_channel<P::S>(rs_row0 + n, c));
#pragma unroll
          for (int i = 0; i < 4; ++i) f[4 * qq + i] = (acc[mt][nt][4 * (2 * p2 + qq) + i] + (float)rv[i]) * scale;
        }
        if (accumulate) {
          const u32x4 d = swap_quads_bf16(pv[mt][p2]);
#pragma unroll
          for (int w = 0; w < 4; ++w) {
            f[2 * w] += bf16_lo(d[w]);
            f[2 * w + 1] += bf16_hi(d[w]);
          }
        }
        u32x4 o;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
          const float lo = post != 1.f ? fmaxf(f[2 * w], f[2 * w] * post) : f[2 * w];
          const float hi = post != 1.f ? fmaxf(f[2 * w + 1], f[2 * w + 1] * post) : f[2 * w + 1];
          o[w] = pack_bf16x2(lo, hi);
        }
        o = swap_quads_bf16(o);
        if (ok) *reinterpret_cast<u32x4*>(dst + cb + mt * 32 + 16 * p2) = o;
      }
  }
}
template <class P>
__device__ __forceinline__ void final_epilogue(const f32x16 (&acc)[P::MT][P::NT], const bf16_t* RS, int rs_row0, bf16_t* ob, int r0, int tt,
                                               int Tb, float scale, float post, int accumulate, const Lane ln) {
  if (accumulate)  // wave-uniform
    final_epilogue_rows<P, true>(acc, RS, rs_row0, ob, r0, tt, Tb, scale, post, ln);
  else
    final_epilogue_rows<P, false>(acc, RS, rs_row0, ob, r0, tt, Tb, scale, post, ln);
}

}  // namespace evmi
