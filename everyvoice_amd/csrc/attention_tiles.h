// Device helpers shared by the attention kernels of attention_train.hip (head dimension 32 / 64 / 128) and attention_generic.hip
// (any head dimension up to 256): the accumulator <-> tile-row mapping, the dropout factors of a score tile, the swizzled
// LDS offsets of the fp32 tiles and the position-slot operand read of the bf16 tiles.
#pragma once

#include "common.h"

namespace evmi {

// value at p (p must be a valid address for every lane), zero for lanes that are not live.  The load is unconditional and the
// select follows it: a load under a per-lane condition is compiled as a branch around it with the memory counter drained behind
// every one (one dependent round trip per element: 128 of them in the prologue of a 128-wide head, 32 per key tile).
__device__ __forceinline__ float live_load(const float* __restrict__ p, bool live) {
  const float v = *p;
  return live ? v : 0.f;
}


// register r of a 32x32 accumulator <-> row index within the tile, for half-wave kh
__device__ __forceinline__ int acc_row(int r, int kh) { return (r & 3) + 8 * (r >> 2) + 4 * kh; }

// Dropout factors (keep or 0) of the 16 accumulator registers of a 32 x 32 score tile.
//   attn_drop_rows: the registers are keys k0 + acc_row(r, kh) of ONE query row (row_base = the row's first element): registers r, r + 1
//                   (r even) are the two elements of a pair -- one hash for both (pairs: T even and the tensor below 2^33 elements)
//   attn_drop_cols: the lane holds ONE key, the registers are queries q0 + acc_row(r, kh): the pair's other element sits in the
//                   neighbouring lane (key ^ 1) at the same register -- each lane hashes the registers of its own parity and the two
//                   exchange (one DPP move per hash)
// Same bits as uniform01(seed, element index) per element (common.h), which the other parities / sizes take.
__device__ __forceinline__ void attn_drop_rows(float (&dm)[16], bool pairs, unsigned long long seed, unsigned long long row_base, int k0, int kh,
                                               float p_drop, float keep) {
  if (pairs) {
    const unsigned jb = (unsigned)(row_base >> 1) + (unsigned)(k0 >> 1) + 2u * (unsigned)kh;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      float u0, u1;
      dropout_pair(seed, jb + (unsigned)(((r & 3) >> 1) + 4 * (r >> 2)), u0, u1);
      dm[r] = u0 >= p_drop ? keep : 0.f;
      dm[r + 1] = u1 >= p_drop ? keep : 0.f;
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) dm[r] = uniform01(seed, row_base + (unsigned long long)(k0 + acc_row(r, kh))) >= p_drop ? keep : 0.f;
  }
}
// (four registers at a time -- 4 g4 .. 4 g4 + 3 -- so that the factors do not stay live across the whole tile)
__device__ __forceinline__ void attn_drop_cols(float (&dm)[4], int g4, bool pairs, unsigned long long seed, unsigned long long batch_base, int tk,
                                               int tkc, int q0, int kh, int T, float p_drop, float keep) {
  if (pairs) {
    const unsigned par = (unsigned)tk & 1u, th = (unsigned)T >> 1;
    const unsigned jb = (unsigned)((batch_base + (unsigned long long)(tk & ~1)) >> 1);  // (the pair's index: not the clamped key's)
#pragma unroll
    for (int c = 0; c < 2; ++c) {
      const int tq = q0 + 8 * g4 + 4 * kh + 2 * c + (int)par;  // query of register 4 g4 + 2 c + par
      const unsigned mine = dropout_hash(seed, jb + (unsigned)min(tq, T - 1) * th, 0u);
      const unsigned other = (unsigned)__builtin_amdgcn_mov_dpp((int)mine, 0xB1, 0xF, 0xF, true);  // quad_perm [1, 0, 3, 2]: lane ^ 1
      const unsigned h0 = par ? other : mine, h1 = par ? mine : other;                              // registers 4 g4 + 2 c and + 1
      dm[2 * c] = dropout_u16(h0, par) >= p_drop ? keep : 0.f;
      dm[2 * c + 1] = dropout_u16(h1, par) >= p_drop ? keep : 0.f;
    }
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int tq = q0 + 8 * g4 + 4 * kh + e;
      dm[e] = uniform01(seed, batch_base + (unsigned long long)tkc + (unsigned long long)min(tq, T - 1) * (unsigned long long)T) >= p_drop ? keep : 0.f;
    }
  }
}
static inline bool attn_drop_pairs(int B, int T) { return !(T & 1) && (unsigned long long)B * T * T < (1ull << 33); }

typedef __attribute__((address_space(3))) float atf_lds_float_t;
typedef __attribute__((address_space(1))) const float atf_glb_float_t;
// Per-lane offsets of the two kinds of read, computed once (32 registers; the rest of an address is an instruction immediate):
//   along a row : lane reads column ln of row 2 s + kh             -> (2 s + kh) * 32 + row_off[s & 15]
//   across rows : lane reads column acc_row(r, kh) of row 32 i + ln -> i * 1024 + col_off[r]
struct SwzOffsets {
  int row_off[16], col_off[16];
  __device__ __forceinline__ SwzOffsets(int ln, int kh) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      row_off[j] = ln ^ ((2 * j + kh) & 31);
      col_off[j] = ln * 32 + (((j & 3) + 8 * (j >> 2) + 4 * kh) ^ ln);
    }
  }
  __device__ __forceinline__ int along(int s, int kh) const { return (2 * s + kh) * 32 + row_off[s & 15]; }
  __device__ __forceinline__ int across(int i, int r) const { return i * 1024 + col_off[r]; }
};

constexpr int ATB_PD = 8;  // bf16 row padding

typedef __attribute__((address_space(3))) float at_lds_float_t;
typedef __attribute__((address_space(1))) const float at_glb_float_t;

// A operand of a contraction over the tile's positions: lane (channel row, half) takes positions 16 kb + 4 half + {0..3} and + 8
__device__ __forceinline__ bf16x8 load_pos_slots(const bf16_t* __restrict__ row, int kb, int kh) {
  const bf16x4 lo = *reinterpret_cast<const bf16x4*>(row + 16 * kb + 4 * kh);
  const bf16x4 hi = *reinterpret_cast<const bf16x4*>(row + 16 * kb + 4 * kh + 8);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

// attention_train.hip: D[b][h][t] = sum_d dO[d][b][t] * O[d][b][t] for any head dimension (attention_rowdot_kernel)
void launch_attention_rowdot(const float* out, const float* dout, float* dsum, int B, int T, int heads, int dh, hipStream_t s);

}  // namespace evmi
