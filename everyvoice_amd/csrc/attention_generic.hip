// Multi-head self-attention at ANY head dimension 1 <= dh <= 256: the kernels of attention_train.hip with the head
// dimension padded to DHP, one of 32 / 64 / 96 / 128 / 192 / 256, and the real dh a run-time argument.  Same mathematics, tensor
// layouts, masking and dropout stream as the specialised kernels (see the header of attention_train.hip):
//
//   qkv [3D][B][T] channel-major, lens [B] (key padding mask) -> out [D][B][T], lse [B][H][T] (+inf for a row without keys)
//
// The padding rule.  Channels dh .. DHP - 1 of a head do not exist in memory:
//   * every load of one is CLAMPED to channel dh - 1 of the same head (a valid, finite row; never a neighbour's memory);
//   * in a contraction over the head dimension (S = Q K^T, dPd = dO V^T) BOTH operands of a padded channel are finite and one is
//     exactly zero: the register-side operand (qreg / doreg / kreg / vreg) is zeroed by a select, the LDS side holds the clamped
//     row (fp32: LDS-direct loads have no conversion step) or zeros (bf16: tile_convert_g).  A zero alone is not enough: 0 * NaN
//     and 0 * Inf are NaN, and what lies behind a head's last channel is whatever the caller keeps there;
//   * in a contraction over keys or queries (O = P V, dQ, dK, dV) the padded channels are OUTPUT rows: computed, never stored.
//
// Registers.  The register-resident operands grow with DHP (DHP / 2 floats each for Q and dO, 16 accumulators per 32 output
// channels), and a wave has 512 registers at one wave per SIMD.  Where a whole head does not fit:
//   * fp32 backward: KS = 2 or 4 waves share 32 queries (keys), each contracting over 1 / KS of the channels (ag_group_sum);
//   * fp32 forward at 256, bf16 dK / dV at 128 and 256: the OUTPUT channels of a head are split across NS = DHP / 32 / NC
//     workgroups, each recomputing the score tile and owning NC 32-channel chunks of the accumulators.
// Either way one writer per output element and a fixed summation order: the backward stays bitwise reproducible.  The bf16
// kernels are bounded to two waves per SIMD up to DHP = 128 and one above.  No instantiation uses scratch memory.
#include <type_traits>

#include "attention_tiles.h"

namespace evmi {
namespace {

// ---- tiles ---------------------------------------------------------------------------------------------------------------
// fp32: rows row0 .. row0 + ROWS - 1 (clamped to dh - 1) of a head's channel-major slice, columns t0 .. t0 + 31 (clamped to
// T - 1), by LDS-direct loads into the swizzled operand layout of attention_train.hip: element (d, t) at d * 32 + (t ^ (d & 31))
template <int ROWS>
__device__ __forceinline__ void tile_request_swz_g(float* __restrict__ dst, const float* __restrict__ src, long long N, int row0, int dh, int t0,
                                                   int T, int tid) {
  const int d0 = tid >> 5, p = tid & 31;
  float* l = dst + (tid & ~63);
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) {
    const int d = d0 + 8 * i;
    // (opaque to the optimiser: it otherwise keeps every row's 64-bit offset and swizzled column in registers from one step to the
    // next -- ROWS / 8 of them per tile, which the wide heads do not have -- where recomputing them is a few operations per load)
    int row = min(row0 + d, dh - 1), col = p;
    asm volatile("" : "+v"(row), "+v"(col));
    const float* g = src + (long long)row * N + min(t0 + (col ^ (d & 31)), T - 1);
    __builtin_amdgcn_global_load_lds((atf_glb_float_t*)g, (atf_lds_float_t*)(l + 256 * i), 4, 0, 0);
  }
}
// bf16: the raw fp32 [ROWS][32] tile, element v = tid + 256 i (row v >> 5, column v & 31) at raw[v]
template <int ROWS>
__device__ __forceinline__ void tile_request_g(float* __restrict__ raw, const float* __restrict__ src, long long N, int row0, int dh, int t0, int T,
                                               int tid) {
  const int d0 = tid >> 5, col = min(t0 + (tid & 31), T - 1);
  float* l = raw + (tid & ~63);
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) {
    int row = min(row0 + d0 + 8 * i, dh - 1);
    asm volatile("" : "+v"(row));  // (as in tile_request_swz_g)
    const float* g = src + (long long)row * N + col;
    __builtin_amdgcn_global_load_lds((at_glb_float_t*)g, (at_lds_float_t*)(l + 256 * i), 4, 0, 0);
  }
}
// the thread's own elements of a landed tile -> bf16 [position][channel] (PC, row stride LP) and / or [channel][position] (CP),
// zero past T and zero for the padded channels (row0 + row >= dh)
template <int ROWS, int LP, bool PC, bool CP>
__device__ __forceinline__ void tile_convert_g(const float* __restrict__ raw, bf16_t* __restrict__ x_pc, bf16_t* __restrict__ x_cp, int row0, int dh,
                                               int t0, int T, int tid) {
  constexpr int LC = 32 + ATB_PD;
  const int tt = tid & 31, d0 = tid >> 5;
  const bool in = t0 + tt < T;
  float r[ROWS / 8];
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) r[i] = raw[tid + 256 * i];
#pragma unroll
  for (int i = 0; i < ROWS / 8; ++i) {
    const bf16_t val = (bf16_t)((in && row0 + d0 + 8 * i < dh) ? r[i] : 0.f);
    if (PC) x_pc[tt * LP + d0 + 8 * i] = val;
    if (CP) x_cp[(d0 + 8 * i) * LC + tt] = val;
  }
}

// The two kinds of read of a swizzled tile (SwzOffsets of attention_tiles.h) with ONE exclusive-or per read in place of 32 offset
// registers -- the registers are what a 192- or 256-wide head has none to spare of, and the operation hides under the matrix cores:
//   along a row : column ln of row 2 s + kh              -> 64 s + ((32 kh | (ln ^ kh)) ^ (2 s & 31))
//   across rows : column acc_row(r, kh) of row 32 i + ln -> 1024 i + ((32 ln | (ln ^ 4 kh)) ^ ((r & 3) + 8 (r >> 2)))
struct SwzXor {
  int row_base, col_base;
  __device__ __forceinline__ SwzXor(int ln, int kh) : row_base(32 * kh | (ln ^ kh)), col_base(32 * ln | (ln ^ 4 * kh)) {}
  __device__ __forceinline__ int along(int s, int) const { return 64 * s + (row_base ^ ((2 * s) & 31)); }
  __device__ __forceinline__ int across(int i, int r) const { return 1024 * i + (col_base ^ ((r & 3) + 8 * (r >> 2))); }
};

// channel c of a head at position t (clamped by the caller), zero for a dead lane or a padded channel
__device__ __forceinline__ float chan_load(const float* __restrict__ base, long long N, int c, int dh, int t, bool live) {
  return live_load(base + (long long)min(c, dh - 1) * N + t, live && c < dh);
}

// ---- fp32 operands (v_mfma_f32_32x32x2_f32) ---------------------------------------------------------------------------------
// grid (ceil(T / 128) * NS, H, B), 256 threads: every wave owns 32 queries; workgroup part = blockIdx.x % NS owns the output
// channels part * NC * 32 .. + NC * 32 - 1 of the head.  lse may be NULL (the inference forward).
template <int DHP, int NC>
__global__ __launch_bounds__(256) void attention_generic_fwd_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                                   float* __restrict__ out, float* __restrict__ lse, int B, int T, int D, int dh,
                                                                   float scale, float p_drop, SeedArg seed_arg) {
  constexpr int NS = DHP / 32 / NC, VR = NC * 32;
  const unsigned long long seed = seed_arg.get();
  extern __shared__ __attribute__((aligned(16))) float ag_lds[];
  float* Kb = ag_lds;                  // [2 generations][DHP][32], swizzled
  float* Vb = ag_lds + 2 * DHP * 32;   // [2 generations][VR][32]: the workgroup's own output channels
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, kh = lane >> 5;
  const SwzXor sw(ln, kh);
  const int part = blockIdx.x % NS, c0 = part * VR;
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = min(lens[b], T);
  const long long N = (long long)B * T;
  const float* q = qkv + ((long long)(h * dh) * B + b) * T;
  const float* kg = qkv + ((long long)(D + h * dh) * B + b) * T;
  const float* vg = qkv + ((long long)(2 * D + h * dh) * B + b) * T;
  if (len > 0) {
    tile_request_swz_g<DHP>(Kb, kg, N, 0, dh, 0, T, tid);
    tile_request_swz_g<VR>(Vb, vg, N, c0, dh, 0, T, tid);
  }
  const int tq = (blockIdx.x / NS) * 128 + wave * 32 + ln;
  const bool qlive = tq < T;
  const int tqc = min(tq, T - 1);
  float qreg[DHP / 2];
#pragma unroll
  for (int s = 0; s < DHP / 2; ++s) qreg[s] = chan_load(q, N, 2 * s + kh, dh, tqc, qlive) * scale;
  f32x16 acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  const unsigned long long row_base = ((unsigned long long)b * T + (unsigned long long)(qlive ? tq : 0)) * T;

  for (int k0 = 0, gen = 0; k0 < len; k0 += 32, gen ^= 1) {
    lds_dma_barrier();  // this step's tiles have landed for every wave; the other generation's readers are done
    if (k0 + 32 < len) {
      tile_request_swz_g<DHP>(Kb + (gen ^ 1) * DHP * 32, kg, N, 0, dh, k0 + 32, T, tid);
      tile_request_swz_g<VR>(Vb + (gen ^ 1) * VR * 32, vg, N, c0, dh, k0 + 32, T, tid);
    }
    const float* Ks = Kb + gen * DHP * 32;
    const float* Vs = Vb + gen * VR * 32;
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < DHP / 2; ++s) st = __builtin_amdgcn_mfma_f32_32x32x2f32(Ks[sw.along(s, kh)], qreg[s], st, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      if (k0 + acc_row(r, kh) >= len) st[r] = -INFINITY;
      mx = fmaxf(mx, st[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);  // finite: every processed tile has a valid key
    const float corr = expf(m_run - m_new);
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = expf(st[r] - m_new);
      ps += st[r];  // the normaliser sums the probabilities BEFORE dropout
      if (p_drop > 0.f)
        st[r] = uniform01(seed + h, row_base + (unsigned long long)(k0 + acc_row(r, kh))) >= p_drop ? st[r] * keep : 0.f;
    }
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * corr + ps;
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] *= corr;
#pragma unroll
      for (int r = 0; r < 16; ++r)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(Vs[sw.across(i, r)], st[r], acc[i], 0, 0, 0);
    }
  }
  if (!qlive) return;
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;  // an item of length 0 has no keys: zero rows
  float* o = out + ((long long)(h * dh) * B + b) * T + tq;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + i * 32 + acc_row(r, kh);
      if (c < dh) o[(long long)c * N] = acc[i][r] * inv;
    }
  if (kh == 0 && part == 0 && lse) lse[((long long)b * H + h) * T + tq] = l_run > 0.f ? m_run + logf(l_run) : INFINITY;
}

// A head wider than 128 channels in the two backward kernels: its register operands (DHP / 2 floats for each of two tensors) and
// its accumulators do not fit one wave, so KS = 2 or 4 waves SHARE 32 queries (keys).  Each holds 1 / KS of the head's channels,
// contracts the score tile over them, and the group exchanges the partial tiles through LDS -- every wave adds them in wave order:
// the same bits in all of them; then each owns the output channels of its share.  Nothing is computed twice, every output element
// still has one writer and a fixed summation order.  v: this wave's partial tile; xch: [4 waves][16 registers][64 lanes].
template <int KS>
__device__ __forceinline__ f32x16 ag_group_sum(float* __restrict__ xch, f32x16 v, int wave, int lane) {
  float* mine = xch + wave * 1024 + lane;
  const float* first = xch + (wave & ~(KS - 1)) * 1024 + lane;
#pragma unroll
  for (int r = 0; r < 16; ++r) mine[r * 64] = v[r];
  lds_barrier();
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    float t = first[r * 64];
#pragma unroll
    for (int j = 1; j < KS; ++j) t += first[j * 1024 + r * 64];
    v[r] = t;
  }
  lds_barrier();  // the next exchange overwrites what the others read here
  return v;
}

// dQ: grid (ceil(T / (128 / KS)), H, B); every wave (group of KS waves) owns 32 queries and walks the key tiles
template <int DHP, int KS>
__global__ __launch_bounds__(256) void attention_generic_dq_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                                  const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                  const float* __restrict__ dsum, float* __restrict__ dqkv, int B, int T,
                                                                  int D, int dh, float scale, float p_drop, SeedArg seed_arg) {
  constexpr int NC = DHP / 32 / KS, SH = DHP / 2 / KS;  // this wave's output chunks and register operands (channels 2 (half SH + s) + kh)
  const unsigned long long seed = seed_arg.get();
  extern __shared__ __attribute__((aligned(16))) float ag_lds[];
  float* Kb = ag_lds;                  // [2 generations][DHP][32], swizzled
  float* Vb = ag_lds + 2 * DHP * 32;
  float* xch = ag_lds + 4 * DHP * 32;  // (KS > 1) the groups' exchange
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, kh = lane >> 5;
  const SwzXor sw(ln, kh);
  const int grp = wave / KS, half = wave % KS, c0 = half * NC * 32;
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = min(lens[b], T);
  const long long N = (long long)B * T;
  const float* q = qkv + ((long long)(h * dh) * B + b) * T;
  const float* kg = qkv + ((long long)(D + h * dh) * B + b) * T;
  const float* vg = qkv + ((long long)(2 * D + h * dh) * B + b) * T;
  const float* dog = d_o + ((long long)(h * dh) * B + b) * T;
  if (len > 0) {
    tile_request_swz_g<DHP>(Kb, kg, N, 0, dh, 0, T, tid);
    tile_request_swz_g<DHP>(Vb, vg, N, 0, dh, 0, T, tid);
  }
  const int tq = blockIdx.x * (128 / KS) + grp * 32 + ln;
  const bool qlive = tq < T;
  const int tqc = min(tq, T - 1);
  float qreg[SH], doreg[SH];
#pragma unroll
  for (int s = 0; s < SH; ++s) {
    qreg[s] = chan_load(q, N, 2 * (half * SH + s) + kh, dh, tqc, qlive) * scale;
    doreg[s] = chan_load(dog, N, 2 * (half * SH + s) + kh, dh, tqc, qlive);
  }
  const float my_lse_raw = lse[((long long)b * H + h) * T + tqc];
  const float my_lse = qlive ? my_lse_raw : INFINITY;
  const float my_d = live_load(dsum + ((long long)b * H + h) * T + tqc, qlive);
  const float keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  const unsigned long long row_base = ((unsigned long long)b * T + (unsigned long long)(qlive ? tq : 0)) * T;
  f32x16 acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  for (int k0 = 0, gen = 0; k0 < len; k0 += 32, gen ^= 1) {
    lds_dma_barrier();
    if (k0 + 32 < len) {
      tile_request_swz_g<DHP>(Kb + (gen ^ 1) * DHP * 32, kg, N, 0, dh, k0 + 32, T, tid);
      tile_request_swz_g<DHP>(Vb + (gen ^ 1) * DHP * 32, vg, N, 0, dh, k0 + 32, T, tid);
    }
    const float* Ks = Kb + gen * DHP * 32;
    const float* Vs = Vb + gen * DHP * 32;
    const float* Kh = Ks + half * SH * 64;  // rows 2 half SH .. : this wave's half of the contraction (2 SH is a multiple of 32)
    const float* Vh = Vs + half * SH * 64;
    f32x16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
#pragma unroll
    for (int s = 0; s < SH; ++s) {
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(Kh[sw.along(s, kh)], qreg[s], st, 0, 0, 0);   // S^T  = K Q^T
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(Vh[sw.along(s, kh)], doreg[s], dp, 0, 0, 0);  // dPd^T = V dO^T
    }
    if (KS > 1) {
      st = ag_group_sum<KS>(xch, st, wave, lane);
      dp = ag_group_sum<KS>(xch, dp, wave, lane);
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, kh);
      const float pr = key < len ? expf(st[r] - my_lse) : 0.f;
      float g = dp[r];
      if (p_drop > 0.f) g = uniform01(seed + h, row_base + (unsigned long long)key) >= p_drop ? g * keep : 0.f;
      st[r] = pr * (g - my_d);  // dS^T as it lies: lane = query, register = key
    }
    const float* Kc = Ks + c0 * 32;  // this wave's own output channels
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r)  // dQ^T [d][query] += K^T [d][key] dS^T [key][query]
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(Kc[sw.across(i, r)], st[r], acc[i], 0, 0, 0);
  }
  if (!qlive) return;
  float* o = dqkv + ((long long)(h * dh) * B + b) * T + tq;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + i * 32 + acc_row(r, kh);
      if (c < dh) o[(long long)c * N] = acc[i][r] * scale;
    }
}

// dK and dV: grid (ceil(T / (128 / KS)), H, B); every wave (group of KS waves) owns 32 keys and walks the query tiles
template <int DHP, int KS>
__global__ __launch_bounds__(256) void attention_generic_dkv_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                                   const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                   const float* __restrict__ dsum, float* __restrict__ dqkv, int B, int T,
                                                                   int D, int dh, float scale, float p_drop, SeedArg seed_arg) {
  constexpr int NC = DHP / 32 / KS, SH = DHP / 2 / KS;
  const unsigned long long seed = seed_arg.get();
  extern __shared__ __attribute__((aligned(16))) float ag_lds[];
  float* Qb = ag_lds;                  // [2 generations][DHP][32], swizzled
  float* Ob = ag_lds + 2 * DHP * 32;
  float* stat = ag_lds + 4 * DHP * 32; // [2 generations][lse of the 32 queries | D of the 32 queries]
  float* xch = stat + 128;             // (KS > 1) the groups' exchange
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, kh = lane >> 5;
  const SwzXor sw(ln, kh);
  const int grp = wave / KS, half = wave % KS, c0 = half * NC * 32, tile0 = blockIdx.x * (128 / KS);
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = min(lens[b], T);
  const long long N = (long long)B * T;
  const float* qg = qkv + ((long long)(h * dh) * B + b) * T;
  const float* kg = qkv + ((long long)(D + h * dh) * B + b) * T;
  const float* vg = qkv + ((long long)(2 * D + h * dh) * B + b) * T;
  const float* dog = d_o + ((long long)(h * dh) * B + b) * T;
  const int tk = tile0 + grp * 32 + ln;
  const bool klive = tk < len;
  const int tkc = min(tk, T - 1);  // padded keys receive no probability mass: zero gradients
  float kreg[SH], vreg[SH];
#pragma unroll
  for (int s = 0; s < SH; ++s) {
    kreg[s] = chan_load(kg, N, 2 * (half * SH + s) + kh, dh, tkc, klive) * scale;
    vreg[s] = chan_load(vg, N, 2 * (half * SH + s) + kh, dh, tkc, klive);
  }
  const float keep = p_drop > 0.f ? 1.f / (1.f - p_drop) : 1.f;
  f32x16 acck[NC], accv[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acck[i][r] = accv[i][r] = 0.f;
  const bool block_live = tile0 < len;  // uniform per workgroup
  // wave 0 also brings the tile's 32 (lse, D) pairs: lanes 0-31 the lse, lanes 32-63 D, clamped (queries past T are masked below)
  const float* stat_src = (kh ? dsum : lse) + ((long long)b * H + h) * T;
  auto request = [&](int q0, int gen) {
    tile_request_swz_g<DHP>(Qb + gen * DHP * 32, qg, N, 0, dh, q0, T, tid);
    tile_request_swz_g<DHP>(Ob + gen * DHP * 32, dog, N, 0, dh, q0, T, tid);
    if (wave == 0) __builtin_amdgcn_global_load_lds((atf_glb_float_t*)(stat_src + min(q0 + ln, T - 1)), (atf_lds_float_t*)(stat + 64 * gen), 4, 0, 0);
  };
  if (block_live) request(0, 0);

  for (int q0 = 0, gen = 0; q0 < T && block_live; q0 += 32, gen ^= 1) {
    lds_dma_barrier();
    if (q0 + 32 < T) request(q0 + 32, gen ^ 1);
    const float* Qs = Qb + gen * DHP * 32;
    const float* Os = Ob + gen * DHP * 32;
    const float* lse_s = stat + 64 * gen;
    const float* d_s = lse_s + 32;
    const float* Qh = Qs + half * SH * 64;  // this wave's half of the contraction
    const float* Oh = Os + half * SH * 64;
    f32x16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
#pragma unroll
    for (int s = 0; s < SH; ++s) {
      st = __builtin_amdgcn_mfma_f32_32x32x2f32(Qh[sw.along(s, kh)], kreg[s], st, 0, 0, 0);  // S   = Q K^T : lane = key, registers = queries
      dp = __builtin_amdgcn_mfma_f32_32x32x2f32(Oh[sw.along(s, kh)], vreg[s], dp, 0, 0, 0);  // dPd = dO V^T
    }
    if (KS > 1) {
      st = ag_group_sum<KS>(xch, st, wave, lane);
      dp = ag_group_sum<KS>(xch, dp, wave, lane);
    }
    f32x16 pd;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int qi = acc_row(r, kh);
      const int tq = q0 + qi;
      float pr = expf(st[r] - lse_s[qi]);
      pr = (klive && tq < T) ? pr : 0.f;
      float mk = 1.f;
      if (p_drop > 0.f) mk = uniform01(seed + h, ((unsigned long long)b * T + (unsigned long long)min(tq, T - 1)) * T + (unsigned long long)min(tk, T - 1)) >= p_drop ? keep : 0.f;
      pd[r] = pr * mk;                        // Pd   : the dropped-out probabilities that multiplied V
      st[r] = pr * (dp[r] * mk - d_s[qi]);    // dS
    }
    const float* Qc = Qs + c0 * 32;  // this wave's own output channels
    const float* Oc = Os + c0 * 32;
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        accv[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(Oc[sw.across(i, r)], pd[r], accv[i], 0, 0, 0);  // dV^T += dO^T Pd
        acck[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(Qc[sw.across(i, r)], st[r], acck[i], 0, 0, 0);  // dK^T += Q^T dS
      }
  }
  if (tk >= T) return;
  float* dk = dqkv + ((long long)(D + h * dh) * B + b) * T + tk;
  float* dv = dqkv + ((long long)(2 * D + h * dh) * B + b) * T + tk;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + i * 32 + acc_row(r, kh);
      if (c < dh) {
        dk[(long long)c * N] = acck[i][r] * scale;
        dv[(long long)c * N] = accv[i][r];
      }
    }
}

// ---- bf16 operands (v_mfma_f32_32x32x16_bf16; fp32 scores, statistics and accumulators) ------------------------------------
// Operand staging as in attention_train.hip: the fp32 tile of step i + 1 lands in a raw area under step i's matrix work and every
// thread converts the elements it requested.  All LDS is dynamic (a 256-wide head needs more than the static limit).
constexpr int ag_occupancy(int DHP) { return DHP > 128 ? 1 : 2; }

template <int DHP, int NC>
constexpr size_t ag_fwd_bf16_lds() {
  return (size_t)(32 * (DHP + ATB_PD) + NC * 32 * (32 + ATB_PD)) * sizeof(bf16_t) + (size_t)(DHP * 32 + NC * 32 * 32) * sizeof(float);
}
template <int DHP>
constexpr size_t ag_dq_bf16_lds() {
  return (size_t)(2 * 32 * (DHP + ATB_PD) + DHP * (32 + ATB_PD)) * sizeof(bf16_t) + (size_t)(2 * DHP * 32) * sizeof(float);
}
template <int DHP>
constexpr size_t ag_dkv_bf16_lds() {
  return (size_t)(2 * 32 * (DHP + ATB_PD) + 2 * DHP * (32 + ATB_PD)) * sizeof(bf16_t) + (size_t)(2 * DHP * 32 + 2 * 64) * sizeof(float);
}

template <int DHP, int NC, int DROP>  // DROP 0: no dropout; 1: one hash per element; 2: one hash per pair of elements (attn_drop_pairs)
__global__ __launch_bounds__(256, ag_occupancy(DHP)) void attention_generic_fwd_bf16_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                                                          float* __restrict__ out, float* __restrict__ lse, int B,
                                                                                          int T, int D, int dh, float scale, float p_drop,
                                                                                          SeedArg seed_arg) {
  constexpr int NS = DHP / 32 / NC, VR = NC * 32;
  const unsigned long long seed = seed_arg.get();
  constexpr int LP = DHP + ATB_PD, LC = 32 + ATB_PD;
  extern __shared__ __attribute__((aligned(16))) unsigned char ag_dyn_lds[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(ag_dyn_lds);  // [key][channel]
  bf16_t* Vs = Ks + 32 * LP;                           // [own channel][key]
  float* rawK = reinterpret_cast<float*>(Vs + VR * LC);
  float* rawV = rawK + DHP * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, kh = lane >> 5;
  const int part = blockIdx.x % NS, c0 = part * VR;
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = min(lens[b], T);
  const long long N = (long long)B * T;
  const float* q = qkv + ((long long)(h * dh) * B + b) * T;
  const float* kg = qkv + ((long long)(D + h * dh) * B + b) * T;
  const float* vg = qkv + ((long long)(2 * D + h * dh) * B + b) * T;
  if (len > 0) {
    tile_request_g<DHP>(rawK, kg, N, 0, dh, 0, T, tid);
    tile_request_g<VR>(rawV, vg, N, c0, dh, 0, T, tid);
  }
  const int tq = (blockIdx.x / NS) * 128 + wave * 32 + ln;
  const bool qlive = tq < T;
  const int tqc = min(tq, T - 1);
  bf16x8 qreg[DHP / 16];
#pragma unroll
  for (int s = 0; s < DHP / 16; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) qreg[s][e] = (bf16_t)(chan_load(q, N, 16 * s + 8 * kh + e, dh, tqc, qlive) * scale);
  f32x16 acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float keep = DROP ? 1.f / (1.f - p_drop) : 1.f;
  constexpr bool drop_pairs = DROP == 2;
  const unsigned long long row_base = ((unsigned long long)b * T + (unsigned long long)(qlive ? tq : 0)) * T;

  for (int k0 = 0; k0 < len; k0 += 32) {
    lds_dma_barrier();  // the requested tile has landed for every wave; the previous step's operand reads are over
    tile_convert_g<DHP, LP, true, false>(rawK, Ks, nullptr, 0, dh, k0, T, tid);
    tile_convert_g<VR, LP, false, true>(rawV, nullptr, Vs, c0, dh, k0, T, tid);
    __syncthreads();
    if (k0 + 32 < len) {
      tile_request_g<DHP>(rawK, kg, N, 0, dh, k0 + 32, T, tid);
      tile_request_g<VR>(rawV, vg, N, c0, dh, k0 + 32, T, tid);
    }
    f32x16 st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
#pragma unroll
    for (int s = 0; s < DHP / 16; ++s)
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&Ks[ln * LP + 16 * s + 8 * kh]), qreg[s], st, 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      st[r] = k0 + acc_row(r, kh) < len ? st[r] : -INFINITY;
      mx = fmaxf(mx, st[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);  // finite: key k0 of the tile is live
    const float corr = __expf(m_run - m_new);
    float ps = 0.f;
    bf16x8 pb[2];
    float dm[16];
    if (DROP) attn_drop_rows(dm, drop_pairs, seed + h, row_base, k0, kh, p_drop, keep);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float pr = __expf(st[r] - m_new);
      ps += pr;
      if (DROP) pr = dm[r] != 0.f ? pr * keep : 0.f;
      pb[r >> 3][r & 7] = (bf16_t)pr;
    }
    ps += __shfl_xor(ps, 32, 64);
    l_run = l_run * corr + ps;
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < NC; ++i) {
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][r] *= corr;
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(load_pos_slots(&Vs[(i * 32 + ln) * LC], kb, kh), pb[kb], acc[i], 0, 0, 0);
    }
  }
  if (!qlive) return;
  const float inv = l_run > 0.f ? 1.f / l_run : 0.f;
  float* o = out + ((long long)(h * dh) * B + b) * T + tq;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + i * 32 + acc_row(r, kh);
      if (c < dh) o[(long long)c * N] = acc[i][r] * inv;
    }
  if (kh == 0 && part == 0 && lse) lse[((long long)b * H + h) * T + tq] = l_run > 0.f ? m_run + logf(l_run) : INFINITY;  // (inference: no lse)
}

template <int DHP, int NC, int DROP>
__global__ __launch_bounds__(256, ag_occupancy(DHP)) void attention_generic_dq_bf16_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                                                         const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                                         const float* __restrict__ dsum, float* __restrict__ dqkv,
                                                                                         int B, int T, int D, int dh, float scale, float p_drop,
                                                                                         SeedArg seed_arg) {
  constexpr int NS = DHP / 32 / NC;
  const unsigned long long seed = seed_arg.get();
  constexpr int LP = DHP + ATB_PD, LC = 32 + ATB_PD;
  extern __shared__ __attribute__((aligned(16))) unsigned char ag_dyn_lds[];
  bf16_t* Ks = reinterpret_cast<bf16_t*>(ag_dyn_lds);  // [key][channel]: S^T = K Q^T
  bf16_t* Kt = Ks + 32 * LP;                           // [channel][key]: dQ^T += K^T dS^T
  bf16_t* Vs = Kt + DHP * LC;                          // [key][channel]: dPd^T = V dO^T
  float* rawK = reinterpret_cast<float*>(Vs + 32 * LP);
  float* rawV = rawK + DHP * 32;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, kh = lane >> 5;
  const int part = blockIdx.x % NS, c0 = part * NC * 32;
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = min(lens[b], T);
  const long long N = (long long)B * T;
  const float* q = qkv + ((long long)(h * dh) * B + b) * T;
  const float* kg = qkv + ((long long)(D + h * dh) * B + b) * T;
  const float* vg = qkv + ((long long)(2 * D + h * dh) * B + b) * T;
  const float* dog = d_o + ((long long)(h * dh) * B + b) * T;
  if (len > 0) {
    tile_request_g<DHP>(rawK, kg, N, 0, dh, 0, T, tid);
    tile_request_g<DHP>(rawV, vg, N, 0, dh, 0, T, tid);
  }
  const int tq = (blockIdx.x / NS) * 128 + wave * 32 + ln;
  const bool qlive = tq < T;
  const int tqc = min(tq, T - 1);
  bf16x8 qreg[DHP / 16], doreg[DHP / 16];
#pragma unroll
  for (int s = 0; s < DHP / 16; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 16 * s + 8 * kh + e;
      qreg[s][e] = (bf16_t)(chan_load(q, N, c, dh, tqc, qlive) * scale);
      doreg[s][e] = (bf16_t)chan_load(dog, N, c, dh, tqc, qlive);
    }
  const float my_lse_raw = lse[((long long)b * H + h) * T + tqc];
  const float my_lse = qlive ? my_lse_raw : INFINITY;
  const float my_d = live_load(dsum + ((long long)b * H + h) * T + tqc, qlive);
  const float keep = DROP ? 1.f / (1.f - p_drop) : 1.f;
  constexpr bool drop_pairs = DROP == 2;
  const unsigned long long row_base = ((unsigned long long)b * T + (unsigned long long)(qlive ? tq : 0)) * T;
  f32x16 acc[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;

  for (int k0 = 0; k0 < len; k0 += 32) {
    lds_dma_barrier();
    tile_convert_g<DHP, LP, true, true>(rawK, Ks, Kt, 0, dh, k0, T, tid);
    tile_convert_g<DHP, LP, true, false>(rawV, Vs, nullptr, 0, dh, k0, T, tid);
    __syncthreads();
    if (k0 + 32 < len) {
      tile_request_g<DHP>(rawK, kg, N, 0, dh, k0 + 32, T, tid);
      tile_request_g<DHP>(rawV, vg, N, 0, dh, k0 + 32, T, tid);
    }
    f32x16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
#pragma unroll
    for (int s = 0; s < DHP / 16; ++s) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&Ks[ln * LP + 16 * s + 8 * kh]), qreg[s], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&Vs[ln * LP + 16 * s + 8 * kh]), doreg[s], dp, 0, 0, 0);
    }
    bf16x8 dsb[2];
    float dm[16];
    if (DROP) attn_drop_rows(dm, drop_pairs, seed + h, row_base, k0, kh, p_drop, keep);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int key = k0 + acc_row(r, kh);
      float pr = __expf(st[r] - my_lse);
      pr = key < len ? pr : 0.f;
      float g = dp[r];
      if (DROP) g = dm[r] != 0.f ? g * keep : 0.f;
      dsb[r >> 3][r & 7] = (bf16_t)(pr * (g - my_d));
    }
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb)
        acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(load_pos_slots(&Kt[(c0 + i * 32 + ln) * LC], kb, kh), dsb[kb], acc[i], 0, 0, 0);
  }
  if (!qlive) return;
  float* o = dqkv + ((long long)(h * dh) * B + b) * T + tq;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + i * 32 + acc_row(r, kh);
      if (c < dh) o[(long long)c * N] = acc[i][r] * scale;
    }
}

template <int DHP, int NC, int DROP>
__global__ __launch_bounds__(256, ag_occupancy(DHP)) void attention_generic_dkv_bf16_kernel(const float* __restrict__ qkv, const int* __restrict__ lens,
                                                                                          const float* __restrict__ d_o, const float* __restrict__ lse,
                                                                                          const float* __restrict__ dsum, float* __restrict__ dqkv,
                                                                                          int B, int T, int D, int dh, float scale, float p_drop,
                                                                                          SeedArg seed_arg) {
  constexpr int NS = DHP / 32 / NC;
  const unsigned long long seed = seed_arg.get();
  constexpr int LP = DHP + ATB_PD, LC = 32 + ATB_PD;
  extern __shared__ __attribute__((aligned(16))) unsigned char ag_dyn_lds[];
  bf16_t* Qs = reinterpret_cast<bf16_t*>(ag_dyn_lds);  // [query][channel]
  bf16_t* Qt = Qs + 32 * LP;                           // [channel][query]
  bf16_t* Os = Qt + DHP * LC;                          // dO [query][channel]
  bf16_t* Ot = Os + 32 * LP;                           // dO [channel][query]
  float* rawQ = reinterpret_cast<float*>(Ot + DHP * LC);
  float* rawO = rawQ + DHP * 32;
  float* stat = rawO + DHP * 32;                       // [2 generations][lse of the 32 queries | D of the 32 queries]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, ln = lane & 31, kh = lane >> 5;
  const int part = blockIdx.x % NS, c0 = part * NC * 32, tile0 = (blockIdx.x / NS) * 128;
  const int h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
  const int len = min(lens[b], T);
  const long long N = (long long)B * T;
  const float* qg = qkv + ((long long)(h * dh) * B + b) * T;
  const float* kg = qkv + ((long long)(D + h * dh) * B + b) * T;
  const float* vg = qkv + ((long long)(2 * D + h * dh) * B + b) * T;
  const float* dog = d_o + ((long long)(h * dh) * B + b) * T;
  const bool block_live = tile0 < len;
  // wave 0 also brings the tile's 32 (lse, D) pairs: lanes 0-31 the lse, lanes 32-63 D, clamped (queries past T are masked below)
  const float* stat_src = (kh ? dsum : lse) + ((long long)b * H + h) * T;
  if (block_live) {
    tile_request_g<DHP>(rawQ, qg, N, 0, dh, 0, T, tid);
    tile_request_g<DHP>(rawO, dog, N, 0, dh, 0, T, tid);
    if (wave == 0) __builtin_amdgcn_global_load_lds((at_glb_float_t*)(stat_src + min(ln, T - 1)), (at_lds_float_t*)stat, 4, 0, 0);
  }
  const int tk = tile0 + wave * 32 + ln;
  const bool klive = tk < len;
  const int tkc = min(tk, T - 1);
  bf16x8 kreg[DHP / 16], vreg[DHP / 16];
#pragma unroll
  for (int s = 0; s < DHP / 16; ++s)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const int c = 16 * s + 8 * kh + e;
      kreg[s][e] = (bf16_t)(chan_load(kg, N, c, dh, tkc, klive) * scale);
      vreg[s][e] = (bf16_t)chan_load(vg, N, c, dh, tkc, klive);
    }
  const float keep = DROP ? 1.f / (1.f - p_drop) : 1.f;
  const unsigned long long batch_base = (unsigned long long)b * T * T;
  constexpr bool drop_pairs = DROP == 2;
  f32x16 acck[NC], accv[NC];
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acck[i][r] = accv[i][r] = 0.f;

  for (int q0 = 0, gen = 0; q0 < T && block_live; q0 += 32, gen ^= 1) {
    lds_dma_barrier();
    tile_convert_g<DHP, LP, true, true>(rawQ, Qs, Qt, 0, dh, q0, T, tid);
    tile_convert_g<DHP, LP, true, true>(rawO, Os, Ot, 0, dh, q0, T, tid);
    __syncthreads();
    if (q0 + 32 < T) {
      tile_request_g<DHP>(rawQ, qg, N, 0, dh, q0 + 32, T, tid);
      tile_request_g<DHP>(rawO, dog, N, 0, dh, q0 + 32, T, tid);
      if (wave == 0)
        __builtin_amdgcn_global_load_lds((at_glb_float_t*)(stat_src + min(q0 + 32 + ln, T - 1)), (at_lds_float_t*)(stat + 64 * (gen ^ 1)), 4, 0, 0);
    }
    f32x16 st, dp;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = dp[r] = 0.f;
#pragma unroll
    for (int s = 0; s < DHP / 16; ++s) {
      st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&Qs[ln * LP + 16 * s + 8 * kh]), kreg[s], st, 0, 0, 0);
      dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*reinterpret_cast<const bf16x8*>(&Os[ln * LP + 16 * s + 8 * kh]), vreg[s], dp, 0, 0, 0);
    }
    // the 16 queries of this half-wave's registers: (r & 3) + 8 (r >> 2) + 4 kh -> four 16-byte vectors of each statistic
    bf16x8 pdb[2], dsb[2];
    const float* st_l = stat + 64 * gen + 4 * kh;
#pragma unroll
    for (int g4 = 0; g4 < 4; ++g4) {
      const f32x4 lse_q = *reinterpret_cast<const f32x4*>(st_l + 8 * g4);
      const f32x4 d_q = *reinterpret_cast<const f32x4*>(st_l + 32 + 8 * g4);
      float dm[4];
      if (DROP) attn_drop_cols(dm, g4, drop_pairs, seed + h, batch_base, tk, tkc, q0, kh, T, p_drop, keep);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int r = 4 * g4 + e;
        const int tq = q0 + 8 * g4 + 4 * kh + e;
        float pr = __expf(st[r] - lse_q[e]);
        pr = (klive && tq < T) ? pr : 0.f;
        const float mk = DROP ? dm[e] : 1.f;
        pdb[r >> 3][r & 7] = (bf16_t)(pr * mk);
        dsb[r >> 3][r & 7] = (bf16_t)(pr * (dp[r] * mk - d_q[e]));
      }
    }
#pragma unroll
    for (int i = 0; i < NC; ++i)
#pragma unroll
      for (int kb = 0; kb < 2; ++kb) {
        accv[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(load_pos_slots(&Ot[(c0 + i * 32 + ln) * LC], kb, kh), pdb[kb], accv[i], 0, 0, 0);
        acck[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(load_pos_slots(&Qt[(c0 + i * 32 + ln) * LC], kb, kh), dsb[kb], acck[i], 0, 0, 0);
      }
  }
  if (tk >= T) return;
  float* dk = dqkv + ((long long)(D + h * dh) * B + b) * T + tk;
  float* dv = dqkv + ((long long)(2 * D + h * dh) * B + b) * T + tk;
#pragma unroll
  for (int i = 0; i < NC; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + i * 32 + acc_row(r, kh);
      if (c < dh) {
        dk[(long long)c * N] = acck[i][r] * scale;
        dv[(long long)c * N] = accv[i][r];
      }
    }
}

// ---- host ------------------------------------------------------------------------------------------------------------------
// Output chunks (of 32 channels) one workgroup owns, per kernel and padded head dimension: the whole head where that compiles
// without scratch, a divisor of DHP / 32 otherwise (DESIGN.md 21 has the resource table these were chosen from).
enum AgKernel { AG_FWD, AG_FWD_BF16, AG_DQ_BF16, AG_DKV_BF16 };
constexpr int ag_chunks(AgKernel k, int DHP) {
  const int all = DHP / 32;
  switch (k) {
    case AG_FWD: return DHP == 256 ? 4 : all;
    case AG_DKV_BF16: return DHP == 256 ? 4 : DHP == 128 ? 2 : all;
    default: return all;
  }
}
// waves that share 32 queries (keys) in the fp32 backward kernels (ag_group_sum)
constexpr int ag_group_dq(int DHP) { return DHP > 128 ? 2 : 1; }
constexpr int ag_group_dkv(int DHP) { return DHP > 192 ? 4 : DHP > 128 ? 2 : 1; }

// body(std::integral_constant<int, DHP>{}) for the smallest padded head dimension that holds dh (1 <= dh <= 256)
template <class F>
int with_padded_head_dim(int dh, F&& body) {
  if (dh <= 32) return body(std::integral_constant<int, 32>{});
  if (dh <= 64) return body(std::integral_constant<int, 64>{});
  if (dh <= 96) return body(std::integral_constant<int, 96>{});
  if (dh <= 128) return body(std::integral_constant<int, 128>{});
  if (dh <= 192) return body(std::integral_constant<int, 192>{});
  return body(std::integral_constant<int, 256>{});
}

// the argument checks every entry point makes before its first HIP call
int check_args(const char* what, bool pointers, int B, int T, int D, int heads, float p_drop) {
  if (!pointers) return fail(EVMI_ERR_INVALID_ARG, std::string(what) + ": null pointer");
  if (B <= 0 || T <= 0 || D <= 0 || heads <= 0 || D % heads || p_drop < 0.f || p_drop >= 1.f)
    return fail(EVMI_ERR_INVALID_ARG, std::string(what) + ": shape / dropout (sizes positive, D a multiple of heads, 0 <= p_drop < 1)");
  if (B > 65535 || heads > 65535) return fail(EVMI_ERR_UNSUPPORTED, std::string(what) + ": grid limits (B and heads at most 65535)");
  if (D / heads > 256) return fail(EVMI_ERR_UNSUPPORTED, std::string(what) + ": head dimension D / heads must be at most 256");
  return EVMI_OK;
}

inline dim3 ag_grid(int T, int parts, int heads, int B) { return dim3((unsigned)((T + 127) / 128 * parts), heads, B); }

int launch_fwd_f32(const char* what, const float* qkv, const int* lens, float* out, float* lse_or_null, int B, int T, int D, int heads, float p_drop,
                   SeedArg seed, hipStream_t s) {
  const int dh = D / heads;
  const float scale = 1.f / sqrtf((float)dh);
  if (int rc = with_padded_head_dim(dh, [&](auto c) {
        constexpr int DHP = decltype(c)::value, NC = ag_chunks(AG_FWD, DHP);
        return launch_with_lds(attention_generic_fwd_kernel<DHP, NC>, ag_grid(T, DHP / 32 / NC, heads, B), dim3(256),
                               (size_t)2 * (DHP + NC * 32) * 32 * sizeof(float), s, qkv, lens, out, lse_or_null, B, T, D, dh, scale, p_drop, seed);
      }))
    return rc;
  EVMI_LAUNCH_CHECK(what);
  return EVMI_OK;
}

int launch_fwd_bf16(const char* what, const float* qkv, const int* lens, float* out, float* lse_or_null, int B, int T, int D, int heads, float p_drop,
                    SeedArg seed, hipStream_t s) {
  const int dh = D / heads;
  const float scale = 1.f / sqrtf((float)dh);
  const int drop = p_drop > 0.f ? (attn_drop_pairs(B, T) ? 2 : 1) : 0;
  if (int rc = with_padded_head_dim(dh, [&](auto c) {
        constexpr int DHP = decltype(c)::value, NC = ag_chunks(AG_FWD_BF16, DHP);
        const auto fwd = drop == 2   ? attention_generic_fwd_bf16_kernel<DHP, NC, 2>
                         : drop == 1 ? attention_generic_fwd_bf16_kernel<DHP, NC, 1>
                                     : attention_generic_fwd_bf16_kernel<DHP, NC, 0>;
        return launch_with_lds(fwd, ag_grid(T, DHP / 32 / NC, heads, B), dim3(256), ag_fwd_bf16_lds<DHP, NC>(), s, qkv, lens, out, lse_or_null, B, T,
                               D, dh, scale, p_drop, seed);
      }))
    return rc;
  EVMI_LAUNCH_CHECK(what);
  return EVMI_OK;
}

}  // namespace
}  // namespace evmi

using namespace evmi;

extern "C" {

int evmi_attention_generic_f32(const float* qkv_dev, const int* lens_dev, float* out_dev, int B, int T, int D, int heads, void* stream) {
  if (int rc = check_args("attention_generic_f32", qkv_dev && lens_dev && out_dev, B, T, D, heads, 0.f)) return rc;
  return launch_fwd_f32("attention_generic_f32", qkv_dev, lens_dev, out_dev, nullptr, B, T, D, heads, 0.f, SeedArg{0ull, nullptr}, (hipStream_t)stream);
}

int evmi_attention_generic_bf16(const float* qkv_dev, const int* lens_dev, float* out_dev, int B, int T, int D, int heads, void* stream) {
  if (int rc = check_args("attention_generic_bf16", qkv_dev && lens_dev && out_dev, B, T, D, heads, 0.f)) return rc;
  return launch_fwd_bf16("attention_generic_bf16", qkv_dev, lens_dev, out_dev, nullptr, B, T, D, heads, 0.f, SeedArg{0ull, nullptr}, (hipStream_t)stream);
}

int evmi_mha_generic_fwd_f32(const float* qkv_dev, const int* lens_dev, float* out_dev, float* lse_dev, int B, int T, int D, int heads,
                             float p_drop, unsigned long long seed_value, const unsigned long long* seed_base_dev, void* stream) {
  if (int rc = check_args("mha_generic_fwd_f32", qkv_dev && lens_dev && out_dev && lse_dev, B, T, D, heads, p_drop)) return rc;
  return launch_fwd_f32("mha_generic_fwd_f32", qkv_dev, lens_dev, out_dev, lse_dev, B, T, D, heads, p_drop, SeedArg{seed_value, seed_base_dev},
                        (hipStream_t)stream);
}

int evmi_mha_generic_fwd_bf16(const float* qkv_dev, const int* lens_dev, float* out_dev, float* lse_dev, int B, int T, int D, int heads,
                              float p_drop, unsigned long long seed_value, const unsigned long long* seed_base_dev, void* stream) {
  if (int rc = check_args("mha_generic_fwd_bf16", qkv_dev && lens_dev && out_dev && lse_dev, B, T, D, heads, p_drop)) return rc;
  return launch_fwd_bf16("mha_generic_fwd_bf16", qkv_dev, lens_dev, out_dev, lse_dev, B, T, D, heads, p_drop, SeedArg{seed_value, seed_base_dev},
                         (hipStream_t)stream);
}

int evmi_mha_generic_bwd_f32(const float* qkv_dev, const int* lens_dev, const float* out_dev, const float* dout_dev, const float* lse_dev,
                             float* dsum_dev, float* dqkv_dev, int B, int T, int D, int heads, float p_drop, unsigned long long seed_value,
                             const unsigned long long* seed_base_dev, void* stream) {
  if (int rc = check_args("mha_generic_bwd_f32", qkv_dev && lens_dev && out_dev && dout_dev && lse_dev && dsum_dev && dqkv_dev, B, T, D, heads, p_drop))
    return rc;
  const SeedArg seed{seed_value, seed_base_dev};
  const int dh = D / heads;
  const float scale = 1.f / sqrtf((float)dh);
  hipStream_t s = (hipStream_t)stream;
  launch_attention_rowdot(out_dev, dout_dev, dsum_dev, B, T, heads, dh, s);
  if (int rc = with_padded_head_dim(dh, [&](auto c) {
        constexpr int DHP = decltype(c)::value, KQ = ag_group_dq(DHP), KKV = ag_group_dkv(DHP);
        constexpr size_t tiles = (size_t)4 * DHP * 32 * sizeof(float), xch = 4096 * sizeof(float);
        if (int rc = launch_with_lds(attention_generic_dq_kernel<DHP, KQ>, dim3((unsigned)((T + 128 / KQ - 1) / (128 / KQ)), heads, B), dim3(256),
                                     tiles + (KQ > 1 ? xch : 0), s, qkv_dev, lens_dev, dout_dev, lse_dev, dsum_dev, dqkv_dev, B, T, D, dh, scale,
                                     p_drop, seed))
          return rc;
        return launch_with_lds(attention_generic_dkv_kernel<DHP, KKV>, dim3((unsigned)((T + 128 / KKV - 1) / (128 / KKV)), heads, B), dim3(256),
                               tiles + 128 * sizeof(float) + (KKV > 1 ? xch : 0), s, qkv_dev, lens_dev, dout_dev, lse_dev, dsum_dev, dqkv_dev, B, T,
                               D, dh, scale, p_drop, seed);
      }))
    return rc;
  EVMI_LAUNCH_CHECK("mha_generic_bwd_f32");
  return EVMI_OK;
}

int evmi_mha_generic_bwd_bf16(const float* qkv_dev, const int* lens_dev, const float* out_dev, const float* dout_dev, const float* lse_dev,
                              float* dsum_dev, float* dqkv_dev, int B, int T, int D, int heads, float p_drop, unsigned long long seed_value,
                              const unsigned long long* seed_base_dev, void* stream) {
  if (int rc = check_args("mha_generic_bwd_bf16", qkv_dev && lens_dev && out_dev && dout_dev && lse_dev && dsum_dev && dqkv_dev, B, T, D, heads, p_drop))
    return rc;
  const SeedArg seed{seed_value, seed_base_dev};
  const int dh = D / heads;
  const float scale = 1.f / sqrtf((float)dh);
  hipStream_t s = (hipStream_t)stream;
  launch_attention_rowdot(out_dev, dout_dev, dsum_dev, B, T, heads, dh, s);
  const int drop = p_drop > 0.f ? (attn_drop_pairs(B, T) ? 2 : 1) : 0;
  if (int rc = with_padded_head_dim(dh, [&](auto c) {
        constexpr int DHP = decltype(c)::value, NQ = ag_chunks(AG_DQ_BF16, DHP), NKV = ag_chunks(AG_DKV_BF16, DHP);
        const auto dq = drop == 2   ? attention_generic_dq_bf16_kernel<DHP, NQ, 2>
                        : drop == 1 ? attention_generic_dq_bf16_kernel<DHP, NQ, 1>
                                    : attention_generic_dq_bf16_kernel<DHP, NQ, 0>;
        const auto dkv = drop == 2   ? attention_generic_dkv_bf16_kernel<DHP, NKV, 2>
                         : drop == 1 ? attention_generic_dkv_bf16_kernel<DHP, NKV, 1>
                                     : attention_generic_dkv_bf16_kernel<DHP, NKV, 0>;
        if (int rc = launch_with_lds(dq, ag_grid(T, DHP / 32 / NQ, heads, B), dim3(256), ag_dq_bf16_lds<DHP>(), s, qkv_dev, lens_dev, dout_dev, lse_dev,
                                     dsum_dev, dqkv_dev, B, T, D, dh, scale, p_drop, seed))
          return rc;
        return launch_with_lds(dkv, ag_grid(T, DHP / 32 / NKV, heads, B), dim3(256), ag_dkv_bf16_lds<DHP>(), s, qkv_dev, lens_dev, dout_dev, lse_dev,
                               dsum_dev, dqkv_dev, B, T, D, dh, scale, p_drop, seed);
      }))
    return rc;
  EVMI_LAUNCH_CHECK("mha_generic_bwd_bf16");
  return EVMI_OK;
}

}  // extern "C"
