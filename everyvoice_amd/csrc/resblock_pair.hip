// Instantiations and launchers of the fused residual kernels (resblock_pair_kernel.h, resblock_pair_chunked_kernel.h,
// resblock_branch_kernel.h; their shared device code: resblock_tiles.h).

#include "resblock_branch_kernel.h"
#include "resblock_pair_chunked_kernel.h"

namespace evmi {

//                  C  KS  BN  TAPS MAXDIL WAVES NWBUF WRES WM   (sixteen waves at 32 channels: four per SIMD keep the VALU-bound activation
//                  passes and the LDS latency of the short MFMA steps covered, -7 ... -9 %; at 64 channels the 2 (channels) x 8 (rows) split
//                  costs a fragment read per MFMA instead of 0.75 and measured equal or slower: eight waves there)
// C = 32: all taps of one convolution fit LDS at once (single buffer): 2 weight steps per tile.  (Measured and removed in round 5:
// a two-workgroups-per-CU form with T1 overlaying the operand tile, 1.22 vs 1.16 ms on c32 / k11; a conv1 / conv2 wave pipeline
// with the weights in registers, 17.82 vs 17.63 ms per forward -- DESIGN.md §9.7, §9.11.)
#define EVMI_PAIR_TABLE(X)               \
  X(64, 3, 256, 2, 5, 8, 2, WR, 1)       \
  X(64, 7, 256, 2, 5, 8, 2, WR, 1)       \
  X(64, 11, 256, 2, 5, 8, 2, WR, 1)      \
  X(32, 3, 512, 3, 5, 8, 2, 0, 1)        \
  X(32, 7, 512, 7, 5, 8, 1, 0, 1)        \
  X(32, 11, 512, 11, 5, 16, 1, WR, 1)

static const PairLaunch* pair_table(int* n) {
#define WR 1  // weights resident in registers (PairCfg::WRES)
#define X(c, ks, bn, taps, md, waves, nwbuf, wres, wm) \
  make_pair_launch<PairCfg<c, ks, bn, taps, md, waves, 0, nwbuf, wres, wm>>("resblock_pair_mfma<c" #c ",k" #ks ",bn" #bn ",t" #taps ">"),
  static const PairLaunch table[] = {
      EVMI_PAIR_TABLE(X)
      // C = 128: chunked variant (64-channel operand chunks, 2 x 4 waves of 64 x 64).  Measured on MI355X
      // (B=32, T=49152): k3 0.49 ms fused vs 0.56 ms as two conv_tc launches; k7 / k11 are MFMA/LDS-bound
      // either way and 3-4 % slower fused (0.86 vs 0.83, 1.19 vs 1.14 ms), so only k3 is routed here.
      make_pair_chunked_launch<PairChunkedCfg<128, 64, 3, 256, 5, 2, 4>>("resblock_pair_mfma<c128,k3,bn256,kc64>"),
  };
#undef X
#undef WR
  *n = (int)(sizeof(table) / sizeof(table[0]));
  return table;
}

const PairLaunch* find_resblock_pair(int c, int ks, int dil) {
  // A/B switch: EVMI_PAIR_C128=0 routes the 128-channel k = 3 pairs to two LDS-DMA convolution launches instead
  static const bool c128_pairs = env_int("EVMI_PAIR_C128", 1) != 0;
  if (c >= 128 && !c128_pairs) return nullptr;
  int n = 0;
  const PairLaunch* t = pair_table(&n);
  for (int i = 0; i < n; ++i)
    if (t[i].c == c && t[i].ks == ks && dil <= t[i].max_dil) return &t[i];
  return nullptr;
}

void relayout_resblock_pair(const float* w, int c, int ks, int kc, uint16_t* dst) {
  for (int mo = 0; mo < c; ++mo)
    for (int ci = 0; ci < c; ++ci)
      for (int jt = 0; jt < ks; ++jt)
        dst[((((size_t)(ci / kc)) * ks + jt) * c + mo) * kc + ci % kc] = f32_to_bf16_bits(w[((size_t)mo * c + ci) * ks + jt]);
}

// Persistent grid of the fused kernels: wg_per_cu workgroups per CU (LDS-bound residency), a multiple of 8 so every XCD gets the same
// number of workgroups (the kernels' tile walk relies on it), and no more than the tiles need
static int persistent_grid(int n_cu, int wg_per_cu, int n_tiles) {
  const int grid = ((n_cu > 0 ? n_cu : 256) * wg_per_cu + 7) / 8 * 8;
  const int needed = (n_tiles + 7) / 8 * 8;
  return grid > needed ? needed : grid;
}

int launch_resblock_pair(const PairLaunch* L, PairArgs a, int B, int n_cu, hipStream_t stream) {
  a.tiles_per_item = (a.T + L->tt - 1) / L->tt;
  a.n_tiles = a.tiles_per_item * B;
  const int grid = persistent_grid(n_cu, L->wg_per_cu, a.n_tiles);
  if (int rc = launch_with_lds(a.lens.frames ? L->kernel_ragged : L->kernel, dim3(grid), dim3(L->threads), L->lds_bytes, stream, a)) return rc;
  EVMI_LAUNCH_CHECK(L->name);
  return EVMI_OK;
}

// ---- whole branches (resblock_branch_kernel.h) ------------------------------------------------------------------------------------------
//                    C  KS  BN  TAPS WAVES NWBUF
// Only where the pair kernels are bound by the residual stream's round trips and the branch's halo stays small: k = 3 and k = 7 at 32
// channels, k = 3 at 64 (k = 11 recomputes 23 % of every tile and is MFMA-bound as pairs already; 64 channels x k = 7 does not fit).
static const BranchLaunch* branch_table(int* n) {
  static const BranchLaunch table[] = {
      make_branch_launch<BranchCfg<32, 3, 512, 3, 16, 2>>("resblock_branch_mfma<c32,k3,bn512>"),
      make_branch_launch<BranchCfg<32, 7, 512, 7, 16, 1>>("resblock_branch_mfma<c32,k7,bn512>"),
      make_branch_launch<BranchCfg<64, 3, 256, 2, 8, 2>>("resblock_branch_mfma<c64,k3,bn256>"),
  };
  *n = (int)(sizeof(table) / sizeof(table[0]));
  return table;
}

// valid rows per tile of a branch with these dilations, or 0 when a convolution would read past the LDS tiles
static int branch_valid_rows(const BranchLaunch& L, int np, const int* dil) {
  const int H = (L.ks - 1) / 2;
  if (np != 3 || dil[0] < 1 || L.bn + 2 * dil[0] * H > L.rb) return 0;
  int m = 0;
  for (int p = 0; p < np; ++p) {
    const int h1 = dil[p] * H;
    if (dil[p] < 1 || m + 2 * h1 + L.bn > L.rb || m + h1 + L.bn + 2 * H > L.rb) return 0;
    m += h1 + H;
  }
  const int tt = L.bn + 2 * dil[0] * H - 2 * m;
  return tt > 0 ? tt : 0;
}

const BranchLaunch* find_resblock_branch(int c, int ks, int np, const int* dil) {
  // A/B switch: EVMI_BRANCH=0 keeps the pair kernels (same bits: tests/test_gpu_generator.py compares the two)
  static const bool enabled = env_int("EVMI_BRANCH", 1) != 0;
  if (!enabled) return nullptr;
  int n = 0;
  const BranchLaunch* t = branch_table(&n);
  for (int i = 0; i < n; ++i)
    if (t[i].c == c && t[i].ks == ks && 4 * branch_valid_rows(t[i], np, dil) >= 3 * t[i].bn) return &t[i];  // (a halo above 25 % does not pay)
  return nullptr;
}

int launch_resblock_branch(const BranchLaunch* L, BranchArgs a, int B, int n_cu, hipStream_t stream) {
  a.tt = branch_valid_rows(*L, a.np, a.dil);
  if (a.tt <= 0) return fail(EVMI_ERR_UNSUPPORTED, "resblock_branch: dilations beyond the LDS tiles");
  a.tiles_per_item = (a.T + a.tt - 1) / a.tt;
  a.n_tiles = a.tiles_per_item * B;
  const int grid = persistent_grid(n_cu, 1, a.n_tiles);
  if (int rc = launch_with_lds(a.lens.frames ? L->kernel_ragged : L->kernel, dim3(grid), dim3(L->threads), L->lds_bytes, stream, a)) return rc;
  EVMI_LAUNCH_CHECK(L->name);
  return EVMI_OK;
}

}  // namespace evmi

// ---- one pair, one branch alone (include/evmi.h) -------------------------------------------------------------------------------------------
using namespace evmi;

namespace {

// n_cu of the entry points: 0 = the current device's compute units, a positive value as given
int resolve_n_cu(int n_cu, int* out) {
  if (n_cu > 0) { *out = n_cu; return EVMI_OK; }
  int dev = 0, cu = 0;
  EVMI_HIP_CHECK(hipGetDevice(&dev));
  EVMI_HIP_CHECK(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
  *out = cu > 0 ? cu : 256;
  return EVMI_OK;
}

// what both entry points refuse before any launch
int fused_refusal(const char* who, const void* x, const void* out, int B, int T, int C, int n_cu) {
  if (B <= 0 || T <= 0 || n_cu < 0) return fail(EVMI_ERR_INVALID_ARG, std::string(who) + ": B and T must be positive, n_cu >= 0");
  if ((long long)T * C >= (1LL << 30)) return fail(EVMI_ERR_UNSUPPORTED, std::string(who) + ": an item of 2^30 elements or more");
  const char* xb = static_cast<const char*>(x);
  const char* ob = static_cast<const char*>(out);
  const long long bytes = 2LL * B * T * C;
  if (xb < ob + bytes && ob < xb + bytes) return fail(EVMI_ERR_INVALID_ARG, std::string(who) + ": x and out overlap (a tile reads the halo rows of its neighbours)");
  return EVMI_OK;
}

}  // namespace

extern "C" {

int evmi_resblock_pair_plan(int C, int ks, int dil, int* tt, int* bn, int* kc, long long* weight_elems) {
  const PairLaunch* L = (C > 0 && ks > 0 && dil >= 1) ? find_resblock_pair(C, ks, dil) : nullptr;
  if (tt) *tt = L ? L->tt : 0;
  if (bn) *bn = L ? L->bn : 0;
  if (kc) *kc = L ? L->kc : 0;
  if (weight_elems) *weight_elems = L ? (long long)C * C * ks : 0;
  return L ? 1 : 0;
}

int evmi_resblock_branch_plan(int C, int ks, int np, const int* dil, int* tt, int* bn) {
  const BranchLaunch* L = (C > 0 && ks > 0 && dil) ? find_resblock_branch(C, ks, np, dil) : nullptr;
  if (tt) *tt = L ? branch_valid_rows(*L, np, dil) : 0;
  if (bn) *bn = L ? L->bn : 0;
  return L ? 1 : 0;
}

int evmi_resblock_pair_relayout_f32(const float* w_host, void* dst_bf16_host, int C, int ks, int kc) {
  if (!w_host || !dst_bf16_host) return fail(EVMI_ERR_INVALID_ARG, "resblock_pair_relayout: null pointer");
  if (C <= 0 || ks <= 0 || kc <= 0 || C % kc) return fail(EVMI_ERR_INVALID_ARG, "resblock_pair_relayout: kc must divide C");
  relayout_resblock_pair(w_host, C, ks, kc, static_cast<uint16_t*>(dst_bf16_host));
  return EVMI_OK;
}

int evmi_resblock_pair_bf16(const void* x, const void* w1_laid, const float* b1_dev, const void* w2_laid, const float* b2_dev, void* out, int B,
                            int T, int C, int ks, int dil, float slope, float post_slope, float out_scale, int accumulate, int n_cu, void* stream) {
  if (!x || !w1_laid || !b1_dev || !w2_laid || !b2_dev || !out) return fail(EVMI_ERR_INVALID_ARG, "resblock_pair: null pointer");
  const PairLaunch* L = (C > 0 && ks > 0 && dil >= 1) ? find_resblock_pair(C, ks, dil) : nullptr;
  if (!L) return fail(EVMI_ERR_UNSUPPORTED, "resblock_pair: no fused kernel for c=" + std::to_string(C) + " k=" + std::to_string(ks) + " dil=" + std::to_string(dil));
  if (int rc = fused_refusal("resblock_pair", x, out, B, T, C, n_cu)) return rc;
  if (int rc = resolve_n_cu(n_cu, &n_cu)) return rc;
  PairArgs pa;
  pa.x = reinterpret_cast<const bf16_t*>(x);
  pa.w1 = reinterpret_cast<const bf16_t*>(w1_laid);
  pa.w2 = reinterpret_cast<const bf16_t*>(w2_laid);
  pa.b1 = b1_dev;
  pa.b2 = b2_dev;
  pa.out = reinterpret_cast<bf16_t*>(out);
  pa.T = T;
  pa.dil1 = dil;
  pa.slope = slope;
  pa.post_slope = post_slope;
  pa.out_scale = out_scale;
  pa.accumulate = accumulate ? 1 : 0;
  pa.timeline = nullptr;
  return launch_resblock_pair(L, pa, B, n_cu, (hipStream_t)stream);
}

int evmi_resblock_branch_bf16(const void* x, const void* const* w_laid, const float* const* bias_dev, void* out, int B, int T, int C, int ks, int np,
                              const int* dil, float slope, float post_slope, float out_scale, int accumulate, int n_cu, void* stream) {
  if (!x || !w_laid || !bias_dev || !out || !dil) return fail(EVMI_ERR_INVALID_ARG, "resblock_branch: null pointer");
  const BranchLaunch* L = (C > 0 && ks > 0) ? find_resblock_branch(C, ks, np, dil) : nullptr;
  if (!L) return fail(EVMI_ERR_UNSUPPORTED, "resblock_branch: no fused kernel for c=" + std::to_string(C) + " k=" + std::to_string(ks) + " np=" + std::to_string(np) + " with these dilations");
  for (int i = 0; i < 2 * np; ++i)
    if (!w_laid[i] || !bias_dev[i]) return fail(EVMI_ERR_INVALID_ARG, "resblock_branch: null pointer");
  if (int rc = fused_refusal("resblock_branch", x, out, B, T, C, n_cu)) return rc;
  if (int rc = resolve_n_cu(n_cu, &n_cu)) return rc;
  BranchArgs ba;
  ba.x = reinterpret_cast<const bf16_t*>(x);
  ba.out = reinterpret_cast<bf16_t*>(out);
  for (int i = 0; i < 6; ++i) {
    ba.w[i] = reinterpret_cast<const bf16_t*>(w_laid[i]);
    ba.b[i] = bias_dev[i];
  }
  for (int p = 0; p < 3; ++p) ba.dil[p] = dil[p];
  ba.T = T;
  ba.np = np;
  ba.slope = slope;
  ba.post_slope = post_slope;
  ba.out_scale = out_scale;
  ba.accumulate = accumulate ? 1 : 0;
  return launch_resblock_branch(L, ba, B, n_cu, (hipStream_t)stream);
}

}  // extern "C"
