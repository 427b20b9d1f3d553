// The generic-size iSTFTNet output head: the contract of istft_head_kernel (istft_head.hip) with the channel count, n_fft and hop as
// RUN-TIME values.  The specialised kernel stays the path of n_fft 16 / hop 4 on 32 / 64 / 128 channels; this one takes everything
// inside the domain below, so that a vocoder the project can train is a vocoder its default precision can run.
//
//   domain:  C a multiple of 8, 8 <= C <= 512;  n_fft even, 4 <= n_fft <= 128;  1 <= hop <= n_fft / 2
//   tile:    F = 64 / 128 / 192 frames per workgroup of four waves (istft_head_frame_tile: a function of n_fft and hop alone);
//            sample t needs frames floor((t + n_fft/2 - n_fft + 1) / hop) .. floor((t + n_fft/2) / hop), so a workgroup whose first
//            sample is a multiple of hop needs lo = (n_fft/2 - 1) / hop frames before its first and lo + 1 after its last hop block:
//            F frames yield hop * (F - 2 lo - 1) samples.  (Where hop divides n_fft/2 that is F - ceil(n_fft / hop) + 1; where it does
//            not, one frame fewer: a hop-aligned block of hop samples then touches ceil(n_fft / hop) + 1 frames.)
//   weights: the zero-padded image of conv_tc_generic.h for (c_in = C, c_out = n_fft + 2, ks = 7), streamed per 64-channel group and
//            32-channel chunk; bias fp32 [n_fft + 2]
#pragma once

#include "conv_tc_generic.h"

namespace evmi {

constexpr int kIstftMinNfft = 4, kIstftMaxNfft = 128, kIstftMaxC = 512, kIstftKs = 7;

inline bool istft_head_nfft_ok(int n_fft) { return n_fft >= kIstftMinNfft && n_fft <= kIstftMaxNfft && n_fft % 2 == 0; }
inline bool istft_head_hop_ok(int n_fft, int hop) { return hop >= 1 && 2 * hop <= n_fft; }
inline bool istft_head_channels_ok(int c) { return c >= 8 && c <= kIstftMaxC && c % 8 == 0; }
// the shapes istft_head_kernel (istft_head.hip) is instantiated for
inline bool istft_head_specialised(int c, int n_fft, int hop) { return n_fft == 16 && hop == 4 && (c == 32 || c == 64 || c == 128); }

inline int istft_head_halo(int n_fft, int hop) { return 2 * ((n_fft / 2 - 1) / hop) + 1; }
// Frames per workgroup: the smallest tile that spends at most half of its frames on the halo; short heads (polar tile of 128 frames
// within 32 KB) start at 128 frames, which halves the weight-image traffic per frame.  192 is the largest the LDS holds at n_fft 128.
inline int istft_head_frame_tile(int n_fft, int hop) {
  const int halo = istft_head_halo(n_fft, hop);
  for (int f = n_fft <= 62 ? 128 : 64; f < 192; f += 64)
    if (f - halo >= f / 2) return f;
  return 192;
}

int launch_istft_head_generic(const bf16_t* x, const bf16_t* w_img, const float* bias, float* wav, int B, int L, int C, int n_fft, int hop,
                              ItemLens lens, hipStream_t s);  // lens: ragged batch (common.h), ItemLens{} = none

}  // namespace evmi
