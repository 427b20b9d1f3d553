// The generic-shape bf16 MFMA convolution: the contract of conv_tc_mfma.h (ConvTcArgs, unchanged) with c_in, c_out, ks and dil as
// RUN-TIME values.  The specialised tables of conv_tc_mfma.hip stay the fast path for the shapes they hold; this kernel takes
// every shape inside the limits below, so that a schema-valid generator never meets "no MFMA instantiation".
//
//   limits:  c_in, c_out multiples of 8 (16-byte channel vectors);  ks >= 1;  dil >= 1;  (ks - 1) * dil <= kGenericMaxHalo rows
//   tile:    256 rows x 64 output channels per workgroup of four waves; wave w owns rows [64 w, 64 w + 64) as 4 x 4 tiles of
//            v_mfma_f32_16x16x32_bf16 (mfma16_layout.h: weights are the A operand, activation rows the B operand)
//   K order: per output element (32-channel chunk, tap, channel): fixed by the shape alone, not by the tile position or the batch
//   weights: [m-tile of 64][chunk of 32][tap][64][32] bf16, ZERO-padded in both channel directions (conv_generic_weight_index):
//            the kernel reads whole tiles without guards; the activation tile's channel tail is zero-filled in LDS
#pragma once

#include "conv_tc_mfma.h"

namespace evmi {

constexpr int kGenericBM = 64, kGenericBN = 256, kGenericKC = 32, kGenericMaxHalo = 256;

// nullptr when the kernel takes the shape, else the reason (a static string)
const char* conv_generic_refusal(int c_in, int c_out, int ks, int dil);
// bf16 elements of the weight image (padding included)
inline long long conv_generic_weight_elems(int c_in, int c_out, int ks) {
  const long long mt = (c_out + kGenericBM - 1) / kGenericBM, nch = (c_in + kGenericKC - 1) / kGenericKC;
  return mt * nch * ks * kGenericBM * kGenericKC;
}
// position of w[m][c][j] (output channel, input channel, tap) in the image
#if defined(__HIPCC__)
__host__ __device__
#endif
inline long long conv_generic_weight_index(int c_in, int ks, int m, int j, int c) {
  const long long nch = (c_in + kGenericKC - 1) / kGenericKC;
  return ((((long long)(m / kGenericBM) * nch + c / kGenericKC) * ks + j) * kGenericBM + m % kGenericBM) * kGenericKC + c % kGenericKC;
}
// a.x rows hold c_in channels; grid (row tiles, B, m-tiles)
int launch_conv_generic(const ConvTcArgs& a, int c_in, int ks, int B, hipStream_t stream);

}  // namespace evmi
