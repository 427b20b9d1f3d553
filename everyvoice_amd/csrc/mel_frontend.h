// Geometry of the mel front end (csrc/mel_frontend.hip), shared with the C ABI (csrc/api.hip).
#pragma once
#include "common.h"

namespace evmi {

struct MelPlan {
  int k0, k1;         // the DFT k-loop runs over [k0, k1): the even-aligned support of the window inside n_fft
  int skew;           // LDS words added per hop: 1 for an even hop, 0 for an odd one
  int frame_stride;   // hop + skew: words between the rows of consecutive frames (odd)
  int chunk_tiles;    // 16-bin column tiles per chunk of the magnitude tile
  long long lds_bytes;
};

// EVMI_OK, or the refusal of the launch (its code, a message that begins with `who`); no HIP call.
int mel_plan(const char* who, int n_fft, int win, int hop, int n_mels, int nb_pad, MelPlan* p);
int launch_mel_frontend(const char* who, const float* audio, const float* basis_ri, const float* melb, float* out, float* energy,
                        float* mag_out, int B, int n_samples, int n_fft, int win, int hop, int nb_pad, int n_mels, int apply_log,
                        hipStream_t s, const int* lens);

}  // namespace evmi
