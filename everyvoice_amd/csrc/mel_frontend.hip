// STFT -> magnitude -> mel -> log front-end of the reference's default "mel-librosa" spectrogram
// (everyvoice/utils/heavy.py:69-100 and :39-40), one kernel, fp32 throughout.
//
//   frames[f][k] = audio_reflect_padded[f*hop + k] * hann[k]          (center=True, pad_mode="reflect")
//   re/im[f][b]  = sum_k frames[f][k] * cos/sin(2*pi*b*k/n_fft)        b in [0, n_fft/2]
//   mag          = sqrt(re^2 + im^2 + 1e-9)
//   mel[m][f]    = sum_b basis[m][b] * mag[f][b]                        (librosa Slaney basis, given by the host)
//   out          = log(max(mel, 1e-5))                                 (optional)
//
// The DFT is a GEMM [32 frames x n_fft] x [n_fft x 2*(n_fft/2+1)] on the fp32-input matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32 fmaf chains, 157 TFLOP/s class) against a window-folded basis
// held in HBM/L2 (n_fft=1024: 4.2 MB).  The frame matrix is never materialised: the padded audio
// segment of a 32-frame block sits once in LDS, skewed by one word per hop when the hop is even (index
// s + s/hop) and not at all when it is odd, so the 32 lanes of an A-fragment read are always an odd
// number of words apart (hop + 1 or hop) and hit 32 distinct banks.
//
// A window shorter than n_fft sits centred in it (torch.stft): basis rows outside [left, left + win) are
// exactly zero, so the k-loop runs over [k0, k1) only (left rounded down / left + win rounded up to even:
// the MFMA takes two k per step) and only the samples that loop reads are staged.  A dropped product is
// a * 0 added to a finite accumulator: the result equals the full loop's bit for bit.
#include "common.h"
#include "mel_frontend.h"

namespace evmi {

constexpr int MEL_FRAMES = 32;   // frames per workgroup (one MFMA M tile)
constexpr int MEL_THREADS = 512;

__device__ __forceinline__ int reflect_index(int i, int n) {
  // torch "reflect" padding (no edge repeat); valid for |overshoot| < n
  if (i < 0) i = -i;
  if (i >= n) i = 2 * (n - 1) - i;
  return i;
}

// basis_ri: [n_fft][2*NB] fp32, column 2b = hann[k]*cos(2 pi b k / n_fft), column 2b+1 = -hann[k]*sin(...)
//           (NB = n_fft/2 + 1 padded up to a multiple of 16 -> 2*NB multiple of 32, extra columns zero)
// melb:     [n_mels][n_bins] fp32
// out:      [B][n_mels][n_frames] fp32 (torch layout)      energy: [B][n_frames] or nullptr
// The bins are processed in `chunk_tiles` column tiles (16 bins each) at a time so that the magnitude tile fits the LDS next to
// the audio segment at n_fft = 2048 (BASELINE config 5: 44.1 kHz, hop 512); the mel accumulators live in registers across the
// chunks and walk the bins in ascending order whatever the chunking, so the result does not depend on it.
constexpr int MEL_ROWS_PER_THREAD = 8;  // n_mels <= 16 * 8

// SKEW: 1 for an even hop (index s + s / hop), 0 for an odd one (index s); k0, k1: the even-aligned support of the window
template <int SKEW>
__global__ __launch_bounds__(MEL_THREADS) void mel_frontend_kernel(
    const float* __restrict__ audio, const float* __restrict__ basis_ri, const float* __restrict__ melb,
    float* __restrict__ out, float* __restrict__ energy, float* __restrict__ mag_out, int n_samples_max, int n_frames,
    int n_fft, int hop, int nb_pad, int n_bins, int n_mels, int apply_log, int chunk_tiles, const int* __restrict__ lens,
    int k0, int k1) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int kspan = k1 - k0;
  const int seg = (MEL_FRAMES - 1) * hop + kspan;           // audio samples a block reads: sample s is k0 + s of frame 0
  float* As = reinterpret_cast<float*>(smem);                // skewed: index s + SKEW * (s / hop)
  const int as_words = seg + (SKEW ? seg / hop : 0) + 1;
  float* Ls = As + ((as_words + 3) & ~3);                    // log-mel rows [MEL_FRAMES][n_mels + 1] for the energy reduction
  float* Ms = Ls + ((MEL_FRAMES * (n_mels + 1) + 3) & ~3);   // magnitudes of one bin chunk [MEL_FRAMES][16 * chunk_tiles + 1]
  const int ms_stride = 16 * chunk_tiles + 1;

  const int b = blockIdx.y;
  const int f0 = blockIdx.x * MEL_FRAMES;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // ragged batches: item b holds lens[b] samples of its n_samples_max-long row and reflects at ITS end; frames past its own
  // 1 + lens[b] / hop are computed from whatever follows (finite) and are the caller's to ignore
  const int n_samples = lens ? max(min(lens[b], n_samples_max), n_fft / 2 + 1) : n_samples_max;
  const float* ab = audio + (long long)b * n_samples_max;
  const int pad = n_fft / 2;

  for (int s = tid; s < seg; s += MEL_THREADS) {
    const int g = f0 * hop + k0 + s - pad;  // position in the un-padded signal
    // positions beyond the reflect-padded signal only feed frames >= n_frames (never stored)
    const float v = (g >= -pad && g <= n_samples - 1 + pad) ? ab[reflect_index(g, n_samples)] : 0.f;
    As[SKEW ? s + s / hop : s] = v;
  }
  __syncthreads();

  const int n_col_tiles = (2 * nb_pad) / 32;
  const int i = lane & 31, kh = lane >> 5;
  const int a_base = i * (hop + SKEW);  // (skewed) start of frame i: (i*hop) + (i*hop)/hop
  const int fr = tid & 31, mg = tid >> 5;  // mel projection: thread -> (frame, mel rows mg, mg + 16, ...)
  float macc[MEL_ROWS_PER_THREAD];
#pragma unroll
  for (int j = 0; j < MEL_ROWS_PER_THREAD; ++j) macc[j] = 0.f;

  for (int ct0 = 0; ct0 < n_col_tiles; ct0 += chunk_tiles) {
    const int ct1 = min(ct0 + chunk_tiles, n_col_tiles);
    const int bin0 = ct0 * 16, bin1 = min(ct1 * 16, n_bins);
    // ---- DFT on the fp32 matrix cores: wave w takes column tiles ct0 + w, ct0 + w + 8, ... of the (re, im) basis ------
    for (int ct = ct0 + wave; ct < ct1; ct += MEL_THREADS / 64) {
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.f;
      const int ld = 2 * nb_pad;
      const float* bcol = basis_ri + (long long)k0 * ld + ct * 32 + i;  // column of this lane, from basis row k0
#pragma unroll 8
      for (int k = 0; k < kspan; k += 2) {
        const int kk = k + kh;
        // frame i, sample k0 + kk: (skewed) index a_base + kk + kk / hop  (the window is folded into the basis)
        const float av = As[SKEW ? a_base + kk + kk / hop : a_base + kk];
        const float bv = bcol[(long long)kk * ld];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
      }
      // D layout: lane holds column j = lane&31 (even = re, odd = im of bin ct*16 + j/2) for frames
      // (r&3) + 8*(r>>2) + 4*(lane>>5)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const float sq = acc[r] * acc[r];
        const float other = __shfl_xor(sq, 1, 64);
        const int frame = (r & 3) + 8 * (r >> 2) + 4 * kh;
        const int bin = ct * 16 + (i >> 1);
        if (!(i & 1) && bin < n_bins) Ms[frame * ms_stride + bin - bin0] = sqrtf(sq + other + 1e-9f);
      }
    }
    __syncthreads();

    if (mag_out) {  // optional linear-magnitude output [B][n_bins][n_frames]
      for (int v = tid; v < MEL_FRAMES * (bin1 - bin0); v += MEL_THREADS) {
        const int bin = bin0 + v / MEL_FRAMES, f = v % MEL_FRAMES;
        if (f0 + f < n_frames) mag_out[((long long)b * n_bins + bin) * n_frames + f0 + f] = Ms[f * ms_stride + bin - bin0];
      }
    }
    // ---- mel projection, this chunk's bins (ascending-bin fmaf chain continued from the previous chunk) ----------
    {
      const float* mrow = Ms + fr * ms_stride - bin0;
      const float* wbase = melb + (long long)mg * n_bins;
      const long long wstep = (long long)(MEL_THREADS / 32) * n_bins;
      const int rows = (n_mels - mg + MEL_THREADS / 32 - 1) / (MEL_THREADS / 32);  // mel rows of this thread
      for (int bin = bin0; bin < bin1; ++bin) {
        const float mv = mrow[bin];
#pragma unroll
        for (int j = 0; j < MEL_ROWS_PER_THREAD; ++j)
          if (j < rows) macc[j] = fmaf(wbase[j * wstep + bin], mv, macc[j]);
      }
    }
    __syncthreads();  // the next chunk overwrites Ms
  }
#pragma unroll
  for (int j = 0; j < MEL_ROWS_PER_THREAD; ++j) {
    const int m = mg + j * (MEL_THREADS / 32);
    if (m < n_mels) {
      float acc = macc[j];
      if (apply_log) acc = logf(fmaxf(acc, 1e-5f));
      if (f0 + fr < n_frames) out[((long long)b * n_mels + m) * n_frames + f0 + fr] = acc;
      Ls[fr * (n_mels + 1) + m] = acc;
    }
  }
  if (energy) {  // energy[f] = || mel[:, f] ||_2 over the (log-)mel bins (everyvoice/preprocessor/preprocessor.py:302-309)
    __syncthreads();
    if (tid < MEL_FRAMES && f0 + tid < n_frames) {
      float e = 0.f;
      for (int m = 0; m < n_mels; ++m) e = fmaf(Ls[tid * (n_mels + 1) + m], Ls[tid * (n_mels + 1) + m], e);
      energy[(long long)b * n_frames + f0 + tid] = sqrtf(e);
    }
  }
}

// The geometry of one launch, host arithmetic only: what evmi_mel_spectrogram_plan reports and what the launch uses.
int mel_plan(const char* who, int n_fft, int win, int hop, int n_mels, int nb_pad, MelPlan* p) {
  const std::string w(who);
  if (n_fft <= 0 || n_fft % 2) return fail(EVMI_ERR_UNSUPPORTED, w + ": n_fft = " + std::to_string(n_fft) + " must be even and positive");
  if (win < 1 || win > n_fft)
    return fail(EVMI_ERR_INVALID_ARG, w + ": win_length = " + std::to_string(win) + " outside [1, n_fft = " + std::to_string(n_fft) + "]");
  if (hop < 1 || hop > n_fft)
    return fail(EVMI_ERR_INVALID_ARG, w + ": hop = " + std::to_string(hop) + " outside [1, n_fft = " + std::to_string(n_fft) + "]");
  if (n_mels < 1) return fail(EVMI_ERR_INVALID_ARG, w + ": n_mels = " + std::to_string(n_mels) + " must be positive");
  if (n_mels > MEL_ROWS_PER_THREAD * (MEL_THREADS / 32)) return fail(EVMI_ERR_UNSUPPORTED, w + ": n_mels = " + std::to_string(n_mels) + " > 128");
  if (nb_pad % 16 || nb_pad < n_fft / 2 + 1) return fail(EVMI_ERR_INVALID_ARG, w + ": bad shape (n_bins_padded)");
  const int left = (n_fft - win) / 2;
  p->k0 = left & ~1;
  p->k1 = (left + win + 1) & ~1;  // <= n_fft: n_fft is even
  p->skew = (hop & 1) ? 0 : 1;    // frame rows hop + skew words apart: always odd
  p->frame_stride = hop + p->skew;
  const long long seg = (long long)(MEL_FRAMES - 1) * hop + (p->k1 - p->k0);
  const long long as_words = (seg + (p->skew ? seg / hop : 0) + 1 + 3) & ~3LL;
  const long long ls_words = (MEL_FRAMES * (n_mels + 1) + 3) & ~3;
  const long long budget = 160 * 1024 / sizeof(float);
  const int n_col_tiles = (2 * nb_pad) / 32;
  if (as_words + ls_words + MEL_FRAMES * 17 > budget)
    return fail(EVMI_ERR_UNSUPPORTED, w + ": n_fft = " + std::to_string(n_fft) + ", win_length = " + std::to_string(win) + ", hop = " +
                                          std::to_string(hop) + ": the audio tile of 32 frames does not fit the 160 KB LDS budget");
  // the largest bin chunk that fits beside the audio segment, then the chunks evened out
  int max_tiles = (int)(((budget - as_words - ls_words) / MEL_FRAMES - 1) / 16);
  if (max_tiles > n_col_tiles) max_tiles = n_col_tiles;
  const int n_chunks = (n_col_tiles + max_tiles - 1) / max_tiles;
  p->chunk_tiles = (n_col_tiles + n_chunks - 1) / n_chunks;
  p->lds_bytes = (as_words + ls_words + (long long)MEL_FRAMES * (16 * p->chunk_tiles + 1)) * (long long)sizeof(float);
  return EVMI_OK;
}

int launch_mel_frontend(const char* who, const float* audio, const float* basis_ri, const float* melb, float* out, float* energy,
                        float* mag_out, int B, int n_samples, int n_fft, int win, int hop, int nb_pad, int n_mels, int apply_log,
                        hipStream_t s, const int* lens) {
  MelPlan p;
  if (int rc = mel_plan(who, n_fft, win, hop, n_mels, nb_pad, &p)) return rc;
  if (B <= 0 || n_samples <= 0) return fail(EVMI_ERR_INVALID_ARG, std::string(who) + ": bad shape");
  if (n_samples <= n_fft / 2) return fail(EVMI_ERR_INVALID_ARG, std::string(who) + ": reflect padding needs n_samples > n_fft/2");
  const int n_frames = 1 + n_samples / hop, n_bins = n_fft / 2 + 1;
  dim3 grid((n_frames + MEL_FRAMES - 1) / MEL_FRAMES, B);
  auto kernel = p.skew ? mel_frontend_kernel<1> : mel_frontend_kernel<0>;
  if (int rc = launch_with_lds(kernel, grid, dim3(MEL_THREADS), (size_t)p.lds_bytes, s, audio, basis_ri, melb, out, energy, mag_out, n_samples,
                               n_frames, n_fft, hop, nb_pad, n_bins, n_mels, apply_log, p.chunk_tiles, lens, p.k0, p.k1))
    return rc;
  EVMI_LAUNCH_CHECK("mel_frontend");
  return EVMI_OK;
}

}  // namespace evmi
