// What the forward (stft_ir.hip) and the backward (stft_ir_bwd.hip) of the STFT-masked-noise impulse response share: the
// kernels' argument block and its builder, the layout of the basis buffer that gfx_istft_basis_f32 fills, the LDS pitches
// of the FFT-384 kernels and softplus as both evaluate it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace gfx {

using cxf = float __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float softplus_t(float v) { return v > 20.0f ? v : log1pf(expf(v)); }

// (a by-value kernel argument: the layout fixes every kernel's argument offsets, unused fields included)
struct IstftArgs {
    int64_t R;
    int n_fft, hop, T, K, kpad;   // K = n_fft/2+1 bins, T frames
    int64_t ir_len;
    int64_t nstride;              // floats between the noise spectra of consecutive rows (0: one spectrum shared by all)
};

__host__ __device__ inline int64_t kpad_of(int64_t n_fft) { return ((2 * (n_fft / 2 + 1)) + 3) / 4 * 4; }
__host__ __device__ inline int64_t half_cols(int64_t n_fft) { return ((n_fft / 2 + 1) + 15) / 16 * 16; }

inline IstftArgs istft_args(int64_t R, int64_t n_fft, int64_t hop, int64_t num_frames, int64_t ir_len, int64_t noise_rows) {
    IstftArgs a;
    a.R = R;
    a.n_fft = (int)n_fft;
    a.hop = (int)hop;
    a.T = (int)num_frames;
    a.K = (int)(n_fft / 2 + 1);
    a.kpad = (int)kpad_of(n_fft);
    a.ir_len = ir_len;
    a.nstride = noise_rows == 1 ? 0 : 2 * (n_fft / 2 + 1) * num_frames * 2;
    return a;
}

// The basis buffer, in floats: the full basis (kpad, n_fft) at 0, the half basis (K, 2, half_cols) behind it, then the
// FFT tables (2 n_fft floats).
inline int64_t basis_half_off(int64_t n_fft) { return kpad_of(n_fft) * n_fft; }
inline int64_t basis_tables_off(int64_t n_fft) { return basis_half_off(n_fft) + (n_fft / 2 + 1) * 2 * half_cols(n_fft); }
inline int64_t basis_total(int64_t n_fft) { return basis_tables_off(n_fft) + 2 * n_fft; }

// LN lanes work on a frame (LN = 8: 192 = 8 x 24, LN = 16: 192 = 16 x 12) and a wave on 64 / LN frames, each lane touching
// 8-byte (spectrum) or 2 x 4-byte (overlap-add image) entries at l, l + LN, ...: a frame pitch of 2 LN banks (mod 64) puts
// the dwords of neighbouring frames' lanes side by side, so that a wave's access takes the four cycles its 512 bytes need
// anyway.  With the natural pitches (193 entries / 192 floats) lanes of neighbouring frames met in the same banks, up to
// eight deep.
template <int LN> constexpr int f3_pitch() { return LN == 8 ? 200 : 208; }       // 8-byte entries per frame: 2 LN dwords mod 64
template <int LN> constexpr int f3_ola_pitch() { return LN == 8 ? 208 : 224; }   // floats per block of 192 samples: 2 LN mod 64

}  // namespace gfx
