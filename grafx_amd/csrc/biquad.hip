// Exact time-domain biquad cascade as a parallel scan (gfx950).
//
// Replaces IIRFilter._process_lfilter / _process_ssm — reference core/iir.py:154-261 — whose upstream
// implementations call torchaudio.functional.lfilter / torchlpc.sample_wise_lpc (neither is installed here):
// K second-order sections applied in series to every row-channel,
//     w[n] = x[n] - a1 w[n-1] - a2 w[n-2],   y[n] = b0 w[n] + b1 w[n-1] + b2 w[n-2]      (a0-normalised)
// with zero initial state (gfx_biquad_cascade_f32) or with every section's (w[-1], w[-2]) given and (w[L-1], w[L-2])
// returned (gfx_biquad_cascade_state_f32: block-wise processing of a long signal).  No FFT, no truncation of the impulse response (the FSM backend aliases it to
// fsm_fir_len taps), 8 B of HBM traffic per channel-sample.
//
// Parallelisation: RL lanes walk TWO row-channels (packed fp32: the two channels of a stereo row, or two neighbouring mono
// rows) in tiles of RL x 8 samples, no barriers and no cross-lane LDS traffic in the time loop.  RL = 64 (one wave per pair,
// 512-sample tiles, the next tile requested ahead) unless there are pairs enough (>= 8192) to fill the chip with RL = 16
// (four pairs per wave, 128-sample tiles): a pair's tiles are a sequential chain, and with few pairs the time is that
// chain's latency.  The recursion is the linear system s[n] = M s[n-1] + (x[n], 0), M = [[-a1, -a2], [1, 0]],
// s = (w[n], w[n-1]):
//   1. each lane runs its 8 samples from a zero state                 -> end state e_t
//   2. Hillis-Steele scan over the 16 lanes of a DPP row with M^(8*2^d), d < 4 -> state at the end of every chunk.  The
//      shifted operands come from DPP row shifts (row_shr:1/2/4/8, zero fill: the lanes a step does not reach add zero),
//      i.e. from the vector ALU's own lane crossbar.  RL = 64: two more steps carry the rows' totals across (row_bcast:15
//      into rows 1 and 3, row_bcast:31 into rows 2 and 3), weighted per lane with M^(8 (l % 16 + 1)) from a 16-entry table.
//      The state entering the tile (the carry) is injected at lane 0 (its end state += M^8 * carry), so the scan delivers
//      every lane's TRUE entering state (one lane below: row_shr:1 / wave_shr:1) and the last lane's total is the next
//      tile's carry (row_ror:1 / v_readlane)
//   3. every lane reruns its 8 samples from that state and applies the numerator.
// The matrix powers are formed in double per (row-channel, section) when the workgroup starts and live in LDS (256 B per
// pair and section, + 512 B for RL = 64).  Rounds 2-3 scanned over the 64 lanes with __shfl_up = ds_bpermute_b32: 16 trips
// through the LDS crossbar per section and tile of a row-channel, ~9 cycles each of the CU's ONE LDS unit -- that, not
// arithmetic or HBM, was the kernel's time (K = 6 at 8192 x 2 x 131072: 7.3 ms = 2.3 TB/s; two row-channels per wave in
// packed fp32 alone changed nothing).
//
// ssm_quirk: upstream's "ssm" backend drives the recursive part of every section with the ORIGINAL input
// instead of the previous section's output (core/iir.py:226-246 index `input_signal`, not `x`); for K = 1
// the two backends agree, for K > 1 this flag reproduces what "ssm" actually returns.
#include "biquad_common.hpp"

namespace gfx {

struct BqArgs {
    gfx_rowmap_t xmap, ymap;
    int64_t L, total;
    int Cin, Cf, Cout, K, quirk, vec;
};

#define BQ_STATE 0
#include "biquad_kernel.hpp"   // biquad_cascade_kernel
#undef BQ_STATE
#define BQ_STATE 1
#include "biquad_kernel.hpp"   // biquad_cascade_state_kernel
#undef BQ_STATE

static inline size_t bq_lds_bytes(int64_t K, int RL) {
    return (size_t)(BQ_T / RL) * K * sizeof(SecConst) + (RL == 64 ? (size_t)K * 16 * 4 * sizeof(f2) : 0);
}

template <bool STATE>
static int bq_launch(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* Bs, const float* As,
                     const float* zi, float* zf, int64_t R, int64_t C_in, int64_t C_f, int64_t K, int64_t L, int ssm_quirk,
                     void* stream) {
    if (!x || !y || !Bs || !As || R <= 0 || L <= 0 || K < 1 || K > BQ_MAX_K) return GFX_EINVAL;
    if (C_in < 1 || C_f < 1 || (C_in != C_f && C_in != 1 && C_f != 1)) return GFX_EINVAL;
    if (xmap.inner <= 0 || ymap.inner <= 0 || R > 0x7fffffffLL) return GFX_EINVAL;
    BqArgs a;
    a.xmap = xmap; a.ymap = ymap; a.L = L;
    a.Cin = (int)C_in; a.Cf = (int)C_f; a.Cout = (int)(C_in > C_f ? C_in : C_f);
    a.K = (int)K; a.quirk = ssm_quirk ? 1 : 0;
    a.vec = aligned16(x) && aligned16(y) && map_vec(xmap) && map_vec(ymap);
    a.total = R * a.Cout;
    const int64_t pairs = (a.total + 1) / 2;
    // sixteen lanes per pair where such waves fill the chip, else the whole wave
    const bool narrow = pairs >= 8192;
    const int RL = narrow ? 16 : 64;
    const int64_t blocks = (pairs + BQ_T / RL - 1) / (BQ_T / RL);
    if (blocks > 0x7fffffffLL) return GFX_EINVAL;
    const size_t lds = bq_lds_bytes(K, RL);
    if constexpr (STATE) {
        auto kern = narrow ? biquad_cascade_state_kernel<16, false> : biquad_cascade_state_kernel<64, true>;
        if (allow_lds(kern, lds) != GFX_OK) return GFX_ELAUNCH;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(BQ_T), lds, (hipStream_t)stream, x, y, Bs, As, a, zi, zf);
    } else {
        auto kern = narrow ? biquad_cascade_kernel<16, false> : biquad_cascade_kernel<64, true>;
        if (allow_lds(kern, lds) != GFX_OK) return GFX_ELAUNCH;
        hipLaunchKernelGGL(kern, dim3((unsigned)blocks), dim3(BQ_T), lds, (hipStream_t)stream, x, y, Bs, As, a);
    }
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_biquad_cascade_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* Bs,
                           const float* As, int64_t R, int64_t C_in, int64_t C_f, int64_t K, int64_t L, int ssm_quirk,
                           void* stream) {
    return bq_launch<false>(x, xmap, y, ymap, Bs, As, nullptr, nullptr, R, C_in, C_f, K, L, ssm_quirk, stream);
}

int gfx_biquad_cascade_state_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* Bs,
                                 const float* As, const float* zi, float* zf, int64_t R, int64_t C_in, int64_t C_f,
                                 int64_t K, int64_t L, int ssm_quirk, void* stream) {
    return bq_launch<true>(x, xmap, y, ymap, Bs, As, zi, zf, R, C_in, C_f, K, L, ssm_quirk, stream);
}

}  // extern "C"
