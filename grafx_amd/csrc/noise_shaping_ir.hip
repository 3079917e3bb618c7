// FilteredNoiseShapingReverb: impulse-response synthesis (reverb.py:343-366) and its backward.
//   ir[r,c,t] = sum_k noise[c,k,t] * gain[r,c,k] * (exp(t*d) - fg * exp(t*f))
//   d  = sigmoid(log_decay)*(max_decay - min_decay) + min_decay
//   f  = sigmoid(log_fade_in)*(d - min_decay) + min_decay,  fg = sigmoid(z_fade_in_gain)   (fade-in optional)
// and `gain` is the raw log_gain parameter, as upstream multiplies by it un-exponentiated (reverb.py:361).
// The reference materialises the (R,C,K,ir_len) envelope; here the K band terms are summed in registers.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/grafx_amd.h"

namespace gfx {

constexpr int NS_MAX_K = 64;

__global__ __launch_bounds__(256) void noise_shaping_ir_kernel(const float* __restrict__ noise, int64_t noise_stride,
                                                               const float* __restrict__ log_decay,
                                                               const float* __restrict__ gain,
                                                               const float* __restrict__ log_fade_in,
                                                               const float* __restrict__ z_fade_gain,
                                                               float* __restrict__ ir, int C, int K, int64_t ir_len,
                                                               float min_decay, float max_decay) {
    __shared__ float sd[NS_MAX_K], sg[NS_MAX_K], sf[NS_MAX_K], sfg[NS_MAX_K];
    const int64_t rc = blockIdx.y;
    const int c = (int)(rc % C);
    if (threadIdx.x < K) {
        const int64_t i = rc * K + threadIdx.x;
        const float d = (max_decay - min_decay) / (1.0f + expf(-log_decay[i])) + min_decay;
        sd[threadIdx.x] = d;
        sg[threadIdx.x] = gain[i];
        if (log_fade_in) {
            sf[threadIdx.x] = (d - min_decay) / (1.0f + expf(-log_fade_in[i])) + min_decay;
            sfg[threadIdx.x] = 1.0f / (1.0f + expf(-z_fade_gain[i]));
        }
    }
    __syncthreads();
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ir_len) return;
    const float ft = (float)t;
    const float* nz = noise + (int64_t)c * K * noise_stride + t;
    float acc = 0.0f;
    for (int k = 0; k < K; ++k) {
        float env = expf(ft * sd[k]);
        if (log_fade_in) env -= expf(ft * sf[k]) * sfg[k];
        acc += nz[k * noise_stride] * (env * sg[k]);
    }
    ir[rc * ir_len + t] = acc;
}

// ---- backward of noise_shaping_ir_kernel (+ the normalisation): dL/d(parameters) from dL/dh -------------------------------
// With e_d = exp(t d), e_f = exp(t f), n = noise[c,k,t] and v = dL/d(ir):
//   S0 = sum_t v n e_d,  S1 = sum_t v n t e_d,  F0 = sum_t v n e_f,  F1 = sum_t v n t e_f           per (r, c, k)
//   g_gain = S0 - fg F0,   g_d = gain (S1 - fg sigmoid(log_fade_in) F1)
//   g_log_decay = g_d (max - min) sigmoid'(log_decay),   g_log_fade_in = -gain fg F1 (d - min) sigmoid'(log_fade_in),
//   g_z_fade_in_gain = -gain F0 sigmoid'(z_fade_in_gain).
// Normalised taps h = s ir, s = row_gain: v = s gh - (s^3 / C) <gh, ir>_row ir.  The four sums are linear in v, so they are
// taken against gh and against ir in the same pass that takes the workgroup's share of <gh, ir>, and combined by the
// finishing kernel: no workgroup waits for the row's dot product.
// A workgroup owns NSB_CHUNK consecutive samples of one (r, c): its gh (and ir) samples stay in registers, the loop over
// the K bands reads the noise (C K ir_len floats, shared by all rows: from cache) and needs NS <= 8 accumulators at a time.
// Each sum goes down its 16-lane row by DPP (lane 15 ends with the row's sum, a fixed order), the 16 row sums of the
// workgroup through LDS, and thread (k, sum) adds them in index order and stores one partial per workgroup.  No atomics.
constexpr int NSB_E = 8;                    // samples per thread
constexpr int NSB_CHUNK = 256 * NSB_E;      // samples per workgroup
__host__ __device__ inline int64_t nsb_stride(int64_t K) { return 8 * K + 1; }   // floats per workgroup in the workspace

template <int N>
__device__ __forceinline__ float row_shr(float v) {   // lane i of a 16-lane row <- lane i - N, 0 from before the row
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), 0x110 + N, 0xf, 0xf, true));
}
__device__ __forceinline__ float row16_sum(float v) {  // lane 15 of every row: the sum of the row's 16 lanes
    v += row_shr<1>(v);
    v += row_shr<2>(v);
    v += row_shr<4>(v);
    v += row_shr<8>(v);
    return v;
}

// grid: (chunks of NSB_CHUNK samples, row-channels of this launch).  partial: (row-channel, chunk, 8 K + 1) floats:
// [(4 j + q) K + k], j = 0 against gh, 1 against ir, q = S0, S1, F0, F1; the last float is the chunk's sum of gh ir.
template <bool FADE, bool NORM>
__global__ __launch_bounds__(256) void noise_shaping_ir_bwd_kernel(const float* __restrict__ gh, const float* __restrict__ ir,
                                                                   const float* __restrict__ noise, int64_t noise_stride,
                                                                   const float* __restrict__ log_decay,
                                                                   const float* __restrict__ log_fade_in,
                                                                   float* __restrict__ partial, int C, int K, int64_t ir_len,
                                                                   float min_decay, float max_decay) {
    constexpr int NQ = FADE ? 4 : 2, NS = NORM ? 2 * NQ : NQ;
    extern __shared__ __attribute__((aligned(16))) float nsb_red[];   // [K][NS][16] row sums
    __shared__ float sd[NS_MAX_K], sf[NS_MAX_K], dred[16];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t rc = blockIdx.y;
    const int c = (int)(rc % C);
    if (tid < K) {
        const int64_t i = rc * K + tid;
        const float d = (max_decay - min_decay) / (1.0f + expf(-log_decay[i])) + min_decay;   // as the forward has it
        sd[tid] = d;
        if (FADE) sf[tid] = (d - min_decay) / (1.0f + expf(-log_fade_in[i])) + min_decay;
    }
    const int64_t t0 = (int64_t)blockIdx.x * NSB_CHUNK + tid;
    float g[NSB_E], u[NSB_E], tf[NSB_E];
    float dot = 0.0f;
#pragma unroll
    for (int j = 0; j < NSB_E; ++j) {
        const int64_t t = t0 + 256 * j;
        const bool ok = t < ir_len;
        g[j] = ok ? gh[rc * ir_len + t] : 0.0f;
        u[j] = (NORM && ok) ? ir[rc * ir_len + t] : 0.0f;
        tf[j] = ok ? (float)t : 0.0f;
        if (NORM) dot = fmaf(g[j], u[j], dot);
    }
    const int slot = wave * 4 + (lane >> 4);
    const bool last = (lane & 15) == 15;
    if (NORM) {
        dot = row16_sum(dot);
        if (last) dred[slot] = dot;
    }
    __syncthreads();
    const float* nz = noise + (int64_t)c * K * noise_stride;
    for (int k = 0; k < K; ++k) {
        const float d = sd[k], f = FADE ? sf[k] : 0.0f;
        const float* nk = nz + (int64_t)k * noise_stride;
        float n[NSB_E];
#pragma unroll
        for (int j = 0; j < NSB_E; ++j) {
            const int64_t t = t0 + 256 * j;
            n[j] = t < ir_len ? nk[t] : 0.0f;
        }
        float acc[NS];
#pragma unroll
        for (int s = 0; s < NS; ++s) acc[s] = 0.0f;
#pragma unroll
        for (int j = 0; j < NSB_E; ++j) {
            const float a = n[j] * expf(tf[j] * d), at = a * tf[j];
            acc[0] = fmaf(g[j], a, acc[0]);
            acc[1] = fmaf(g[j], at, acc[1]);
            if (NORM) {
                acc[NQ] = fmaf(u[j], a, acc[NQ]);
                acc[NQ + 1] = fmaf(u[j], at, acc[NQ + 1]);
            }
            if (FADE) {
                const float b = n[j] * expf(tf[j] * f), bt = b * tf[j];
                acc[2] = fmaf(g[j], b, acc[2]);
                acc[3] = fmaf(g[j], bt, acc[3]);
                if (NORM) {
                    acc[NQ + 2] = fmaf(u[j], b, acc[NQ + 2]);
                    acc[NQ + 3] = fmaf(u[j], bt, acc[NQ + 3]);
                }
            }
        }
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            const float v = row16_sum(acc[s]);
            if (last) nsb_red[(k * NS + s) * 16 + slot] = v;
        }
    }
    __syncthreads();
    float* out = partial + (rc * gridDim.x + blockIdx.x) * nsb_stride(K);
    for (int i = tid; i < K * NS; i += 256) {
        const int k = i / NS, s = i - k * NS;
        const float* p = nsb_red + i * 16;
        float v = p[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) v += p[w];
        out[(4 * (s / NQ) + s % NQ) * K + k] = v;
    }
    if (NORM && tid == 0) {
        float v = dred[0];
#pragma unroll
        for (int w = 1; w < 16; ++w) v += dred[w];
        out[8 * K] = v;
    }
}

// The partials of the nchunk workgroups of a row-channel added in double in workgroup order, the normalisation's two terms
// combined, and the chain rule.  grid: row-channels, thread k.  sigmoid'(x) = s (1 - s) with s = 1 / (1 + exp(-x)) in float:
// s is 0 or 1 at a saturated parameter (exp overflows to infinity, 1 / infinity = 0), so the gradient there is 0, not NaN.
__global__ __launch_bounds__(64) void noise_shaping_ir_bwd_finish_kernel(
    const float* __restrict__ partial, const float* __restrict__ row_gain, const float* __restrict__ log_decay,
    const float* __restrict__ gain, const float* __restrict__ log_fade_in, const float* __restrict__ z_fade_gain,
    float* __restrict__ g_log_decay, float* __restrict__ g_gain, float* __restrict__ g_log_fade_in,
    float* __restrict__ g_z_fade_gain, int C, int K, int nchunk, float min_decay, float max_decay) {
    const int k = threadIdx.x;
    if (k >= K) return;
    const int64_t rc = blockIdx.x, r = rc / C, stride = nsb_stride(K);
    const bool fade = log_fade_in != nullptr, norm = row_gain != nullptr;
    double A[4] = {0.0, 0.0, 0.0, 0.0}, B[4] = {0.0, 0.0, 0.0, 0.0};
    for (int ch = 0; ch < nchunk; ++ch) {
        const float* p = partial + (rc * nchunk + ch) * stride;
        for (int q = 0; q < (fade ? 4 : 2); ++q) {
            A[q] += (double)p[q * K + k];
            if (norm) B[q] += (double)p[(4 + q) * K + k];
        }
    }
    if (norm) {
        double dot = 0.0;
        for (int64_t i = r * C * nchunk; i < (r + 1) * C * nchunk; ++i) dot += (double)partial[i * stride + 8 * K];
        const double s = (double)row_gain[r], b = s * s * s * dot / (double)C;
        for (int q = 0; q < 4; ++q) A[q] = s * A[q] - b * B[q];
    }
    const int64_t i = rc * K + k;
    const float sl = 1.0f / (1.0f + expf(-log_decay[i]));
    const float d = (max_decay - min_decay) * sl + min_decay;
    const double gn = (double)gain[i];
    double fg = 0.0, sfi = 0.0;
    if (fade) {
        const float sfl = 1.0f / (1.0f + expf(-log_fade_in[i])), sz = 1.0f / (1.0f + expf(-z_fade_gain[i]));
        fg = (double)sz;
        sfi = (double)sfl;
        if (g_log_fade_in)
            g_log_fade_in[i] = (float)(-gn * fg * A[3] * ((double)d - (double)min_decay) * (double)(sfl * (1.0f - sfl)));
        if (g_z_fade_gain) g_z_fade_gain[i] = (float)(-gn * A[2] * (double)(sz * (1.0f - sz)));
    }
    if (g_gain) g_gain[i] = (float)(A[0] - fg * A[2]);
    if (g_log_decay)
        g_log_decay[i] = (float)(gn * (A[1] - fg * sfi * A[3]) * ((double)max_decay - (double)min_decay) *
                                 (double)(sl * (1.0f - sl)));
}

// The grid.y limit: launch(done, n) for runs of n row-channels starting at `done`, each run on a channel boundary (the
// kernels take the channel as their row index mod C) -- 65535 itself is odd, so whole rows of C channels per launch.
template <class Launch>
inline void for_channel_aligned_rows(int64_t rows, int64_t C, Launch launch) {
    const int64_t step = 65535 / C * C;
    for (int64_t done = 0; done < rows; done += step) launch(done, rows - done < step ? rows - done : step);
}

}  // namespace gfx

extern "C" {

int gfx_noise_shaping_ir_f32(const float* noise, int64_t noise_stride, const float* log_decay, const float* log_gain,
                             const float* log_fade_in, const float* z_fade_in_gain, float* ir, int64_t R, int64_t C,
                             int64_t K, int64_t ir_len, float min_decay, float max_decay, void* stream) {
    if (!noise || !log_decay || !log_gain || !ir || R <= 0 || C <= 0 || K <= 0 || K > gfx::NS_MAX_K || ir_len <= 0)
        return GFX_EINVAL;
    if ((log_fade_in == nullptr) != (z_fade_in_gain == nullptr) || noise_stride < ir_len || R * C > 0x7fffffffLL)
        return GFX_EINVAL;
    if (C > 65535) return GFX_EINVAL;
    gfx::for_channel_aligned_rows(R * C, C, [&](int64_t done, int64_t n) {
        hipLaunchKernelGGL(gfx::noise_shaping_ir_kernel, dim3((unsigned)((ir_len + 255) / 256), (unsigned)n), dim3(256), 0,
                           (hipStream_t)stream, noise, noise_stride, log_decay + done * K, log_gain + done * K,
                           log_fade_in ? log_fade_in + done * K : nullptr,
                           z_fade_in_gain ? z_fade_in_gain + done * K : nullptr, ir + done * ir_len, (int)C, (int)K,
                           ir_len, min_decay, max_decay);
    });
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

size_t gfx_noise_shaping_ir_bwd_ws_bytes(int64_t R, int64_t C, int64_t K, int64_t ir_len) {
    if (R <= 0 || C <= 0 || K <= 0 || ir_len <= 0) return 0;
    return (size_t)R * (size_t)C * (size_t)((ir_len + gfx::NSB_CHUNK - 1) / gfx::NSB_CHUNK) * (size_t)gfx::nsb_stride(K) *
           sizeof(float);
}

int gfx_noise_shaping_ir_bwd_f32(const float* grad_ir, const float* ir, const float* row_gain, const float* noise,
                                 int64_t noise_stride, const float* log_decay, const float* log_gain,
                                 const float* log_fade_in, const float* z_fade_in_gain, float* g_log_decay,
                                 float* g_log_gain, float* g_log_fade_in, float* g_z_fade_in_gain, int64_t R, int64_t C,
                                 int64_t K, int64_t ir_len, float min_decay, float max_decay, void* ws, size_t ws_bytes,
                                 void* stream) {
    if (!grad_ir || !noise || !log_decay || !log_gain || R <= 0 || C <= 0 || K <= 0 || K > gfx::NS_MAX_K || ir_len <= 0)
        return GFX_EINVAL;
    if ((ir == nullptr) != (row_gain == nullptr) || (log_fade_in == nullptr) != (z_fade_in_gain == nullptr))
        return GFX_EINVAL;
    if (!g_log_decay && !g_log_gain && !g_log_fade_in && !g_z_fade_in_gain) return GFX_EINVAL;
    if ((g_log_fade_in || g_z_fade_in_gain) && !log_fade_in) return GFX_EINVAL;
    if (noise_stride < ir_len || C > 65535 || R * C > 0x7fffffffLL) return GFX_EINVAL;
    const int64_t nchunk = (ir_len + gfx::NSB_CHUNK - 1) / gfx::NSB_CHUNK;
    if (nchunk > 0x7fffffffLL) return GFX_EINVAL;
    if (!ws || ws_bytes < gfx_noise_shaping_ir_bwd_ws_bytes(R, C, K, ir_len)) return GFX_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    float* partial = (float*)ws;
    const bool fade = log_fade_in != nullptr, norm = ir != nullptr;
    auto kern = fade ? (norm ? gfx::noise_shaping_ir_bwd_kernel<true, true> : gfx::noise_shaping_ir_bwd_kernel<true, false>)
                     : (norm ? gfx::noise_shaping_ir_bwd_kernel<false, true> : gfx::noise_shaping_ir_bwd_kernel<false, false>);
    const size_t lds = (size_t)K * (fade ? 4 : 2) * (norm ? 2 : 1) * 16 * sizeof(float);   // <= 32 KiB
    gfx::for_channel_aligned_rows(R * C, C, [&](int64_t done, int64_t n) {
        hipLaunchKernelGGL(kern, dim3((unsigned)nchunk, (unsigned)n), dim3(256), lds, st, grad_ir + done * ir_len,
                           ir ? ir + done * ir_len : nullptr, noise, noise_stride, log_decay + done * K,
                           log_fade_in ? log_fade_in + done * K : nullptr, partial + done * nchunk * gfx::nsb_stride(K),
                           (int)C, (int)K, ir_len, min_decay, max_decay);
    });
    hipLaunchKernelGGL(gfx::noise_shaping_ir_bwd_finish_kernel, dim3((unsigned)(R * C)), dim3(64), 0, st,
                       (const float*)partial, row_gain, log_decay, log_gain, log_fade_in, z_fade_in_gain, g_log_decay,
                       g_log_gain, g_log_fade_in, g_z_fade_in_gain, (int)C, (int)K, (int)nchunk, min_decay, max_decay);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
