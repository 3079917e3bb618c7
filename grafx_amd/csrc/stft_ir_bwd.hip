// STFT-masked noise reverb: the backward of the impulse-response synthesis in its FFT form (stft_ir.hip:
// stft_ir_fft384_kernel; n_fft = 384, hop = 192) -- a dot pre-pass, the frame kernel and a finishing kernel.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/grafx_amd.h"
#include "small_dft.hpp"
#include "stft_ir.hpp"

namespace gfx {

// ---- backward of the FFT form: dL/d(init, delta, gain_env) from dL/dh --------------------------------------------------
// The adjoint of stft_ir_fft384_kernel (+ the normalisation), frame by frame.  With v the un-normalised taps the forward
// stored, gain = row_gain and gh = dL/dh:
//   gv = gain gh - gain^3 v S / 2,  S = sum_{c,t} gh v      (normalised; gv = gh otherwise)
//   gs = (gv0 + gv1, gv0 - gv1)                             (ms_to_lr is its own transpose)
//   gy[192 + t] = gs[t] / env[192 + t]                      (env: the forward's w1^2 (+ w0^2); zero outside [0, ir_len))
//   gf[m][n] = window[n] gy[192 m + n],  GF[k, m] = sum_n gf[m][n] e^(-2 pi i k n / 384)
//   g_lm[k, m] = (1|2)/384 (Re nz Re GF + Im nz Im GF) mask / 8      (Im of DC / Nyquist does not count, as in the forward)
//   g_init[k] = sum_m g_lm,  g_delta[k] = -sigmoid(delta[k]) sum_m m g_lm,  g_gain_env[m] = sum_k g_lm.
// Frame m reads the blocks m - 1 and m of 192 taps and writes nothing that overlaps, so a workgroup takes FR whole frames
// (none is redone, unlike the forward): it builds gy of its FR + 1 blocks of both channels in LDS, then per channel runs
// the forward real DFT as one 192-point complex transform of z[j] = gf[2j] + i gf[2j+1] -- the mirror of the forward
// kernel: lane l transforms z[l + LN j], j < C1, in registers, multiplies by e^(-2 pi i b l / 192), hands over through LDS,
// LN-point transforms give Z[C1 a + b]; GF[k] = E[k] + e^(-2 pi i k / 384) O[k], E = (Z[k] + conj Z[192-k]) / 2,
// O = (Z[k] - conj Z[192-k]) / 2i.  Frames, spectra and g_lm stay in LDS.  Sums, all in a fixed order and without atomics:
// g_gain_env[m] is complete in its workgroup (each lane its bins in order, then a butterfly over the frame's LN lanes);
// the bin sums over the workgroup's frames are taken by thread k over f = 0 .. FR - 1 and stored as one partial per
// workgroup, which stft_ir_bwd_finish_kernel adds in double in workgroup order.  S comes from a pre-pass of block partials
// (stft_ir_bwd_dot_kernel) that every workgroup of the row adds in double in the same order.
constexpr int IRB_DOT = 4096;        // elements of the flattened (2, ir_len) row per workgroup of the pre-pass
constexpr int IRB_FR = 16, IRB_LN = 16;

// workgroups per row of the pre-pass and of the frame kernel: the workspace holds a partial for each
inline int64_t irb_ndot(int64_t ir_len) { return (2 * ir_len + IRB_DOT - 1) / IRB_DOT; }
inline int64_t irb_nwg(int64_t num_frames) { return (num_frames + IRB_FR - 1) / IRB_FR; }

__global__ __launch_bounds__(256) void stft_ir_bwd_dot_kernel(const float* __restrict__ gh, const float* __restrict__ v,
                                                              float* __restrict__ partial, int64_t row_len) {
    __shared__ float red[4];
    const int64_t r = blockIdx.y;
    const float* a = gh + r * row_len;
    const float* b = v + r * row_len;
    const int64_t i0 = (int64_t)blockIdx.x * IRB_DOT + threadIdx.x;
    float e = 0.0f;
#pragma unroll
    for (int j = 0; j < IRB_DOT / 256; ++j) {
        const int64_t i = i0 + 256 * j;
        if (i < row_len) e = fmaf(a[i], b[i], e);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) e += __shfl_down(e, d, 64);   // the block sum of istft_ola_kernel (stft_ir.hip)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = e;
    __syncthreads();
    if (threadIdx.x == 0) partial[r * gridDim.x + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

template <int FR, int LN>
__global__ __launch_bounds__(FR * LN) void stft_ir_bwd_fft384_kernel(
    const float* __restrict__ gh,          // (R,2,ir_len)
    const float* __restrict__ v,           // (R,2,ir_len) the forward's un-normalised taps, or null (un-normalised mode)
    const float* __restrict__ row_gain,    // (R), with v
    const float* __restrict__ dot_partial, // (R,ndot), with v
    const float* __restrict__ noise_stft, const float* __restrict__ init_lm, const float* __restrict__ delta_lm,
    const float* __restrict__ gain_env, const float* __restrict__ window, const float* __restrict__ tables,
    float* __restrict__ g_gain_env,        // (R,2,T) or null
    float* __restrict__ partial,           // (R,nwg,2,2,K): sum_m g_lm, sum_m m g_lm of the workgroup's frames
    IstftArgs a, int ms_to_lr, int ndot) {
    constexpr int M = 192, C1 = M / LN, NT = FR * LN, PITCH = f3_pitch<LN>(), OP = f3_ola_pitch<LN>(), NB = FR + 1, K = 193;
    constexpr int QG = (K + LN - 1) / LN;    // bins a lane finishes
    static_assert(C1 <= LN, "one second-stage transform per lane");
    static_assert(NT >= K && NT >= 64, "thread k sums bin k");
    __shared__ __attribute__((aligned(16))) float gys[2 * NB * OP];   // gy of the workgroup's blocks, both channels
    __shared__ __attribute__((aligned(16))) cxf Xs[FR * PITCH];       // stage-1 results, then Z, then g_lm (as floats)
    __shared__ cxf tw384[M], tw192[M];
    __shared__ float slope_s[200], h0_s[200], win_s[384];
    __shared__ float coef_s[2];
    const int tid = threadIdx.x;
    const int64_t r = blockIdx.y;
    const int mfirst = blockIdx.x * FR;     // first frame; local block jl is the block mfirst - 1 + jl of 192 taps
    // (the staging loops and the log-mask expression are stft_ir_fft384_kernel's, written out: shared, they reorder both)
    for (int i = tid; i < 2 * M; i += NT) {
        if (i < M) {
            tw384[i] = reinterpret_cast<const cxf*>(tables)[i];
            tw192[i] = reinterpret_cast<const cxf*>(tables)[M + i];
        }
        win_s[i] = window[i];
    }
    if (tid < 64) {
        // gv = cg gh - cv v: S in double from the pre-pass partials, lane l takes l, l + 64, ... in order, then a tree
        float cg = 1.0f, cv = 0.0f;
        if (v) {
            double s = 0.0;
            for (int b = tid; b < ndot; b += 64) s += (double)dot_partial[r * ndot + b];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_down(s, d, 64);
            cg = row_gain[r];
            cv = (float)(0.5 * (double)cg * (double)cg * (double)cg * s);
        }
        if (tid == 0) {
            coef_s[0] = cg;
            coef_s[1] = cv;
        }
    }
    __syncthreads();
    {
        const float cg = coef_s[0], cv = coef_s[1];
        const float* gh0 = gh + (r * 2) * a.ir_len;
        const float* gh1 = gh0 + a.ir_len;
        const float* v0p = v ? v + (r * 2) * a.ir_len : nullptr;
        for (int i = tid; i < NB * M; i += NT) {
            const int jl = i / M, s = i - jl * M;
            const int j = mfirst - 1 + jl;
            const int64_t t = (int64_t)j * M + s;
            float y0 = 0.0f, y1 = 0.0f;
            if (j >= 0 && t < a.ir_len) {
                float g0 = gh0[t], g1 = gh1[t];
                if (v0p) {
                    g0 = cg * g0 - cv * v0p[t];
                    g1 = cg * g1 - cv * v0p[a.ir_len + t];
                }
                if (ms_to_lr) {
                    const float sm = g0 + g1, df = g0 - g1;
                    g0 = sm;
                    g1 = df;
                }
                const float w1 = win_s[s + M], w0 = win_s[s];
                float env = fmaf(w1, w1, 0.0f);
                if (j + 1 < a.T) env = fmaf(w0, w0, env);
                y0 = g0 / env;
                y1 = g1 / env;
            }
            gys[jl * OP + s] = y0;
            gys[NB * OP + jl * OP + s] = y1;
        }
    }
    const int f = tid / LN, l = tid % LN;   // LN lanes per frame
    const int m = mfirst + f;
    const bool m_ok = m < a.T;
    const float mf = (float)m;
    float* G = reinterpret_cast<float*>(Xs);
    for (int c = 0; c < 2; ++c) {
        const int64_t rc = r * 2 + c;
        for (int i = tid; i < K; i += NT) {
            slope_s[i] = -softplus_t(delta_lm[rc * K + i]);
            h0_s[i] = init_lm[rc * K + i];
        }
        // the frame's noise bins in flight while the transform runs; lane l takes bins l, l + LN, ...
        const float* nz0 = noise_stft + r * a.nstride + ((int64_t)c * K * a.T + (m_ok ? m : 0)) * 2;
        float2 nz[QG];
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const int k = l + LN * q;
            nz[q] = (m_ok && k < K) ? *reinterpret_cast<const float2*>(nz0 + (int64_t)k * a.T * 2) : make_float2(0.0f, 0.0f);
        }
        const float genv = (gain_env && m_ok) ? gain_env[rc * a.T + m] : 0.0f;
        __syncthreads();   // gys, the parameters; the previous channel's reads of G are done
        cxf x1[C1];
        {
            const float* gy = gys + c * NB * OP + f * OP;    // samples n < 192 of the frame; n >= 192 in the next block
#pragma unroll
            for (int j = 0; j < C1; ++j) {
                const int n = 2 * (l + LN * j);              // n, n + 1 lie in the same block (192 is even)
                const float2 g = *reinterpret_cast<const float2*>(n < M ? gy + n : gy + OP + (n - M));
                x1[j] = cxf{win_s[n] * g.x, win_s[n + 1] * g.y};
            }
        }
        sdft<C1, false>(x1);
#pragma unroll
        for (int b = 0; b < C1; ++b) {
            const cxf y = x1[spos(C1, b)], w = tw192[b * l];       // times conj(w)
            Xs[f * PITCH + b * LN + l] = cxf{y.x * w.x + y.y * w.y, y.y * w.x - y.x * w.y};
        }
        __syncthreads();
        cxf u[LN];
        if (l < C1) {
            const cxf* Y = Xs + f * PITCH + l * LN;
#pragma unroll
            for (int i = 0; i < LN; ++i) u[i] = Y[i];
            sdft<LN, false>(u);
        }
        __syncthreads();   // every stage-1 value has been read
        if (l < C1) {
#pragma unroll
            for (int aa = 0; aa < LN; ++aa) Xs[f * PITCH + C1 * aa + l] = u[spos(LN, aa)];   // Z[C1 a + b]
        }
        __syncthreads();
        float gl[QG];
        {
            const cxf* Z = Xs + f * PITCH;
#pragma unroll
            for (int q = 0; q < QG; ++q) {
                const int k = l + LN * q;
                gl[q] = 0.0f;
                if (k < K) {
                    const cxf A = Z[k == M ? 0 : k], B = Z[(k == 0 || k == M) ? 0 : M - k];
                    const cxf e = cxf{A.x + B.x, A.y - B.y};                  // A + conj B
                    const cxf d = cxf{A.y + B.y, B.x - A.x};                  // (A - conj B) / i
                    const cxf w = k == M ? cxf{-1.0f, 0.0f} : tw384[k];       // times conj(w)
                    const cxf o = cxf{d.x * w.x + d.y * w.y, d.y * w.x - d.x * w.y};
                    const cxf gf = (e + o) * 0.5f;
                    const bool edge = k == 0 || k == M;
                    float lm = __fadd_rn(h0_s[k], __fmul_rn(slope_s[k], mf));
                    if (gain_env) lm = __fadd_rn(lm, genv);
                    const float mask = expf(lm / 8.0f);
                    const float dotp = edge ? nz[q].x * gf.x : 2.0f * (nz[q].x * gf.x + nz[q].y * gf.y);
                    gl[q] = m_ok ? dotp * (1.0f / 384.0f) * mask * 0.125f : 0.0f;
                }
            }
        }
        {
            float s = 0.0f;
#pragma unroll
            for (int q = 0; q < QG; ++q) s += gl[q];
#pragma unroll
            for (int d = LN / 2; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
            if (g_gain_env && m_ok && l == 0) g_gain_env[rc * a.T + m] = s;
        }
        __syncthreads();   // every Z has been read
#pragma unroll
        for (int q = 0; q < QG; ++q) {
            const int k = l + LN * q;
            if (k < K) G[f * (2 * PITCH) + k] = gl[q];
        }
        __syncthreads();
        if (tid < K) {
            float s0 = 0.0f, s1 = 0.0f;
#pragma unroll
            for (int ff = 0; ff < FR; ++ff) {
                const float g = G[ff * (2 * PITCH) + tid];
                s0 += g;
                s1 = fmaf((float)(mfirst + ff), g, s1);
            }
            float* p = partial + (((r * gridDim.x + blockIdx.x) * 2 + c) * 2) * K;
            p[tid] = s0;
            p[K + tid] = s1;
        }
    }
}

// g_init[r,c,k] = sum_wg partial[.][0][k], g_delta[r,c,k] = -sigmoid(delta[r,c,k]) sum_wg partial[.][1][k]: in double, in
// workgroup order.  grid: R * 2 (row-channels), thread k.
__global__ __launch_bounds__(256) void stft_ir_bwd_finish_kernel(const float* __restrict__ partial,
                                                                 const float* __restrict__ delta_lm,
                                                                 float* __restrict__ g_init, float* __restrict__ g_delta,
                                                                 int nwg) {
    constexpr int K = 193;
    const int k = threadIdx.x;
    if (k >= K) return;
    const int64_t rc = blockIdx.x, r = rc >> 1;
    const int c = (int)(rc & 1);
    double s0 = 0.0, s1 = 0.0;
    for (int w = 0; w < nwg; ++w) {
        const float* p = partial + (((r * nwg + w) * 2 + c) * 2) * K;
        s0 += (double)p[k];
        s1 += (double)p[K + k];
    }
    if (g_init) g_init[rc * K + k] = (float)s0;
    if (g_delta) {
        const float d = delta_lm[rc * K + k];
        const float sg = d > 20.0f ? 1.0f : 1.0f / (1.0f + expf(-d));   // d/dx of softplus_t
        g_delta[rc * K + k] = (float)(-(double)sg * s1);
    }
}

}  // namespace gfx

extern "C" {

size_t gfx_stft_reverb_ir_bwd_ws_bytes(int64_t R, int64_t ir_len) {
    if (R <= 0 || ir_len <= 0) return 0;
    return (size_t)R * (size_t)(gfx::irb_ndot(ir_len) + gfx::irb_nwg(1 + ir_len / 192) * 2 * 2 * 193) * sizeof(float);
}

int gfx_stft_reverb_ir_bwd_f32(const float* grad_ir, const float* ir, const float* row_gain, const float* noise_stft,
                               int64_t noise_rows, const float* init_log_magnitude, const float* delta_log_magnitude,
                               const float* gain_env_log_magnitude, const float* window, const float* basis,
                               float* g_init, float* g_delta, float* g_gain_env, int64_t R, int64_t ir_len, int64_t n_fft,
                               int64_t hop, int64_t num_frames, int ms_to_lr, void* ws, size_t ws_bytes, void* stream) {
    if (noise_rows != 1 && noise_rows != R) return GFX_EINVAL;
    if (!grad_ir || !noise_stft || !init_log_magnitude || !delta_log_magnitude || !window || !basis) return GFX_EINVAL;
    if ((ir == nullptr) != (row_gain == nullptr) || (!g_init && !g_delta && !g_gain_env)) return GFX_EINVAL;
    if (g_gain_env && !gain_env_log_magnitude) return GFX_EINVAL;
    if (n_fft != 384 || hop != 192) return GFX_EINVAL;   // the FFT form only
    if (R <= 0 || R * 2 > 65535 || ir_len <= 0 || num_frames != 1 + ir_len / 192 || num_frames > 0x7fffffffLL / 193)
        return GFX_EINVAL;
    if (!ws || ws_bytes < gfx_stft_reverb_ir_bwd_ws_bytes(R, ir_len)) return GFX_ENOSPC;
    const gfx::IstftArgs a = gfx::istft_args(R, n_fft, hop, num_frames, ir_len, noise_rows);
    hipStream_t st = (hipStream_t)stream;
    const int64_t ndot = gfx::irb_ndot(ir_len), nwg = gfx::irb_nwg(num_frames);
    float* dot_partial = (float*)ws;
    float* partial = dot_partial + R * ndot;
    if (ir)
        hipLaunchKernelGGL(gfx::stft_ir_bwd_dot_kernel, dim3((unsigned)ndot, (unsigned)R), dim3(256), 0, st, grad_ir, ir,
                           dot_partial, 2 * ir_len);
    hipLaunchKernelGGL((gfx::stft_ir_bwd_fft384_kernel<gfx::IRB_FR, gfx::IRB_LN>), dim3((unsigned)nwg, (unsigned)R),
                       dim3(gfx::IRB_FR * gfx::IRB_LN), 0, st, grad_ir, ir, row_gain, (const float*)dot_partial, noise_stft,
                       init_log_magnitude, delta_log_magnitude, gain_env_log_magnitude, window,
                       basis + gfx::basis_tables_off(n_fft), g_gain_env, partial, a, ms_to_lr, (int)ndot);
    if (g_init || g_delta)
        hipLaunchKernelGGL(gfx::stft_ir_bwd_finish_kernel, dim3((unsigned)(R * 2)), dim3(256), 0, st, (const float*)partial,
                           delta_log_magnitude, g_init, g_delta, (int)nwg);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
