// The dynamics stages as standalone passes (used when a configuration cannot take the fused kernel of dynamics.hip):
// energy, the truncated one-pole smoother and its taps, the gain computer, the gain stage, StereoGain.
// Replaces (reference src/grafx/processors): TruncatedOnePoleIIRFilter (core/envelope.py:34-60), energy and the gain
// stage of Compressor / NoiseGate (dynamics.py:390-405), StereoGain (stereo.py:38-41).
// Kernels and entry points: included by dynamics.hip alone and compiled as part of it (the end of that file says why).
#pragma once
#include "dyn_common.hpp"

namespace gfx {

// energy: e[r,n] = mean_c x[r,c,n]^2
__global__ void energy_kernel(const float* __restrict__ x, gfx_rowmap_t xmap, float* __restrict__ e, int64_t R, int64_t L, int C) {
    const float invC = 1.0f / (float)C;
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
        const float* x0 = x + row_off(xmap, r, 0);
        const float* x1 = x + row_off(xmap, r, C == 2 ? 1 : 0);
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < L; n += (int64_t)gridDim.x * blockDim.x) {
            const float a = x0[n], b = x1[n];
            e[r * L + n] = (C == 2 ? (a * a + b * b) : a * a) * invC;
        }
    }
}

// truncated one-pole on (R, L) rows -> (R, Lout); Lout may extend to L + N - 1 (full convolution)
// ESRC (round 6): the rows are the energy mean_c x^2 of a signal read in place (dynamics.py:390) -- the envelope of a
// compressor whose smoother's convolve() aliases (upstream's default tap counts) no longer goes through an energy buffer.
// rowmax (nullable): receives the bits of max |out| of the row (one workgroup walks the row: a plain store), the by-product
// the odd-length aliasing's pair scaling asks for (czt_pair.hip).
template <bool TRUNC, bool ESRC>
__device__ __forceinline__ void onepole_stream(const OnePole& p, const float* u_in, const float* x1, int C, float* out, int64_t L,
                                               int64_t Lout, int64_t N, int relu, float* slots, int t, uint32_t* rowmax) {
    const int lane = t & 63, wave = t >> 6;
    const bool vi = vec_ok(u_in) && (!ESRC || vec_ok(x1)), vo = vec_ok(out);
    const float invC = 1.0f / (float)C;
    auto load_e = [&](int64_t n, bool vec, float (&e)[DE]) {
        load4(u_in, n, L, vec, e);
        if (ESRC) {
            float b[DE] = {0.0f, 0.0f, 0.0f, 0.0f};
            if (C == 2) load4(x1, n, L, vec, b);
#pragma unroll
            for (int i = 0; i < DE; ++i) e[i] = (C == 2 ? (e[i] * e[i] + b[i] * b[i]) : e[i] * e[i]) * invC;
        }
    };
    float carry = 0.0f;
    uint32_t mx = 0;
    const int64_t ntiles = (Lout + DTILE - 1) / DTILE;
    float ne[DE];  // software prefetch of the next tile (see dyn_stream)
    load_e((int64_t)DE * t, vi, ne);
    for (int64_t tile = 0; tile < ntiles; ++tile) {
        const int64_t n = tile * DTILE + DE * t;
        float e[DE], u[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) e[i] = ne[i];
        if (tile + 1 < ntiles) load_e(n + DTILE, vi, ne);
        if (TRUNC) {  // one scan of e[n] - a^N e[n-N] (see dyn_stream)
            float e2[DE];
            load_e(n - N, false, e2);
#pragma unroll
            for (int i = 0; i < DE; ++i) e[i] = fmaf(-p.a_N, e2[i], e[i]);
        }
        scan_tile(p, e, u, carry, slots + 8 * (tile & 1), lane, wave);
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            u[i] = p.one_m_a * u[i];
            if (relu) u[i] = fmaxf(u[i], 0.0f);
            const uint32_t b = __float_as_uint(u[i]) & 0x7fffffffu;
            if (rowmax && n + i < Lout) mx = b > mx ? b : mx;
        }
        store4(out, n, Lout, vo, u);
    }
    if (rowmax) {      // (uniform)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const uint32_t v = (uint32_t)__shfl_xor((int)mx, o);
            mx = v > mx ? v : mx;
        }
        __syncthreads();
        if (lane == 0) slots[wave] = __uint_as_float(mx);
        __syncthreads();
        if (t == 0) {
            uint32_t m = 0;
            for (int w = 0; w < DT / 64; ++w) {
                const uint32_t v = __float_as_uint(slots[w]);
                m = v > m ? v : m;
            }
            *rowmax = m;
        }
    }
}

template <bool ESRC>
__global__ __launch_bounds__(DT) void onepole_kernel(const float* __restrict__ u, gfx_rowmap_t xmap, int C,
                                                     const float* __restrict__ z_alpha, float* __restrict__ out, int64_t L,
                                                     int64_t Lout, int64_t N, int relu, uint32_t* __restrict__ rowmax) {
    __shared__ float slots[16];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    OnePole p;
    onepole_setup(p, z_alpha[r], N, t & 63);
    const float* in0 = ESRC ? u + row_off(xmap, r, 0) : u + r * L;
    const float* in1 = ESRC ? u + row_off(xmap, r, C == 2 ? 1 : 0) : nullptr;
    uint32_t* rm = rowmax ? rowmax + r : nullptr;
    // the FIR has exactly N taps: when Lout > L the tail still needs the a^N term once n >= N
    if (p.trunc)
        onepole_stream<true, ESRC>(p, in0, in1, C, out + r * Lout, L, Lout, N, relu, slots, t, rm);
    else
        onepole_stream<false, ESRC>(p, in0, in1, C, out + r * Lout, L, Lout, N, relu, slots, t, rm);
}

// one-pole FIR taps themselves, h[n] = (1-a) * exp(n * log a)  (envelope.py:51-60), for the generic conv path
__global__ void onepole_fir_kernel(const float* __restrict__ z_alpha, float* __restrict__ h, int64_t R, int64_t N) {
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
        const float a = fminf(sigmoidf(z_alpha[r]), 1.0f - 1e-5f);
        const float la = logf(a);
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < N; n += (int64_t)gridDim.x * blockDim.x)
            h[r * N + n] = (1.0f - a) * expf((float)n * la);
    }
}

// env (R,L) -> gain (R,L):  g = log_gain(log(env + 1e-5));  out = exp(g) or g (log_out)
__global__ void dyn_gain_kernel(const float* __restrict__ env, float* __restrict__ gain,
                                const float* __restrict__ log_threshold, const float* __restrict__ log_ratio,
                                const float* __restrict__ log_knee, int64_t R, int64_t L, int knee, int gate,
                                int log_out) {
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
        Knee q;
        knee_setup(q, log_threshold[r], log_ratio[r], log_knee ? log_knee[r] : 0.0f, knee, gate);
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < L; n += (int64_t)gridDim.x * blockDim.x) {
            const float g = log_gain(q, logf(env[r * L + n] + 1e-5f));
            gain[r * L + n] = log_out ? g : expf(g);
        }
    }
}

// y[r,c,n] = (exp_gain ? exp(g[r,n]) : g[r,n]) * x[r,c,n]
__global__ void apply_gain_kernel(const float* __restrict__ x, gfx_rowmap_t xmap, const float* __restrict__ g,
                                  float* __restrict__ y, gfx_rowmap_t ymap, int64_t R, int64_t L, int C,
                                  int exp_gain) {
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y)
    for (int c = 0; c < C; ++c) {
        const float* xr = x + row_off(xmap, r, c);
        float* yr = y + row_off(ymap, r, c);
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < L; n += (int64_t)gridDim.x * blockDim.x) {
            const float gv = g[r * L + n];
            yr[n] = (exp_gain ? expf(gv) : gv) * xr[n];
        }
    }
}

// y[r,c,n] = exp(log_gain(log(env[r,n] + 1e-5))) * x[r,c,n]: gain computer and gain stage in one pass over an envelope
// that a smoother kernel left in memory (the ballistics configurations: dynamics.py:394-405 behind core/envelope.py:84-101).
// Four samples per thread, 16-byte accesses when the rows allow it.
__global__ __launch_bounds__(256) void dyn_gain_apply_kernel(const float* __restrict__ x, gfx_rowmap_t xmap,
                                                             const float* __restrict__ env, float* __restrict__ y,
                                                             gfx_rowmap_t ymap, const float* __restrict__ log_threshold,
                                                             const float* __restrict__ log_ratio,
                                                             const float* __restrict__ log_knee, int64_t R, int64_t L, int C,
                                                             int knee, int gate, unsigned prows, int vec) {
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
        const unsigned pr = (unsigned)r % prows;
        Knee q;
        knee_setup(q, log_threshold[pr], log_ratio[pr], log_knee ? log_knee[pr] : 0.0f, knee, gate);
        const float* x0 = x + row_off(xmap, r, 0);
        const float* x1 = x + row_off(xmap, r, C == 2 ? 1 : 0);
        float* y0 = y + row_off(ymap, r, 0);
        float* y1 = y + row_off(ymap, r, C == 2 ? 1 : 0);
        const float* er = env + r * L;
        for (int64_t n = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * DE; n < L; n += (int64_t)gridDim.x * blockDim.x * DE) {
            float e[DE], a[DE], b[DE] = {0.0f, 0.0f, 0.0f, 0.0f};
            load4(er, n, L, vec, e);
            load4(x0, n, L, vec, a);
            if (C == 2) load4(x1, n, L, vec, b);
#pragma unroll
            for (int i = 0; i < DE; ++i) {
                const float g = expf(log_gain(q, logf(e[i] + 1e-5f)));
                a[i] *= g;
                b[i] *= g;
            }
            store4(y0, n, L, vec, a);
            if (C == 2) store4(y1, n, L, vec, b);
        }
    }
}

// StereoGain: y[r,c,n] = x[r,cx,n] * exp(log_gain[r,c])   (stereo.py:38-41; mono input broadcasts to 2 channels)
__global__ void stereo_gain_kernel(const float* __restrict__ x, gfx_rowmap_t xmap, const float* __restrict__ log_gain,
                                   float* __restrict__ y, gfx_rowmap_t ymap, int64_t R, int64_t L, int Cin) {
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y)
    for (int c = 0; c < 2; ++c) {
        const float g = expf(log_gain[2 * r + c]);
        const float* xr = x + row_off(xmap, r, Cin == 2 ? c : 0);
        float* yr = y + row_off(ymap, r, c);
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < L; n += (int64_t)gridDim.x * blockDim.x)
            yr[n] = xr[n] * g;
    }
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_energy_f32(const float* x, gfx_rowmap_t xmap, float* e, int64_t R, int64_t C, int64_t L, void* stream) {
    if (!x || !e || R <= 0 || L <= 0 || (C != 1 && C != 2)) return GFX_EINVAL;
    hipLaunchKernelGGL(energy_kernel, row_grid(R, L), dim3(256), 0, (hipStream_t)stream, x, xmap, e, R, L, (int)C);
    return GFX_LAUNCH_OK();
}

int gfx_onepole_f32(const float* u, const float* z_alpha, float* out, int64_t R, int64_t L, int64_t Lout,
                    int64_t iir_len, int relu, void* stream) {
    if (!u || !z_alpha || !out || R <= 0 || L <= 0 || Lout <= 0 || iir_len < 1 || R > 0x7fffffffLL) return GFX_EINVAL;
    const gfx_rowmap_t none = {1, 0, 0, 0};
    hipLaunchKernelGGL(onepole_kernel<false>, dim3((unsigned)R), dim3(DT), 0, (hipStream_t)stream, u, none, 1, z_alpha, out, L,
                       Lout, iir_len, relu, (uint32_t*)nullptr);
    return GFX_LAUNCH_OK();
}

int gfx_onepole_energy_f32(const float* x, gfx_rowmap_t xmap, int64_t C, const float* z_alpha, float* out, int64_t R,
                           int64_t L, int64_t Lout, int64_t iir_len, int relu, uint32_t* rowmax, void* stream) {
    if (!x || !z_alpha || !out || R <= 0 || L <= 0 || Lout <= 0 || iir_len < 1 || R > 0x7fffffffLL || (C != 1 && C != 2) ||
        xmap.inner <= 0)
        return GFX_EINVAL;
    hipLaunchKernelGGL(onepole_kernel<true>, dim3((unsigned)R), dim3(DT), 0, (hipStream_t)stream, x, xmap, (int)C, z_alpha, out,
                       L, Lout, iir_len, relu, rowmax);
    return GFX_LAUNCH_OK();
}

int gfx_onepole_fir_f32(const float* z_alpha, float* h, int64_t R, int64_t iir_len, void* stream) {
    if (!z_alpha || !h || R <= 0 || iir_len < 1) return GFX_EINVAL;
    hipLaunchKernelGGL(onepole_fir_kernel, row_grid(R, iir_len), dim3(256), 0, (hipStream_t)stream, z_alpha, h, R, iir_len);
    return GFX_LAUNCH_OK();
}

int gfx_dyn_gain_f32(const float* env, float* gain, const float* log_threshold, const float* log_ratio,
                     const float* log_knee, int64_t R, int64_t L, int knee, int gate, int log_out, void* stream) {
    if (!env || !gain || !log_threshold || !log_ratio || R <= 0 || L <= 0) return GFX_EINVAL;
    if (knee < 0 || knee > 2 || (knee != 0 && !log_knee)) return GFX_EINVAL;
    hipLaunchKernelGGL(dyn_gain_kernel, row_grid(R, L), dim3(256), 0, (hipStream_t)stream, env, gain, log_threshold,
                       log_ratio, log_knee, R, L, knee, gate, log_out);
    return GFX_LAUNCH_OK();
}

int gfx_apply_gain_f32(const float* x, gfx_rowmap_t xmap, const float* g, float* y, gfx_rowmap_t ymap, int64_t R,
                       int64_t C, int64_t L, int exp_gain, void* stream) {
    if (!x || !g || !y || R <= 0 || L <= 0 || C < 1) return GFX_EINVAL;
    hipLaunchKernelGGL(apply_gain_kernel, row_grid(R, L), dim3(256), 0, (hipStream_t)stream, x, xmap, g, y, ymap, R, L,
                       (int)C, exp_gain);
    return GFX_LAUNCH_OK();
}

int gfx_dyn_gain_apply_f32(const float* x, gfx_rowmap_t xmap, const float* env, float* y, gfx_rowmap_t ymap,
                           const float* log_threshold, const float* log_ratio, const float* log_knee, int64_t param_rows,
                           int64_t R, int64_t C, int64_t L, int knee, int gate, void* stream) {
    if (!x || !env || !y || !log_threshold || !log_ratio || R <= 0 || L <= 0 || (C != 1 && C != 2)) return GFX_EINVAL;
    if (knee < 0 || knee > 2 || (knee != 0 && !log_knee) || param_rows < 1 || param_rows > R) return GFX_EINVAL;
    const int vec = L % 4 == 0 && al16(x, xmap) && al16(y, ymap) && ((uintptr_t)env & 15) == 0;
    int64_t bx = (L + 4 * 256 - 1) / (4 * 256);
    if (bx > 128) bx = 128;
    hipLaunchKernelGGL(dyn_gain_apply_kernel, dim3((unsigned)bx, (unsigned)(R > 65535 ? 65535 : R)), dim3(256), 0,
                       (hipStream_t)stream, x, xmap, env, y, ymap, log_threshold, log_ratio, log_knee, R, L, (int)C, knee,
                       gate, (unsigned)param_rows, vec);
    return GFX_LAUNCH_OK();
}

int gfx_stereo_gain_f32(const float* x, gfx_rowmap_t xmap, const float* log_gain, float* y, gfx_rowmap_t ymap,
                        int64_t R, int64_t C_in, int64_t L, void* stream) {
    if (!x || !log_gain || !y || R <= 0 || L <= 0 || (C_in != 1 && C_in != 2)) return GFX_EINVAL;
    hipLaunchKernelGGL(stereo_gain_kernel, row_grid(R, L), dim3(256), 0, (hipStream_t)stream, x, xmap, log_gain, y,
                       ymap, R, L, (int)C_in);
    return GFX_LAUNCH_OK();
}

}  // extern "C"
