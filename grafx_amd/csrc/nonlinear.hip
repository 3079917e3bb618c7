// Memoryless waveshapers (gfx950): one streaming pass, 8 B per channel-sample, HBM-bound.
//
// Replaces the forward() bodies of grafx.processors.nonlinear (reference nonlinear.py):
//   TanhDistortion           46-79    y = post * (tanh(pre*(x-dc) + b) - tanh(b))
//   PiecewiseTanhDistortion  120-175  tanh in the middle, rescaled tanh branches beyond +kp / -kn
//   PowerDistortion          210-233  y = sum_k tanh(w_k) * f((pre*(x-dc))^k)
//   ChebyshevDistortion      270-307  y = sum_k tanh(w_k) * f(T_k(pre*(x-dc)))
// where f = tanh or identity, dc = the row-channel mean when remove_dc is set (row_mean_kernel),
// pre = exp(log_pre_gain), post = exp(log_post_gain) or 1/pre.  The upstream torch code materialises
// K full-size tensors for the two polynomial shapers; here the K terms live in registers.
// The per-sample math (WsRow, shape, ws_row_setup, bwd_samples) lives in waveshaper.hpp, shared with oversampled.hip.
#include "waveshaper.hpp"

namespace gfx {

struct WsArgs {
    gfx_rowmap_t xmap, ymap;
    int64_t R, L;
    int C, mode, K;
    int use_tanh, inverse_post;
};

template <int MODE>
__global__ __launch_bounds__(256) void waveshaper_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const float* __restrict__ log_pre,
                                                         const float* __restrict__ log_post,
                                                         const float* __restrict__ p0, const float* __restrict__ p1,
                                                         const float* __restrict__ dc, WsArgs a, int vec) {
    __shared__ float sw[WS_MAX_K];
    for (int64_t r = blockIdx.y; r < a.R; r += gridDim.y) {
        WsRow q;
        ws_row_setup<MODE>(q, sw, r, a.K, a.inverse_post, log_pre, log_post, p0, p1);
        for (int c = 0; c < a.C; ++c) {
            q.dc = dc ? dc[r * a.C + c] : 0.0f;
            const float* xr = x + row_off(a.xmap, r, c);
            float* yr = y + row_off(a.ymap, r, c);
            const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
            if (vec) {
                using f4 = float __attribute__((ext_vector_type(4)));
                for (int64_t i = tid; i < a.L / 4; i += nthr) {
                    const f4 v = reinterpret_cast<const f4*>(xr)[i];
                    f4 o;
                    o.x = shape<MODE>(v.x, q, a.K, a.use_tanh);
                    o.y = shape<MODE>(v.y, q, a.K, a.use_tanh);
                    o.z = shape<MODE>(v.z, q, a.K, a.use_tanh);
                    o.w = shape<MODE>(v.w, q, a.K, a.use_tanh);
                    __builtin_nontemporal_store(o, reinterpret_cast<f4*>(yr) + i);
                }
                for (int64_t n = (a.L & ~int64_t(3)) + tid; n < a.L; n += nthr) yr[n] = shape<MODE>(xr[n], q, a.K, a.use_tanh);
            } else {
                for (int64_t n = tid; n < a.L; n += nthr) yr[n] = shape<MODE>(xr[n], q, a.K, a.use_tanh);
            }
        }
    }
}

// mean over time of every row-channel (the remove_dc option): one workgroup per row-channel
__global__ __launch_bounds__(256) void row_mean_kernel(const float* __restrict__ x, gfx_rowmap_t xmap,
                                                       float* __restrict__ mean, int64_t R, int C, int64_t L) {
    __shared__ float part[4];
    for (int64_t rc = blockIdx.x; rc < R * C; rc += gridDim.x) {
        const int64_t r = rc / C;
        const float* xr = x + row_off(xmap, r, (int)(rc - r * C));
        float s = 0.0f;
        for (int64_t n = threadIdx.x; n < L; n += 256) s += xr[n];
        for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
        __syncthreads();
        if (threadIdx.x == 0) mean[rc] = (part[0] + part[1] + part[2] + part[3]) / (float)L;
        __syncthreads();
    }
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_row_mean_f32(const float* x, gfx_rowmap_t xmap, float* mean, int64_t R, int64_t C, int64_t L, void* stream) {
    if (!x || !mean || R <= 0 || C <= 0 || L <= 0 || xmap.inner <= 0 || R > 0x7fffffffLL) return GFX_EINVAL;
    const int64_t n = R * C;
    return launch(row_mean_kernel, dim3((unsigned)(n > 65535 * 16 ? 65535 * 16 : n)), dim3(256), 0, (hipStream_t)stream, x, xmap,
                  mean, R, (int)C, L);
}

int gfx_waveshaper_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L,
                       int mode, int use_tanh, int inverse_post_gain, const float* log_pre_gain,
                       const float* log_post_gain, const float* p0, const float* p1, int64_t K, const float* dc,
                       void* stream) {
    if (!x || !y || R <= 0 || C <= 0 || L <= 0 || R > 0x7fffffffLL || xmap.inner <= 0 || ymap.inner <= 0) return GFX_EINVAL;
    if (ws_check_shaper(mode, inverse_post_gain, log_pre_gain, p0, p1, K) != GFX_OK) return GFX_EINVAL;
    WsArgs a;
    a.xmap = xmap; a.ymap = ymap; a.R = R; a.L = L; a.C = (int)C; a.mode = mode; a.K = (int)K;
    a.use_tanh = use_tanh; a.inverse_post = inverse_post_gain;
    const int vec = aligned16(x) && aligned16(y) && map_vec(xmap) && map_vec(ymap);
    int64_t bx = (L / 4 + 255) / 256;
    if (bx > 64) bx = 64;
    if (bx < 1) bx = 1;
    const dim3 grid((unsigned)bx, (unsigned)(R > 65535 ? 65535 : R));
    hipStream_t st = (hipStream_t)stream;
    return with_ws_mode(mode, [&](auto m) {
        return launch(waveshaper_kernel<decltype(m)::value>, grid, dim3(256), 0, st, x, y, log_pre_gain, log_post_gain, p0, p1, dc,
                      a, vec);
    });
}

}  // extern "C"

// ---- waveshaper backward ---------------------------------------------------------------------------------------------
// One streaming pass over x and gy (12 B per channel-sample with gx, 8 B without), the K polynomial terms in registers as in
// the forward.  With u = (x - dc) pre, G = gy post, y = post s(u):
//   gx          = G s'(u) pre                     (remove_dc: minus its mean over time per row-channel, ws_sub_mean_kernel)
//   g_log_pre   = sum G (s'(u) u - [inverse_post] s(u))            (the difference per sample: summing both parts and
//   g_log_post  = sum G s(u)                                        subtracting the sums cancels to ~1e-2 of them)
//   g_bias      = sum G (sech^2(u + b) - sech^2(b))
//   g_w[k]      = (1 - tanh^2 w_k) sum G f(B_k(u)),   s' = sum_k tanh(w_k) f'(B_k) B_k',   B_k' = k u^(k-1) or k U_(k-1)(u)
//   piecewise   : d/d log_hardness, d/d z_threshold of the two outer branches, see bwd_samples.
// Row sums: every workgroup reduces its share (registers -> wave shuffles -> LDS) and STORES one partial per sum into the
// workspace; ws_bwd_finish_kernel adds a row's partials in double, in a fixed order -- no float atomics, bit-identical runs.
namespace gfx {

struct WsBwdArgs {
    gfx_rowmap_t xmap, gmap, omap;
    int64_t R, L;
    int C, K, NS;                   // NS: sums per row in the workspace (ws_nsums)
    int use_tanh, inverse_post, want_par;
};

static inline int64_t ws_blocks(int64_t L) {
    const int64_t bx = (L / 4 + 255) / 256;
    return bx > 64 ? 64 : (bx < 1 ? 1 : bx);
}

template <int MODE>
__global__ __launch_bounds__(256) void waveshaper_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                             float* __restrict__ gx, const float* __restrict__ log_pre,
                                                             const float* __restrict__ log_post,
                                                             const float* __restrict__ p0, const float* __restrict__ p1,
                                                             const float* __restrict__ dc, float* __restrict__ part,
                                                             float* __restrict__ dcpart, WsBwdArgs a, int vec) {
    constexpr int NA = WsAcc<MODE>::N;
    constexpr bool POLY = MODE == GFX_WS_POWER || MODE == GFX_WS_CHEBYSHEV;
    __shared__ float sw[WS_MAX_K];
    __shared__ float red[4][NA];
    __shared__ float tot[NA];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool par = a.want_par != 0, use_tanh = a.use_tanh != 0;
    const float inv = a.inverse_post ? 1.0f : 0.0f;
    const int nsum = POLY ? 2 + a.K : NA;            // sums of this mode that are in use
    for (int64_t r = blockIdx.y; r < a.R; r += gridDim.y) {
        WsRow q;
        ws_row_setup<MODE>(q, sw, r, a.K, a.inverse_post, log_pre, log_post, p0, p1);
        float acc[NA];
#pragma unroll
        for (int j = 0; j < NA; ++j) acc[j] = 0.0f;
        for (int c = 0; c < a.C; ++c) {
            q.dc = dc ? dc[r * a.C + c] : 0.0f;
            const float* xr = x + row_off(a.xmap, r, c);
            const float* gr = gy + row_off(a.gmap, r, c);
            float* outr = gx ? gx + row_off(a.omap, r, c) : nullptr;
            const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
            float dsum = 0.0f;
            int64_t n0 = tid;                        // first sample of the scalar loop: the whole row, or the tail
            if (vec) {
                using f4 = float __attribute__((ext_vector_type(4)));
                for (int64_t i = tid; i < a.L / 4; i += nthr) {
                    const f4 v = reinterpret_cast<const f4*>(xr)[i], g = reinterpret_cast<const f4*>(gr)[i];
                    const float xs[4] = {v.x, v.y, v.z, v.w}, gs[4] = {g.x, g.y, g.z, g.w};
                    float go[4];
                    bwd_samples<MODE, 4>(xs, gs, go, q, a.K, use_tanh, inv, par, acc);
                    if (outr) {
                        f4 o;
                        o.x = go[0]; o.y = go[1]; o.z = go[2]; o.w = go[3];
                        reinterpret_cast<f4*>(outr)[i] = o;      // (a plain store: remove_dc reads it back)
                        dsum += (go[0] + go[1]) + (go[2] + go[3]);
                    }
                }
                n0 = (a.L & ~int64_t(3)) + tid;
            }
            for (int64_t n = n0; n < a.L; n += nthr) {
                const float xs[1] = {xr[n]}, gs[1] = {gr[n]};
                float go[1];
                bwd_samples<MODE, 1>(xs, gs, go, q, a.K, use_tanh, inv, par, acc);
                if (outr) {
                    outr[n] = go[0];
                    dsum += go[0];
                }
            }
            if (dcpart) {                            // sum over time of this row-channel's gx, for the centring's adjoint
                dsum = wave_sum(dsum);
                __syncthreads();                     // red[][0] free again
                if (lane == 0) red[wave][0] = dsum;
                __syncthreads();
                if (threadIdx.x == 0)
                    dcpart[(r * a.C + c) * gridDim.x + blockIdx.x] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
            }
        }
        if (par) {
            __syncthreads();                         // red / tot free again
            // (os_bwd_kernel of oversampled.hip ends alike: one shared function changed the code of both kernels)
#pragma unroll
            for (int j = 0; j < NA; ++j) {
                if (j < nsum) {
                    const float s = wave_sum(acc[j]);
                    if (lane == 0) red[wave][j] = s;
                }
            }
            __syncthreads();
            if ((int)threadIdx.x < nsum) {
                const int j = threadIdx.x;
                float s = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
                if (MODE == GFX_WS_PIECEWISE) {
                    if (j == 2) s *= q.ap;
                    if (j == 3) s *= q.an;
                    if (j == 4) s *= q.kn * (1.0f - q.kn);
                    if (j == 5) s *= q.kp * (1.0f - q.kp);
                }
                if (POLY && j >= 2) {                // raw sums of G f(B_k) first: the output sum needs them
                    if (j == 2) s *= use_tanh ? tanhf(1.0f) : 1.0f;
                    tot[j] = s;
                }
                if (!POLY || j < 2) tot[j] = s;
            }
            __syncthreads();
            if ((int)threadIdx.x < nsum) {
                const int j = threadIdx.x;
                float s = tot[j];
                if (POLY) {
                    if (j < 2) {                     // sum G s(u) = sum_k w_k sum G f(B_k)
                        float gys = 0.0f;
                        for (int k = 0; k < a.K; ++k) gys += sw[k] * tot[2 + k];
                        s = j == 0 ? s - inv * gys : gys;
                    } else {
                        s *= 1.0f - sw[j - 2] * sw[j - 2];
                    }
                }
                part[(r * a.NS + j) * gridDim.x + blockIdx.x] = s;
            }
        }
    }
}

// a row's npart partials of every sum -> the parameter gradients, a row-channel's ndc partials -> its mean input gradient:
// in double, in a fixed order.  For the streaming backward above (both counts its grid.x) and for the oversampled tile
// backward (C ntiles and ntiles).
__global__ __launch_bounds__(256) void ws_bwd_finish_kernel(const float* __restrict__ part, const float* __restrict__ dcpart,
                                                            float* __restrict__ gmean, float* __restrict__ g_pre,
                                                            float* __restrict__ g_post, float* __restrict__ g_p0,
                                                            float* __restrict__ g_p1, int64_t R, int C, int64_t L, int NS,
                                                            int64_t npart, int64_t ndc, int mode, int K) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    if (part) {
        for (int64_t i = tid; i < R * NS; i += nthr) {
            const int64_t r = i / NS;
            const int j = (int)(i - r * NS);
            float* dst = nullptr;
            if (j == 0) dst = g_pre ? g_pre + r : nullptr;
            else if (j == 1) dst = g_post ? g_post + r : nullptr;
            else if (mode == GFX_WS_TANH) dst = (g_p0 && j == 2) ? g_p0 + r : nullptr;
            else if (mode == GFX_WS_PIECEWISE) dst = j < 4 ? (g_p0 ? g_p0 + 2 * r + (j - 2) : nullptr) : (g_p1 ? g_p1 + 2 * r + (j - 4) : nullptr);
            else dst = g_p0 ? g_p0 + r * K + (j - 2) : nullptr;
            if (!dst) continue;
            double s = 0.0;
            for (int64_t b = 0; b < npart; ++b) s += (double)part[i * npart + b];
            *dst = (float)s;
        }
    }
    if (dcpart) {
        for (int64_t i = tid; i < R * C; i += nthr) {
            double s = 0.0;
            for (int64_t b = 0; b < ndc; ++b) s += (double)dcpart[i * ndc + b];
            gmean[i] = (float)(s / (double)L);
        }
    }
}

int ws_bwd_finish(const WsBwdSpace& s, const WsGrads& g, int64_t R, int64_t C, int64_t L, int64_t K, int64_t npart, int64_t ndc,
                  int mode, hipStream_t stream) {
    if (!s.part && !s.dcpart) return GFX_OK;
    const int NS = ws_nsums(K);
    const int64_t items = R * (NS > (int)C ? NS : (int)C);
    const int64_t nb = (items + 255) / 256;
    return launch(ws_bwd_finish_kernel, dim3((unsigned)(nb > 65535 * 16 ? 65535 * 16 : nb)), dim3(256), 0, stream, s.part,
                  s.dcpart, s.gmean, g.pre, g.post, g.p0, g.p1, R, (int)C, L, NS, npart, ndc, mode, (int)K);
}

// the adjoint of the centring x - mean(x): gx -= mean(gx) per row-channel
__global__ __launch_bounds__(256) void ws_sub_mean_kernel(float* __restrict__ gx, gfx_rowmap_t omap,
                                                          const float* __restrict__ gmean, int64_t R, int C, int64_t L,
                                                          int vec) {
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
        for (int c = 0; c < C; ++c) {
            const float m = gmean[r * C + c];
            float* outr = gx + row_off(omap, r, c);
            const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
            int64_t n0 = tid;
            if (vec) {
                using f4 = float __attribute__((ext_vector_type(4)));
                for (int64_t i = tid; i < L / 4; i += nthr) reinterpret_cast<f4*>(outr)[i] -= m;
                n0 = (L & ~int64_t(3)) + tid;
            }
            for (int64_t n = n0; n < L; n += nthr) outr[n] -= m;
        }
    }
}

}  // namespace gfx

extern "C" {

size_t gfx_waveshaper_bwd_ws_bytes(int64_t R, int64_t C, int64_t L, int64_t K) {
    if (R <= 0 || C <= 0 || L <= 0 || K < 0 || K > WS_MAX_K) return 0;
    const size_t bx = (size_t)ws_blocks(L);
    return sizeof(float) * ws_bwd_floats(R, C, K, bx, bx);
}

int gfx_waveshaper_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R, int64_t C,
                           int64_t L, int mode, int use_tanh, int inverse_post_gain, const float* log_pre_gain,
                           const float* log_post_gain, const float* p0, const float* p1, int64_t K, const float* dc,
                           float* gx, gfx_rowmap_t omap, float* g_log_pre_gain, float* g_log_post_gain, float* g_p0,
                           float* g_p1, void* ws, size_t ws_bytes, void* stream) {
    if (!x || !gy || R <= 0 || C <= 0 || L <= 0 || R > 0x7fffffffLL || xmap.inner <= 0 || gmap.inner <= 0) return GFX_EINVAL;
    if (ws_check_shaper(mode, inverse_post_gain, log_pre_gain, p0, p1, K) != GFX_OK) return GFX_EINVAL;
    const WsGrads grads{g_log_pre_gain, g_log_post_gain, g_p0, g_p1};
    if (ws_check_grads(grads, gx, mode, inverse_post_gain, log_pre_gain, log_post_gain, p0) != GFX_OK) return GFX_EINVAL;
    const bool want_par = grads.any();
    if (gx && (map_negative(xmap) || map_negative(gmap))) return GFX_EINVAL;
    if (!grad_out_ok(gx, omap, x, xmap, gy, gmap, R, C, L)) return GFX_EINVAL;
    const bool center = dc && gx;
    const int64_t bx = ws_blocks(L);
    WsBwdSpace sp;
    const int rc = ws_bwd_carve(ws, ws_bytes, R, C, K, (size_t)bx, (size_t)bx, want_par, center, sp);
    if (rc != GFX_OK) return rc;
    WsBwdArgs a;
    a.xmap = xmap; a.gmap = gmap; a.omap = gx ? omap : xmap; a.R = R; a.L = L; a.C = (int)C; a.K = (int)K; a.NS = ws_nsums(K);
    a.use_tanh = use_tanh; a.inverse_post = inverse_post_gain; a.want_par = want_par;
    const int vec = aligned16(x) && aligned16(gy) && map_vec(xmap) && map_vec(gmap) && (!gx || (aligned16(gx) && map_vec(omap)));
    const dim3 grid((unsigned)bx, (unsigned)(R > 65535 ? 65535 : R));
    hipStream_t st = (hipStream_t)stream;
    const int lrc = with_ws_mode(mode, [&](auto m) {
        return launch(waveshaper_bwd_kernel<decltype(m)::value>, grid, dim3(256), 0, st, x, gy, gx, log_pre_gain, log_post_gain, p0,
                      p1, dc, sp.part, sp.dcpart, a, vec);
    });
    if (lrc != GFX_OK) return GFX_ELAUNCH;
    if (ws_bwd_finish(sp, grads, R, C, L, K, bx, bx, mode, st) != GFX_OK) return GFX_ELAUNCH;
    if (center)
        return launch(ws_sub_mean_kernel, grid, dim3(256), 0, st, gx, omap, sp.gmean, R, (int)C, L,
                      (int)(aligned16(gx) && map_vec(omap)));
    return GFX_OK;
}

}  // extern "C"

// ---- small inverse real DFT (parameter-side front-ends) --------------------------------------------------------------
// y = irfft(X, n) for short transforms of ANY length n <= 8192 as a direct sum: the zero-phase FIR design
// (core/fir.py:20-27: n = 2 bins - 1 = 2047, odd) and the surrogate delay's soft impulse (core/delay.py:73-76).  These
// are per-node front-ends (R x ~1024 bins), where a direct O(n K) sum with the twiddles e^{2 pi i j / n} tabulated
// in LDS (phase index k m mod n carried incrementally: exact) is a few microseconds per row and replaces the FFT library.
//   y[(m + roll) mod n] = w[(m + roll) mod n] / n * ( Re X[0] + 2 sum_{0<k<n/2} Re(X[k] e^{2 pi i k m / n})
//                                                      + [n even] Re X[n/2] (-1)^m )
namespace gfx {

__global__ __launch_bounds__(256) void irdft_kernel(const float* __restrict__ X, int is_real, float* __restrict__ y,
                                                    int K, int n, int roll, const float* __restrict__ window) {
    extern __shared__ float2 tab[];                       // tab[j] = e^{2 pi i j / n}, then the row's spectrum
    float2* spec = tab + n;
    const int64_t row = blockIdx.x;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double s, c;                                       // in double: j / n is not exact in float (6e-7 rad at n = 4001)
        sincospi(2.0 * (double)j / (double)n, &s, &c);
        tab[j] = make_float2((float)c, (float)s);
    }
    for (int k = threadIdx.x; k < K; k += blockDim.x)
        spec[k] = is_real ? make_float2(X[row * K + k], 0.0f)
                          : make_float2(X[(row * K + k) * 2], X[(row * K + k) * 2 + 1]);
    __syncthreads();
    const int half = n / 2;
    const bool even = (n & 1) == 0;
    const int kmax = even ? half - 1 : half;              // bins with weight 2
    for (int m = threadIdx.x; m < n; m += blockDim.x) {
        double acc = 0.0;                                  // thousands of terms: accumulate in double (a tiny kernel)
        int idx = 0;
        for (int k = 1; k <= kmax; ++k) {
            idx += m;
            if (idx >= n) idx -= n;
            const float2 w = tab[idx], x = spec[k];
            acc += (double)x.x * (double)w.x - (double)x.y * (double)w.y;
        }
        float v = (float)((double)spec[0].x + 2.0 * acc);
        if (even) v += (m & 1) ? -spec[half].x : spec[half].x;
        int o = m + roll;
        o -= (o >= n) ? n : 0;
        v /= (float)n;
        y[row * n + o] = window ? v * window[o] : v;
    }
}

// X[k] = sum_m x[m] e^{-2 pi i k m / n}, k = 0 .. n/2: the forward twin (rfft) of irdft_kernel, same table, same exact
// phase index, double accumulation.  The gradient of an inverse real DFT is this transform of the incoming gradient
// (autograd.IrdftFn, autograd.FsmFirFn.backward): with it the parameter-side front-ends of the training path stay off the
// FFT library for every length the inverse kernel covers.
// One workgroup per (row, 32 bins): 8 lanes share a bin, each sums every 8th sample, then a shuffle tree -- the rows are
// few (one per filter), so the work of a row has to spread over many workgroups (a first cut with one workgroup per row
// and the whole sum over m in one thread took 0.65 ms for 32 filters of 4001 taps, all of it latency).
__global__ __launch_bounds__(256) void rdft_kernel(const float* __restrict__ x, float* __restrict__ X, int K, int n) {
    extern __shared__ float2 tab[];                       // tab[j] = e^{2 pi i j / n}, then the row's samples
    float* sig = reinterpret_cast<float*>(tab + n);
    const int64_t row = blockIdx.y;
    for (int j = threadIdx.x; j < n; j += blockDim.x) {
        double s, c;
        sincospi(2.0 * (double)j / (double)n, &s, &c);
        tab[j] = make_float2((float)c, (float)s);
        sig[j] = x[row * n + j];
    }
    __syncthreads();
    const int part = threadIdx.x & 7;
    const int k = blockIdx.x * 32 + (threadIdx.x >> 3);
    double re = 0.0, im = 0.0;
    if (k < K) {
        int idx = (int)(((int64_t)k * part) % n);          // k m mod n for m = part, part + 8, ...
        const int step = (int)(((int64_t)k * 8) % n);
        for (int m = part; m < n; m += 8) {
            const float2 w = tab[idx];
            re += (double)sig[m] * (double)w.x;
            im -= (double)sig[m] * (double)w.y;
            idx += step;
            if (idx >= n) idx -= n;
        }
    }
#pragma unroll
    for (int o = 4; o > 0; o >>= 1) {                       // the 8 lanes of a bin are adjacent
        re += __shfl_down(re, o, 8);
        im += __shfl_down(im, o, 8);
    }
    if (k < K && part == 0) {
        X[(row * K + k) * 2] = (float)re;
        X[(row * K + k) * 2 + 1] = (float)im;
    }
}

}  // namespace gfx

extern "C" int gfx_rdft_f32(const float* x, float* X, int64_t rows, int64_t K, int64_t n, void* stream) {
    if (!x || !X || rows <= 0 || rows > 65535 || n < 1 || n > 8192 || K != n / 2 + 1) return GFX_EINVAL;
    const size_t lds = (size_t)n * (sizeof(float2) + sizeof(float));
    return gfx::launch(gfx::rdft_kernel, dim3((unsigned)((K + 31) / 32), (unsigned)rows), dim3(256), lds, (hipStream_t)stream, x, X,
                       (int)K, (int)n);
}

extern "C" int gfx_irdft_f32(const float* X, int is_real, float* y, int64_t rows, int64_t K, int64_t n, int64_t roll,
                             const float* window, void* stream) {
    if (!X || !y || rows <= 0 || rows > 0x7fffffffLL || n < 1 || n > 8192 || K != n / 2 + 1 || roll < 0 || roll >= n)
        return GFX_EINVAL;
    const size_t lds = (size_t)(n + K) * sizeof(float2);
    return gfx::launch(gfx::irdft_kernel, dim3((unsigned)rows), dim3(256), lds, (hipStream_t)stream, X, is_real, y, (int)K, (int)n,
                       (int)roll, window);
}
