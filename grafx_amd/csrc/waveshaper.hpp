// The per-sample math of the memoryless waveshapers, shared by the streaming kernels (nonlinear.hip) and the oversampled
// tile kernels (oversampled.hip): the row's constants, the shape s with its gains, one backward step of NV samples with the
// terms of every parameter sum, and on the host the argument checks and the workspace layout that the entries of both
// files share.
#pragma once
#include <type_traits>

#include "common.hpp"

namespace gfx {

constexpr int WS_MAX_K = 32;

struct WsRow {
    float pre, post, dc;
    float b, tb;                    // tanh: bias, tanh(bias)
    float kp, kn, gp, gn, ap, an, bp, bn;  // piecewise
    const float* w;                 // polynomial weights (already tanh'ed), in LDS: a run-time-indexed register
};                                  // array would live in scratch memory

template <int MODE>
__device__ __forceinline__ float shape(float x, const WsRow& q, int K, bool use_tanh) {
    const float u = (x - q.dc) * q.pre;
    float y;
    if (MODE == GFX_WS_TANH) {
        y = tanhf(u + q.b) - q.tb;
    } else if (MODE == GFX_WS_PIECEWISE) {
        if (u > q.kp)
            y = q.ap * tanhf(q.gp * (u - q.kp)) + q.bp;
        else if (u < -q.kn)
            y = q.an * tanhf(q.gn * (u + q.kn)) + q.bn;
        else
            y = tanhf(u);
    } else if (MODE == GFX_WS_POWER) {
        float p = 1.0f;
        y = q.w[0] * (use_tanh ? tanhf(1.0f) : 1.0f);
        for (int k = 1; k < K; ++k) {
            p *= u;
            y += q.w[k] * (use_tanh ? tanhf(p) : p);
        }
    } else {  // Chebyshev
        float t0 = 1.0f, t1 = u;
        y = q.w[0] * (use_tanh ? tanhf(1.0f) : 1.0f);
        if (K > 1) y += q.w[1] * (use_tanh ? tanhf(u) : u);
        for (int k = 2; k < K; ++k) {
            const float t2 = 2.0f * u * t1 - t0;
            y += q.w[k] * (use_tanh ? tanhf(t2) : t2);
            t0 = t1;
            t1 = t2;
        }
    }
    return y * q.post;
}

// the row's constants, as both the forward and the backward kernel use them (polynomial weights: tanh'ed, into LDS)
template <int MODE>
__device__ __forceinline__ void ws_row_setup(WsRow& q, float* sw, int64_t r, int K, int inverse_post,
                                             const float* __restrict__ log_pre, const float* __restrict__ log_post,
                                             const float* __restrict__ p0, const float* __restrict__ p1) {
    q.w = sw;
    q.pre = log_pre ? expf(log_pre[r]) : 1.0f;
    q.post = inverse_post ? 1.0f / q.pre : (log_post ? expf(log_post[r]) : 1.0f);
    q.b = q.tb = 0.0f;
    if (MODE == GFX_WS_TANH && p0) {
        q.b = p0[r];
        q.tb = tanhf(q.b);
    }
    if (MODE == GFX_WS_PIECEWISE) {
        // nonlinear.py:163-166: threshold splits as (kn, kp), hardness as (gp, gn)
        q.gp = expf(p0[2 * r]);
        q.gn = expf(p0[2 * r + 1]);
        q.kn = 1.0f / (1.0f + expf(-p1[2 * r]));
        q.kp = 1.0f / (1.0f + expf(-p1[2 * r + 1]));
        q.bp = tanhf(q.kp);
        q.bn = -tanhf(q.kn);
        q.ap = (1.0f - q.bp) / q.gp;
        q.an = (1.0f + q.bn) / q.gn;
    }
    if (MODE == GFX_WS_POWER || MODE == GFX_WS_CHEBYSHEV) {
        __syncthreads();  // previous row's readers are done
        if ((int)threadIdx.x < K) sw[threadIdx.x] = tanhf(p0[r * K + threadIdx.x]);
        __syncthreads();
    }
}

// slots of a row's sums: 0 = d/d log_pre, 1 = d/d log_post, 2.. = the mode's own
template <int MODE>
struct WsAcc {
    static constexpr int N = MODE == GFX_WS_TANH ? 3 : MODE == GFX_WS_PIECEWISE ? 6 : 2 + WS_MAX_K;
};

static inline int ws_nsums(int64_t K) { return K > 0 ? 2 + (int)K : 6; }

// NV samples of one row-channel: their input gradient into go[], their terms onto the thread's sums acc[] (every index a
// compile-time constant after unrolling: a run-time-indexed accumulator array would live in scratch memory)
template <int MODE, int NV>
__device__ __forceinline__ void bwd_samples(const float (&xs)[NV], const float (&gs)[NV], float (&go)[NV], const WsRow& q,
                                            int K, bool use_tanh, float inv, bool par, float (&acc)[WsAcc<MODE>::N]) {
    if (MODE == GFX_WS_TANH) {
        const float db = 1.0f - q.tb * q.tb;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float u = (xs[j] - q.dc) * q.pre, G = gs[j] * q.post;
            const float th = tanhf(u + q.b), d = 1.0f - th * th, s = th - q.tb;
            go[j] = G * d * q.pre;
            if (par) {
                acc[0] += G * (d * u - inv * s);
                acc[1] += G * s;
                acc[2] += G * (d - db);
            }
        }
    } else if (MODE == GFX_WS_PIECEWISE) {
        // hi: y = ap tanh(gp (u - kp)) + bp,  ap = (1 - tanh kp) / gp   -> d/d log gp = ap (a d - t),  a = gp (u - kp)
        //     d/d kp = sech^2(kp) (1 - t / gp) - (1 - bp) d;   lo mirrors it with kn, gn;   (acc[2..5] are scaled by
        //     ap, an, kn (1 - kn), kp (1 - kp) when the partials are written)
        const float skp = 1.0f - q.bp * q.bp, skn = 1.0f - q.bn * q.bn, rgp = 1.0f / q.gp, rgn = 1.0f / q.gn;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            const float u = (xs[j] - q.dc) * q.pre, G = gs[j] * q.post;
            float s, sp;
            if (u > q.kp) {
                const float a = q.gp * (u - q.kp), t = tanhf(a), d = 1.0f - t * t;
                s = q.ap * t + q.bp;
                sp = (1.0f - q.bp) * d;
                if (par) {
                    acc[2] += G * (a * d - t);
                    acc[5] += G * (skp * (1.0f - t * rgp) - sp);
                }
            } else if (u < -q.kn) {
                const float a = q.gn * (u + q.kn), t = tanhf(a), d = 1.0f - t * t;
                s = q.an * t + q.bn;
                sp = (1.0f + q.bn) * d;
                if (par) {
                    acc[3] += G * (a * d - t);
                    acc[4] += G * (sp - skn * (1.0f + t * rgn));
                }
            } else {
                s = tanhf(u);
                sp = 1.0f - s * s;
            }
            go[j] = G * sp * q.pre;
            if (par) {
                acc[0] += G * (sp * u - inv * s);
                acc[1] += G * s;
            }
        }
    } else {
        // k outermost, unrolled to the bound: the recurrences' state and the sums stay in registers.  Chebyshev: T_k and
        // U_(k-1) by the same three-term recurrence (T_k' = k U_(k-1)), started one step early so that k = 1 needs no case.
        float u[NV], G[NV], sp[NV], t0[NV], t1[NV], v0[NV], v1[NV];
        float a0 = 0.0f;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            u[j] = (xs[j] - q.dc) * q.pre;
            G[j] = gs[j] * q.post;
            sp[j] = 0.0f;
            t0[j] = u[j]; t1[j] = 1.0f;      // T_(-1) = T_1 = u, T_0 = 1   (power: t1 = u^(k-1))
            v0[j] = -1.0f; v1[j] = 0.0f;     // U_(-2) = -1, U_(-1) = 0
            a0 += G[j];
        }
        if (par) acc[2] += a0;               // (times f(1) when the partials are written)
#pragma unroll
        for (int k = 1; k < WS_MAX_K; ++k) {
            if (k < K) {
                const float wk = q.w[k];
                float a = 0.0f;
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    float B, Bp;
                    if (MODE == GFX_WS_POWER) {
                        Bp = (float)k * t1[j];
                        B = t1[j] * u[j];
                        t1[j] = B;
                    } else {
                        B = 2.0f * u[j] * t1[j] - t0[j];
                        const float U = 2.0f * u[j] * v1[j] - v0[j];
                        t0[j] = t1[j]; t1[j] = B;
                        v0[j] = v1[j]; v1[j] = U;
                        Bp = (float)k * U;
                    }
                    float f = B, df = 1.0f;
                    if (use_tanh) {
                        f = tanhf(B);
                        df = 1.0f - f * f;
                    }
                    sp[j] += wk * df * Bp;
                    a += G[j] * f;
                }
                if (par) acc[2 + k] += a;
            }
        }
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            go[j] = G[j] * sp[j] * q.pre;
            if (par) acc[0] += G[j] * sp[j] * u[j];
        }
    }
}

// ---- host side: what the streaming and the oversampled entries check and lay out alike ------------------------------
// the shaper's own arguments; K becomes 0 for the shapers that have no polynomial
static inline int ws_check_shaper(int mode, int inverse_post_gain, const float* log_pre_gain, const float* p0, const float* p1,
                                  int64_t& K) {
    if (mode < GFX_WS_TANH || mode > GFX_WS_CHEBYSHEV) return GFX_EINVAL;
    if (inverse_post_gain && !log_pre_gain) return GFX_EINVAL;
    if (mode == GFX_WS_PIECEWISE && (!p0 || !p1)) return GFX_EINVAL;
    const bool poly = mode == GFX_WS_POWER || mode == GFX_WS_CHEBYSHEV;
    if (poly && (!p0 || K < 1 || K > WS_MAX_K)) return GFX_EINVAL;
    if (!poly) K = 0;
    return GFX_OK;
}

// f(std::integral_constant<int, MODE>{}) for the shaper `mode` (checked by ws_check_shaper), and what it returns: how an
// entry picks the instance of a kernel template, `kernel<decltype(m)::value>`
template <typename F>
static inline int with_ws_mode(int mode, F&& f) {
    switch (mode) {
        case GFX_WS_TANH: return f(std::integral_constant<int, GFX_WS_TANH>{});
        case GFX_WS_PIECEWISE: return f(std::integral_constant<int, GFX_WS_PIECEWISE>{});
        case GFX_WS_POWER: return f(std::integral_constant<int, GFX_WS_POWER>{});
        default: return f(std::integral_constant<int, GFX_WS_CHEBYSHEV>{});
    }
}

struct WsGrads {                 // the parameter gradients a backward entry may be asked for
    float *pre, *post, *p0, *p1;
    bool any() const { return pre || post || p0 || p1; }
};

// something to compute, and no gradient of something that is not there (or, for the post gain under inverse_post_gain, not
// used)
static inline int ws_check_grads(const WsGrads& g, const float* gx, int mode, int inverse_post_gain, const float* log_pre_gain,
                                 const float* log_post_gain, const float* p0) {
    if (!gx && !g.any()) return GFX_EINVAL;
    if ((g.pre && !log_pre_gain) || (g.post && (!log_post_gain || inverse_post_gain)) || (g.p0 && !p0) ||
        (g.p1 && mode != GFX_WS_PIECEWISE))
        return GFX_EINVAL;
    return GFX_OK;
}

// The backward workspace, in floats: npart partials of each of a row's ws_nsums(K) sums, ndc partials of each row-channel's
// sum of gx, the row-channels' means of gx.
struct WsBwdSpace {
    float *part, *dcpart, *gmean;
};
static inline size_t ws_bwd_floats(int64_t R, int64_t C, int64_t K, size_t npart, size_t ndc) {
    const size_t rcs = (size_t)R * (size_t)C;
    return (size_t)R * (size_t)ws_nsums(K) * npart + rcs * ndc + rcs;
}
static inline int ws_bwd_carve(void* ws, size_t ws_bytes, int64_t R, int64_t C, int64_t K, size_t npart, size_t ndc,
                               bool want_par, bool center, WsBwdSpace& s) {
    s.part = s.dcpart = s.gmean = nullptr;
    if (!want_par && !center) return GFX_OK;
    // (alignment 1: these entries have never refused a misaligned workspace)
    const int rc = workspace_ok(ws, ws_bytes, sizeof(float) * ws_bwd_floats(R, C, K, npart, ndc), 1);
    if (rc != GFX_OK) return rc;
    float* w = static_cast<float*>(ws);
    if (want_par) s.part = w;
    if (center) {
        s.dcpart = w + (size_t)R * (size_t)ws_nsums(K) * npart;
        s.gmean = s.dcpart + (size_t)R * (size_t)C * ndc;
    }
    return GFX_OK;
}

// a row's npart partials of every sum -> the parameter gradients, a row-channel's ndc partials -> its mean input gradient
// (ws_bwd_finish_kernel, nonlinear.hip); nothing to do where both part and dcpart are null
int ws_bwd_finish(const WsBwdSpace& s, const WsGrads& g, int64_t R, int64_t C, int64_t L, int64_t K, int64_t npart, int64_t ndc,
                  int mode, hipStream_t stream);

}  // namespace gfx
