// Feedback delay -- echo, ping-pong (gfx950): a recursive chunk walk each way and a tile-parallel sum kernel for the
// parameter gradients.  For a row r of C <= 2 channels, c, c' < C:
//
//     i_c = floor(delay[r,c]),  f_c = delay[r,c] - i_c                     float32; 64 <= delay <= max_delay <= 65536
//     s_c[n] = (1 - f_c) w_c[n - i_c] + f_c w_c[n - i_c - 1]               the line's output
//     q_c[n] = (1 - a[r,c]) s_c[n] + a[r,c] q_c[n - 1]                     the loop's one-pole damping, 0 <= a < 1
//     w_c[n] = x_c[n] + sum_c' F[r,c,c'] q_c'[n]                           what enters the line
//     y_c[n] = dry[r] x_c[n] + wet[r] q_c[n]
//
// with w and q zero, or the carried state, below the row's start.  One workgroup of 256 lanes owns a row with all of its
// channels and walks it in chunks of K = min(min_c i_c, FBDELAY_CHUNK) samples: inside a chunk every s reads only what
// earlier chunks wrote, so the chunk is a gather, one first-order scan with a constant coefficient per channel (lane t
// holds samples 4 t .. 4 t + 3 of the chunk; a wave scan of the affine maps q -> A q + B; the cross-wave carry through
// LDS, and no LDS at all while K <= 256, when one wave holds the chunk) and an elementwise mix.  w lives in a (R, C, L)
// workspace: a chunk reads back what the same workgroup stored before a __syncthreads(), and no other workgroup reads a
// row's line within the launch.  The next chunk's x is loaded before the scan.
//
// The backward (a call without a state) is the same loop backwards in time with F transposed:
//     lambda_c[n] = (1 - f_c) mu_c[n + i_c] + f_c mu_c[n + i_c + 1]
//     zeta_c[n]   = wet gy_c[n] + sum_c' F[c',c] lambda_c'[n]
//     mu_c[n]     = (1 - a_c) zeta_c[n] + a_c mu_c[n + 1]
//     gx_c[n]     = dry gy_c[n] + lambda_c[n]
// mu is stored in the workspace the way w is.  The parameter gradients are plain sums over n once mu exists
// (fb_bwd_par_kernel: tiles of FB_TILE samples, double accumulators, a fixed-order workgroup reduction, per-tile partials
// in the workspace; tile_sums_finish_kernel of common.hpp, with FbSlots, adds them per row in a fixed order).  No atomics
// anywhere: equal bits from run to run, and a row's result does not depend on the other rows.  Outside the contract
// (max_c sum_c' |F[c,c']| < 1, 0 <= a < 1, the delay's range; NaNs included) the delay is clamped before it is split, so
// every access stays inside its buffer; the values are unspecified.
#include "common.hpp"

namespace gfx {

constexpr int FB_THREADS = 256;
constexpr int FB_WAVES = FB_THREADS / 64;
constexpr int FB_PER = 4;                          // consecutive samples of a chunk per lane
constexpr int FB_CHUNK = FB_THREADS * FB_PER;      // FBDELAY_CHUNK of ops.py
constexpr int FB_MIN_DELAY = 64;
constexpr int FB_MAX_DELAY = 65536;
constexpr int FB_TILE = 2048;                      // samples of a row per workgroup of the sum kernel
constexpr int FB_MAX_C = 2;

struct FbArgs {
    gfx_rowmap_t xmap, ymap, gmap;                 // x, the output (y or gx), gy
    int64_t L, ntiles;
    int Dmax, S;                                   // S = Dmax + 1 carried samples of w
};

// the delay of a row-channel -> its integer part (64 .. Dmax) and fraction (a NaN comes out as 64)
__device__ __forceinline__ int fb_split(float delay, int Dmax, float& f) {
    const float d = fminf(fmaxf(delay, (float)FB_MIN_DELAY), (float)Dmax);
    const float fl = floorf(d);
    f = d - fl;
    return (int)fl;
}

// inclusive scan over the wave of the affine maps q -> A q + B, the lower lanes applied first
__device__ __forceinline__ void fb_wave_scan(float& A, float& B, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float Ap = __shfl_up(A, o, 64), Bp = __shfl_up(B, o, 64);
        if (lane >= o) {
            B = fmaf(A, Bp, B);
            A *= Ap;
        }
    }
}

// v[c][p] <- the one-pole (1 - a_c) v + a_c (the sample before) over the chunk's samples in lane order; `cnt` of this
// lane's FB_PER samples exist.  carry[c]: the value before the chunk's first sample in, the chunk's last value out (in
// every lane; with `single`, when wave 0 alone holds samples, in wave 0 only and without a barrier).  `xw` is the
// 2 x FB_WAVES x C x 2 floats of the cross-wave exchange, `buf` alternates from chunk to chunk.
template <int C>
__device__ __forceinline__ void fb_chunk_scan(float (&v)[C][FB_PER], const float (&a)[C], int cnt, float (&carry)[C],
                                              bool single, float* xw, int buf) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float A[C], B[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float oma = 1.0f - a[c];
        float l = 0.0f, m = 1.0f;
#pragma unroll
        for (int p = 0; p < FB_PER; ++p)
            if (p < cnt) {
                l = fmaf(a[c], l, oma * v[c][p]);
                m *= a[c];
                v[c][p] = l;
            }
        A[c] = m;
        B[c] = l;
        fb_wave_scan(A[c], B[c], lane);
    }
    float in[C];                                   // the value before this wave's first sample
    if (single) {
#pragma unroll
        for (int c = 0; c < C; ++c) {
            in[c] = carry[c];
            carry[c] = fmaf(__shfl(A[c], 63, 64), carry[c], __shfl(B[c], 63, 64));
        }
    } else {
        float* mine = xw + buf * (FB_WAVES * C * 2);
        if (lane == 63) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                mine[(wave * C + c) * 2] = A[c];
                mine[(wave * C + c) * 2 + 1] = B[c];
            }
        }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float q = carry[c];
            in[c] = q;
#pragma unroll
            for (int w = 0; w < FB_WAVES; ++w) {
                if (w == wave) in[c] = q;
                q = fmaf(mine[(w * C + c) * 2], q, mine[(w * C + c) * 2 + 1]);
            }
            carry[c] = q;
        }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) {
        const float Ae = __shfl_up(A[c], 1, 64), Be = __shfl_up(B[c], 1, 64);
        const float P = lane == 0 ? in[c] : fmaf(Ae, in[c], Be);       // the value before this lane's first sample
        float ap = a[c];
#pragma unroll
        for (int p = 0; p < FB_PER; ++p) {
            if (p < cnt) v[c][p] = fmaf(ap, P, v[c][p]);
            ap *= a[c];
        }
    }
}

// One workgroup per row.  `w`: the (R, C, L) line, written and read back here (no __restrict__: see the head of the file).
template <int C>
__global__ __launch_bounds__(FB_THREADS) void fb_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, float* w,
                                                            float* __restrict__ qsig, const float* __restrict__ delay,
                                                            const float* __restrict__ damping, const float* __restrict__ fbm,
                                                            const float* __restrict__ dry, const float* __restrict__ wet,
                                                            const float* __restrict__ zi, const float* __restrict__ q_in,
                                                            float* __restrict__ q_out, FbArgs g) {
    __shared__ float xw[2 * FB_WAVES * C * 2];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x, L = g.L;
    const int S = g.S;
    int i[C], K = FB_CHUNK;
    float f[C], a[C], F[C][C], carry[C];
    const float* xrow[C];
    const float* zrow[C];
    float *yrow[C], *wrow[C], *qrow[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        i[c] = fb_split(delay[r * C + c], g.Dmax, f[c]);
        K = i[c] < K ? i[c] : K;
        a[c] = damping[r * C + c];
#pragma unroll
        for (int d = 0; d < C; ++d) F[c][d] = fbm[(r * C + c) * C + d];
        carry[c] = q_in ? q_in[r * C + c] : 0.0f;
        xrow[c] = x + row_off(g.xmap, r, c);
        yrow[c] = y + row_off(g.ymap, r, c);
        wrow[c] = w + (r * C + c) * L;
        qrow[c] = qsig ? qsig + (r * C + c) * L : nullptr;
        zrow[c] = zi ? zi + (r * C + c) * (int64_t)S : nullptr;
    }
    const float dr = dry[r], we = wet[r];
    const bool single = K <= 64 * FB_PER;
    float xs[C][FB_PER];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < FB_PER; ++p) {
            const int64_t n = FB_PER * t + p;
            xs[c][p] = (FB_PER * t + p < K && n < L) ? xrow[c][n] : 0.0f;
        }
    int buf = 0;
    for (int64_t n0 = 0; n0 < L; n0 += K, buf ^= 1) {
        const int Kc = (int)(L - n0 < K ? L - n0 : K);
        int cnt = Kc - FB_PER * t;
        cnt = cnt < 0 ? 0 : cnt > FB_PER ? FB_PER : cnt;
        const int64_t nf = n0 + FB_PER * t;        // this lane's first sample
        float v[C][FB_PER];
        if (cnt > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float line[FB_PER + 1];            // w[nf - i - 1 + m]
#pragma unroll
                for (int m = 0; m <= FB_PER; ++m) {
                    const int64_t k = nf - i[c] - 1 + m;     // < n0: m <= cnt with i >= K, beyond that clamped below
                    const int64_t kk = k < n0 ? k : n0 - 1;
                    float val = m <= cnt ? wrow[c][kk > 0 ? kk : 0] : 0.0f;
                    if (kk < 0) val = zrow[c] ? zrow[c][S + kk] : 0.0f;
                    line[m] = val;
                }
#pragma unroll
                for (int p = 0; p < FB_PER; ++p) v[c][p] = fmaf(f[c], line[p], (1.0f - f[c]) * line[p + 1]);
            }
        } else {
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int p = 0; p < FB_PER; ++p) v[c][p] = 0.0f;
        }
        float xn[C][FB_PER];                       // the next chunk's x, in flight under the scan
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) {
                const int64_t n = nf + K + p;
                xn[c][p] = (FB_PER * t + p < K && n < L) ? xrow[c][n] : 0.0f;
            }
        if (!single || t < 64) fb_chunk_scan<C>(v, a, cnt, carry, single, xw, buf);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) {
                if (p >= cnt) continue;
                float wv = xs[c][p];
#pragma unroll
                for (int d = 0; d < C; ++d) wv = fmaf(F[c][d], v[d][p], wv);
                wrow[c][nf + p] = wv;
                yrow[c][nf + p] = fmaf(we, v[c][p], dr * xs[c][p]);
                if (qrow[c]) qrow[c][nf + p] = v[c][p];
            }
        __syncthreads();                           // the chunk's w is in memory before the next gather
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) xs[c][p] = xn[c][p];
    }
    if (q_out && t == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) q_out[r * C + c] = carry[c];
    }
}

// The adjoint walk: n descending, lane t holds samples top - 1 - 4 t - p.  `mu`: the (R, C, L) line of the adjoint.
template <int C>
__global__ __launch_bounds__(FB_THREADS) void fb_bwd_walk_kernel(const float* __restrict__ gy, float* __restrict__ gx, float* mu,
                                                                 const float* __restrict__ delay, const float* __restrict__ damping,
                                                                 const float* __restrict__ fbm, const float* __restrict__ dry,
                                                                 const float* __restrict__ wet, FbArgs g) {
    __shared__ float xw[2 * FB_WAVES * C * 2];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x, L = g.L;
    int i[C], K = FB_CHUNK;
    float f[C], a[C], F[C][C], carry[C];
    const float* grow[C];
    float *orow[C], *mrow[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        i[c] = fb_split(delay[r * C + c], g.Dmax, f[c]);
        K = i[c] < K ? i[c] : K;
        a[c] = damping[r * C + c];
#pragma unroll
        for (int d = 0; d < C; ++d) F[c][d] = fbm[(r * C + c) * C + d];
        carry[c] = 0.0f;
        grow[c] = gy + row_off(g.gmap, r, c);
        orow[c] = gx ? gx + row_off(g.ymap, r, c) : nullptr;
        mrow[c] = mu + (r * C + c) * L;
    }
    const float dr = dry[r], we = wet[r];
    const bool single = K <= 64 * FB_PER;
    float gs[C][FB_PER];
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
        for (int p = 0; p < FB_PER; ++p) {
            const int64_t n = L - 1 - FB_PER * t - p;
            gs[c][p] = (FB_PER * t + p < K && n >= 0) ? grow[c][n] : 0.0f;
        }
    int buf = 0;
    for (int64_t top = L; top > 0; top -= K, buf ^= 1) {
        const int Kc = (int)(top < K ? top : K);
        int cnt = Kc - FB_PER * t;
        cnt = cnt < 0 ? 0 : cnt > FB_PER ? FB_PER : cnt;
        const int64_t nf = top - 1 - FB_PER * t;   // this lane's first (highest) sample
        float lam[C][FB_PER], v[C][FB_PER];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float line[FB_PER + 1];                // mu[nf + i + 1 - m]
#pragma unroll
            for (int m = 0; m <= FB_PER; ++m) {
                const int64_t k = nf + i[c] + 1 - m;         // >= top: m <= cnt with i >= K
                line[m] = (cnt > 0 && m <= cnt && k >= top && k < L) ? mrow[c][k] : 0.0f;
            }
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) lam[c][p] = fmaf(f[c], line[p], (1.0f - f[c]) * line[p + 1]);
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) {
                float z = we * gs[c][p];
#pragma unroll
                for (int d = 0; d < C; ++d) z = fmaf(F[d][c], lam[d][p], z);
                v[c][p] = z;
            }
        float gn[C][FB_PER];                       // the next chunk's gy
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) {
                const int64_t n = nf - K - p;
                gn[c][p] = (FB_PER * t + p < K && n >= 0) ? grow[c][n] : 0.0f;
            }
        if (!single || t < 64) fb_chunk_scan<C>(v, a, cnt, carry, single, xw, buf);
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) {
                if (p >= cnt) continue;
                mrow[c][nf - p] = v[c][p];
                if (orow[c]) orow[c][nf - p] = fmaf(dr, gs[c][p], lam[c][p]);
            }
        __syncthreads();
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int p = 0; p < FB_PER; ++p) gs[c][p] = gn[c][p];
    }
}

// The tile's share of the parameter gradients, P = 2 + 2 C + C C doubles at part[item P]:
// dry | wet | delay[C] | damping[C] (without its 1 / (1 - a)) | feedback[C, C].
template <int C>
__global__ __launch_bounds__(FB_THREADS) void fb_bwd_par_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                const float* __restrict__ q, const float* __restrict__ w,
                                                                const float* __restrict__ mu, const float* __restrict__ delay,
                                                                double* __restrict__ part, FbArgs g) {
    constexpr int P = 2 + 2 * C + C * C;
    __shared__ double red[FB_WAVES][P];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t item = blockIdx.x, L = g.L;
    const int64_t r = item / g.ntiles, tile = item - r * g.ntiles;
    const int64_t n0 = tile * FB_TILE;
    const int left = (int)(L - n0 < FB_TILE ? L - n0 : FB_TILE);
    int i[C];
    float f[C];
    const float* xrow[C];
    const float* grow[C];
#pragma unroll
    for (int c = 0; c < C; ++c) {
        i[c] = fb_split(delay[r * C + c], g.Dmax, f[c]);
        xrow[c] = x + row_off(g.xmap, r, c);
        grow[c] = gy + row_off(g.gmap, r, c);
    }
    double s[P];
#pragma unroll
    for (int k = 0; k < P; ++k) s[k] = 0.0;
    for (int tt = t; tt < left; tt += FB_THREADS) {
        const int64_t n = n0 + tt;
        float qv[C], lam[C];
#pragma unroll
        for (int c = 0; c < C; ++c) qv[c] = q[(r * C + c) * L + n];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float* mrow = mu + (r * C + c) * L;
            const float* wrow = w + (r * C + c) * L;
            const int64_t up = n + i[c], dn = n - i[c];
            const float m0 = up < L ? mrow[up] : 0.0f, m1 = up + 1 < L ? mrow[up + 1] : 0.0f;
            lam[c] = fmaf(f[c], m1, (1.0f - f[c]) * m0);
            const float w0 = dn >= 0 ? wrow[dn] : 0.0f, w1 = dn >= 1 ? wrow[dn - 1] : 0.0f;
            const float sv = fmaf(f[c], w1, (1.0f - f[c]) * w0);
            const float qb = n >= 1 ? q[(r * C + c) * L + n - 1] : 0.0f;
            const double gg = (double)grow[c][n], mm = (double)mrow[n];
            s[0] += gg * (double)xrow[c][n];
            s[1] += gg * (double)qv[c];
            s[2 + c] += mm * ((double)w1 - (double)w0);
            s[2 + C + c] += mm * ((double)qb - (double)sv);
        }
#pragma unroll
        for (int c = 0; c < C; ++c)
#pragma unroll
            for (int d = 0; d < C; ++d) s[2 + 2 * C + c * C + d] += (double)lam[c] * (double)qv[d];
    }
    block_sums<P, FB_WAVES>(s, red, lane, wave, [&](double sum) { part[item * P + t] = sum; });
}

// a row's tile sums -> its parameter gradients (tile_sums_finish_kernel): dry, wet, delay[C], damping[C] with its
// 1 / (1 - a), feedback[C, C]; a null destination is skipped
struct FbSlots {
    const float* damping;
    float *g_delay, *g_damping, *g_feedback, *g_dry, *g_wet;
    int C;
    __device__ float* dest(int64_t r, int64_t slot, double& scale) const {
        if (slot == 0) return g_dry ? g_dry + r : nullptr;
        if (slot == 1) return g_wet ? g_wet + r : nullptr;
        if (slot < 2 + C) return g_delay ? g_delay + r * C + (slot - 2) : nullptr;
        if (slot < 2 + 2 * C) {
            scale = 1.0 / (1.0 - (double)damping[r * C + (slot - 2 - C)]);
            return g_damping ? g_damping + r * C + (slot - 2 - C) : nullptr;
        }
        return g_feedback ? g_feedback + r * C * C + (slot - 2 - 2 * C) : nullptr;
    }
};

// the checks both entries share
static int fb_prepare(const float* x, gfx_rowmap_t xmap, int64_t R, int64_t C, int64_t L, int64_t max_delay, const float* delay,
                      const float* damping, const float* feedback, const float* dry, const float* wet, FbArgs& a) {
    if (!x || !delay || !damping || !feedback || !dry || !wet) return GFX_EINVAL;
    if (R <= 0 || C <= 0 || L <= 0 || C > FB_MAX_C || R > 0x7fffffffLL || xmap.inner <= 0) return GFX_EINVAL;
    if (max_delay < FB_MIN_DELAY || max_delay > FB_MAX_DELAY || L > INT64_MAX / 64 / R) return GFX_EINVAL;
    if (map_negative(xmap)) return GFX_EINVAL;
    a.xmap = a.ymap = a.gmap = xmap;
    a.L = L; a.ntiles = (L + FB_TILE - 1) / FB_TILE;
    a.Dmax = (int)max_delay; a.S = (int)max_delay + 1;
    return GFX_OK;
}

// does the contiguous float range [p, p + n) meet a mapped signal?
static bool fb_meets(const float* p, int64_t n, const float* sig, const gfx_rowmap_t& m, int64_t R, int64_t C, int64_t L) {
    const float *lo, *hi;
    map_span(sig, m, R, C, L, lo, hi);
    return p < hi && lo < p + n;
}

static size_t fb_par_bytes(int64_t R, int64_t C, int64_t L) {
    return sizeof(double) * (size_t)R * (size_t)((L + FB_TILE - 1) / FB_TILE) * (size_t)(2 + 2 * C + C * C);
}

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_fbdelay_ws_bytes(int64_t R, int64_t C, int64_t L) {
    if (R <= 0 || C <= 0 || C > FB_MAX_C || L <= 0 || L > INT64_MAX / 64 / R) return 0;
    return sizeof(float) * (size_t)R * (size_t)C * (size_t)L;
}

int gfx_fbdelay_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L,
                    int64_t max_delay, const float* delay, const float* damping, const float* feedback, const float* dry,
                    const float* wet, const float* zi, const float* q_in, float* zf, float* q_out, float* q, void* ws,
                    size_t ws_bytes, void* stream) {
    FbArgs a;
    if (!y || ymap.inner <= 0) return GFX_EINVAL;
    const int rc = fb_prepare(x, xmap, R, C, L, max_delay, delay, damping, feedback, dry, wet, a);
    if (rc != GFX_OK) return rc;
    if (!zi != !q_in || !zf != !q_out) return GFX_EINVAL;              // a state is its history and the loop filter's last value
    if (map_negative(ymap) || signals_overlap(y, ymap, x, xmap, R, C, L)) return GFX_EINVAL;
    const int64_t nsig = R * C * L;
    if (!history_pair_ok(zi, zf, R, C, a.S)) return GFX_EINVAL;
    if (zi && zf && ranges_meet(q_in, R * C, q_out, R * C)) return GFX_EINVAL;
    const int wrc = workspace_ok(ws, ws_bytes, gfx_fbdelay_ws_bytes(R, C, L), alignof(float));
    if (wrc != GFX_OK) return wrc;
    float* w = static_cast<float*>(ws);
    // the line and the q signal are written while x is read and next to y
    if (fb_meets(w, nsig, x, xmap, R, C, L) || fb_meets(w, nsig, y, ymap, R, C, L)) return GFX_EINVAL;
    if (q && (fb_meets(q, nsig, x, xmap, R, C, L) || fb_meets(q, nsig, y, ymap, R, C, L) || ranges_meet(q, nsig, w, nsig)))
        return GFX_EINVAL;
    a.ymap = ymap;
    hipStream_t st = (hipStream_t)stream;
    auto fwd = C == 1 ? fb_fwd_kernel<1> : fb_fwd_kernel<2>;
    if (launch(fwd, dim3((unsigned)R), dim3(FB_THREADS), 0, st, x, y, w, q, delay, damping, feedback, dry, wet, zi, q_in, q_out,
               a) != GFX_OK)
        return GFX_ELAUNCH;
    if (zf) {
        const gfx_rowmap_t wmap = {R, 0, C * L, L};
        return launch_history_tail(w, wmap, zi, zf, R, C, L, a.S, nullptr, nullptr, st);
    }
    return GFX_OK;
}

size_t gfx_fbdelay_bwd_ws_bytes(int64_t R, int64_t C, int64_t L) {
    if (R <= 0 || C <= 0 || C > FB_MAX_C || L <= 0 || L > INT64_MAX / 64 / R) return 0;
    return fb_par_bytes(R, C, L) + sizeof(float) * (size_t)R * (size_t)C * (size_t)L;
}

int gfx_fbdelay_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, const float* q, const float* w,
                        int64_t R, int64_t C, int64_t L, int64_t max_delay, const float* delay, const float* damping,
                        const float* feedback, const float* dry, const float* wet, float* gx, gfx_rowmap_t gxmap, float* g_delay,
                        float* g_damping, float* g_feedback, float* g_dry, float* g_wet, void* ws, size_t ws_bytes, void* stream) {
    FbArgs a;
    if (!gy || gmap.inner <= 0 || !q || !w) return GFX_EINVAL;
    const int rc = fb_prepare(x, xmap, R, C, L, max_delay, delay, damping, feedback, dry, wet, a);
    if (rc != GFX_OK) return rc;
    const bool params = g_delay || g_damping || g_feedback || g_dry || g_wet;
    if (!gx && !params) return GFX_EINVAL;
    if (map_negative(gmap)) return GFX_EINVAL;
    const int64_t nsig = R * C * L;
    if (!grad_out_ok(gx, gxmap, x, xmap, gy, gmap, R, C, L)) return GFX_EINVAL;
    if (gx && (fb_meets(q, nsig, gx, gxmap, R, C, L) || fb_meets(w, nsig, gx, gxmap, R, C, L))) return GFX_EINVAL;
    const int wrc = workspace_ok(ws, ws_bytes, gfx_fbdelay_bwd_ws_bytes(R, C, L), alignof(double));
    if (wrc != GFX_OK) return wrc;
    if (params && a.ntiles > MAX_GRID_X / R) return GFX_EINVAL;         // grid.x of the sum kernel
    double* part = static_cast<double*>(ws);
    float* mu = reinterpret_cast<float*>(static_cast<char*>(ws) + fb_par_bytes(R, C, L));
    if (gx && fb_meets(mu, nsig, gx, gxmap, R, C, L)) return GFX_EINVAL;
    a.gmap = gmap;
    a.ymap = gx ? gxmap : xmap;
    hipStream_t st = (hipStream_t)stream;
    if (gx || g_delay || g_damping || g_feedback) {                     // (dry and wet need no adjoint line)
        auto walk = C == 1 ? fb_bwd_walk_kernel<1> : fb_bwd_walk_kernel<2>;
        if (launch(walk, dim3((unsigned)R), dim3(FB_THREADS), 0, st, gy, gx, mu, delay, damping, feedback, dry, wet, a) != GFX_OK)
            return GFX_ELAUNCH;
    }
    if (params) {
        if (!(g_delay || g_damping || g_feedback) && hipMemsetAsync(mu, 0, sizeof(float) * (size_t)nsig, st) != hipSuccess)
            return GFX_ELAUNCH;
        auto par = C == 1 ? fb_bwd_par_kernel<1> : fb_bwd_par_kernel<2>;
        if (launch(par, dim3((unsigned)(R * a.ntiles)), dim3(FB_THREADS), 0, st, x, gy, q, w, mu, delay, part, a) != GFX_OK)
            return GFX_ELAUNCH;
        return finish_tile_sums(FbSlots{damping, g_delay, g_damping, g_feedback, g_dry, g_wet, (int)C}, part, R,
                                2 + 2 * C + C * C, a.ntiles, st);
    }
    return GFX_OK;
}

}  // extern "C"
