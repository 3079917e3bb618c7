// Oversampled (anti-aliased) memoryless waveshapers (gfx950): interpolate by F, shape at the high rate, decimate -- one fused
// tile kernel each way, the F L-sized signals only ever in LDS.  For a row-channel x[0..L):
//
//     xc[k] = x[k] - dc                                  0 <= k < L, zero outside
//     u[p]  = sum_k xc[k] h_up[p + o_up - k F]           0 <= p < F L
//     v[p]  = post s(pre u[p])                           0 <= p < F L, and ZERO outside (not s(0): the polynomial
//     y[m]  = sum_p v[p] h_dn[m F + o_dn - p]            0 <= m < L          shapers have a constant term)
//
// with s, pre, post those of gfx_waveshaper_f32 (waveshaper.hpp).  The adjoint, G = gy:
//
//     gv[p]  = sum_m gy[m] h_dn[m F + o_dn - p]          (an interpolation of gy by the reversed decimator)
//     gu[p]  = gv[p] post s'(pre u[p]) pre               (bwd_samples, with (u[p], gv[p]) in the place of (x, gy))
//     gxc[k] = sum_p gu[p] h_up[p + o_up - k F]          (a decimation by the interpolator as it is)
//
// and the parameter sums are those of the streaming backward over p in [0, F L).
//
// A tile is T = os_tile(F) consecutive base-rate samples of one row-channel, one workgroup of 256 lanes; F T is about 4096.
// Both kernels have the same three stages:
//   1. stage the taps and the span of the base-rate signal(s) under the tile, zeros outside [0, L), dc subtracted inside;
//   2. form the tile's F T + N - 1 high-rate samples (N: the taps of stage 3) into LDS, zeros outside [0, F L);
//   3. decimate them from LDS, one output per lane and pass, and write each output once.
// Interpolation taps sit phase-major as in upfirdn.hip (every phase reversed, padded to J = ceil(N / F) slots, slot 0 used
// under a select where the phase has J - 1 taps).  The high-rate samples sit phase-major too: local sample i at
// (i mod F) pitch + i / F.  In stage 2 a wave works on ONE phase and consecutive quotients, so its taps are one broadcast
// address and its signal reads consecutive words; in stage 3 output t reads word t + j / F of phase j mod F for tap j,
// consecutive across lanes, and the tap is a broadcast again: no bank conflicts at any F (x-major, lanes would sit F words
// apart).  A lane with four items in flight (256 apart) shares each tap among them: 1.25 LDS reads a product, not 2.
// The halo a tile recomputes is (N_up + N_dn) / (F T) of its work, 2 % at F = 4.  Base offsets are 64-bit, everything inside
// the tile 32-bit.
#include "waveshaper.hpp"

namespace gfx {

constexpr int OS_THREADS = 256;
constexpr int OS_MAX_FACTOR = 16;
constexpr int OS_MAX_TAPS = 1024;
constexpr int OS_SPAN = 4096;                    // high-rate samples of a tile, before the halo

static inline int os_tile(int64_t F) { return (int)(OS_SPAN / F / 64 * 64); }

struct OsFir {               // N taps as an interpolator by F, phase-major in LDS
    int N, J, Jp, phs;       // slots per phase, the row pitch (J: a wave reads one phase at a time, so the rows need no
                             // skew against each other), the first phase whose slot 0 holds no tap
    int words, offset, reversed;
};

struct OsArgs {
    gfx_rowmap_t xmap, ymap, gmap;       // x, the output (y or gx), gy
    int64_t L, FL, ntiles;
    int C, F, T, K, NS;
    int use_tanh, inverse_post, want_par;
    OsFir up, dn;                        // h_up; backward only: h_dn reversed, the interpolator of gy
    int ND, o_lo;                        // stage 3: its taps, and m F - o_lo is the first high-rate sample under output m
    int xwords, gwords, vpitch;          // LDS words of the two spans, pitch of a phase of the high-rate samples
};

static inline OsFir os_fir(int64_t N, int64_t F, int64_t offset, int reversed) {
    OsFir f;
    f.N = (int)N;
    f.J = (int)((N + F - 1) / F);
    f.Jp = f.J;
    f.phs = (int)(N - (f.J - 1) * F);
    f.words = (int)(F * f.Jp);
    f.offset = (int)offset;
    f.reversed = reversed;
    return f;
}

// slot s of phase ph holds g[ph + (J - 1 - s) F], g the taps as they are or reversed; slot 0 is 0 where that is past the end
__device__ __forceinline__ void os_stage_phases(float* hp, const float* __restrict__ h, const OsFir& f, int F) {
    const int t = threadIdx.x;
    for (int ph = f.phs + t; ph < F; ph += OS_THREADS) hp[ph * f.Jp] = 0.0f;
    for (int i = t; i < f.N; i += OS_THREADS) {
        const int jj = i / F, ph = i - jj * F;
        hp[ph * f.Jp + (f.J - 1 - jj)] = h[f.reversed ? f.N - 1 - i : i];
    }
}

// the span of a base-rate row under the high-rate samples p_lo .. p_lo + nv - 1 of an interpolator: its first sample (what
// slot 0 of the first of them reads) and its length in words
__device__ __forceinline__ int64_t os_span_base(const OsFir& f, int F, int64_t p_lo) {
    return floor_div(p_lo + f.offset, F) - (f.J - 1);
}
static __host__ __device__ __forceinline__ int os_span_words(int J, int F, int nv) { return (nv - 1) / F + J + 1; }

__device__ __forceinline__ void os_stage_span(float* s, const float* __restrict__ row, int64_t kbase, int n, int64_t L,
                                              float mean) {
    for (int w = threadIdx.x; w < n; w += OS_THREADS) {
        const int64_t k = kbase + w;
        s[w] = k >= 0 && k < L ? row[k] - mean : 0.0f;
    }
}

struct OsPhase {             // the high-rate samples p_lo + a + b F, b = 0, 1, ...: one phase of the taps, a run of the span
    const float* g;
    int x0;                  // sample b reads span[x0 + b .. x0 + b + J)
    bool head;               // slot 0 holds a tap
};

__device__ __forceinline__ OsPhase os_phase(const float* hp, const OsFir& f, int F, int64_t p, int64_t kbase) {
    const int64_t e = p + f.offset, q = floor_div(e, F);
    const int ph = (int)(e - q * F);
    return OsPhase{hp + ph * f.Jp, (int)(q - kbase) - (f.J - 1), ph < f.phs};
}

// NB samples of one phase, 256 quotients apart, sharing every tap
template <int NB>
__device__ __forceinline__ void os_dots(const OsPhase& P, const float* span, int b, int J, float (&acc)[NB]) {
    const float* xv = span + P.x0 + b;
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] = P.head ? fmaf(P.g[0], xv[k * OS_THREADS], 0.0f) : 0.0f;
#pragma unroll 4
    for (int s = 1; s < J; ++s) {
        const float g = P.g[s];
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = fmaf(g, xv[s + k * OS_THREADS], acc[k]);
    }
}

// NB outputs of stage 3, 256 apart: out[t] = sum_j v[t F + j] hh[j], v phase-major
template <int NB>
__device__ __forceinline__ void os_decimate(const float* vs, const float* hh, int N, int F, int pitch, int t, float (&acc)[NB]) {
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] = 0.0f;
    const float* col = vs + t;
    int a = 0;
    for (int j = 0; j < N; ++j) {
        const float h = hh[j];
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = fmaf(col[a + k * OS_THREADS], h, acc[k]);
        a += pitch;
        if (a == F * pitch) {
            a = 0;
            ++col;
        }
    }
}

template <int MODE>
__global__ __launch_bounds__(OS_THREADS) void os_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            const float* __restrict__ h_up, const float* __restrict__ h_dn,
                                                            const float* __restrict__ log_pre,
                                                            const float* __restrict__ log_post, const float* __restrict__ p0,
                                                            const float* __restrict__ p1, const float* __restrict__ dc,
                                                            OsArgs a) {
    extern __shared__ __attribute__((aligned(16))) float os_lds[];
    __shared__ float sw[WS_MAX_K];
    float* hp = os_lds;                  // the interpolator, phase-major
    float* hh = hp + a.up.words;         // the decimator, reversed
    float* xs = hh + a.ND;               // the span of x - dc
    float* vs = xs + a.xwords;           // the shaped high-rate samples, phase-major
    const int t = threadIdx.x, F = a.F;
    const int64_t item = blockIdx.x;
    const int64_t rc = item / a.ntiles, tile = item - rc * a.ntiles;
    const int64_t r = rc / a.C;
    const int c = (int)(rc - r * a.C);
    os_stage_phases(hp, h_up, a.up, F);
    for (int j = t; j < a.ND; j += OS_THREADS) hh[j] = h_dn[a.ND - 1 - j];
    WsRow q;
    ws_row_setup<MODE>(q, sw, r, a.K, a.inverse_post, log_pre, log_post, p0, p1);
    q.dc = 0.0f;                         // (subtracted when the span is staged)

    const int64_t m0 = tile * a.T;
    const int left = (int)(a.L - m0 < a.T ? a.L - m0 : a.T);
    const int nv = left * F + a.ND - 1;
    const int64_t p_lo = m0 * F - a.o_lo;
    const int64_t kbase = os_span_base(a.up, F, p_lo);
    os_stage_span(xs, x + row_off(a.xmap, r, c), kbase, os_span_words(a.up.J, F, nv), a.L, dc ? dc[rc] : 0.0f);
    __syncthreads();

    const int i_lo = p_lo < 0 ? (int)(-p_lo < nv ? -p_lo : nv) : 0;          // local samples inside [0, F L)
    const int i_hi = (int)(a.FL - p_lo < nv ? a.FL - p_lo : nv);
    const bool use_tanh = a.use_tanh != 0;
    for (int ph = 0; ph < F; ++ph) {
        const OsPhase P = os_phase(hp, a.up, F, p_lo + ph, kbase);
        const int nb = (nv - ph + F - 1) / F;
        float* vrow = vs + ph * a.vpitch;
        int b = t;
        for (; b + 3 * OS_THREADS < nb; b += 4 * OS_THREADS) {
            float u[4];
            os_dots<4>(P, xs, b, a.up.J, u);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int i = (b + k * OS_THREADS) * F + ph;
                vrow[b + k * OS_THREADS] = i >= i_lo && i < i_hi ? shape<MODE>(u[k], q, a.K, use_tanh) : 0.0f;
            }
        }
        for (; b < nb; b += OS_THREADS) {
            float u[1];
            os_dots<1>(P, xs, b, a.up.J, u);
            const int i = b * F + ph;
            vrow[b] = i >= i_lo && i < i_hi ? shape<MODE>(u[0], q, a.K, use_tanh) : 0.0f;
        }
    }
    __syncthreads();

    float* yrow = y + row_off(a.ymap, r, c) + m0;
    int tt = t;
    for (; tt + 3 * OS_THREADS < left; tt += 4 * OS_THREADS) {
        float acc[4];
        os_decimate<4>(vs, hh, a.ND, F, a.vpitch, tt, acc);
#pragma unroll
        for (int k = 0; k < 4; ++k) yrow[tt + k * OS_THREADS] = acc[k];
    }
    for (; tt < left; tt += OS_THREADS) {
        float acc[1];
        os_decimate<1>(vs, hh, a.ND, F, a.vpitch, tt, acc);
        yrow[tt] = acc[0];
    }
}

// The backward tile: gx for T base samples.  Stage 2 forms gu over the F T + N_up - 1 high-rate samples its gx reaches
// (u and gv by two interpolations, then bwd_samples); a sample adds to the parameter sums in exactly one tile, the one
// whose [F m0, F (m0 + T)) holds it -- the halo serves gx only.  Partial sums: registers -> wave shuffles -> LDS -> one
// store per sum and workgroup; ws_bwd_finish_kernel (nonlinear.hip) adds them in double in a fixed order.
template <int MODE>
__global__ __launch_bounds__(OS_THREADS) void os_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                            float* __restrict__ gx, const float* __restrict__ h_up,
                                                            const float* __restrict__ h_dn, const float* __restrict__ log_pre,
                                                            const float* __restrict__ log_post, const float* __restrict__ p0,
                                                            const float* __restrict__ p1, const float* __restrict__ dc,
                                                            float* __restrict__ part, float* __restrict__ dcpart, OsArgs a) {
    constexpr int NA = WsAcc<MODE>::N;
    constexpr bool POLY = MODE == GFX_WS_POWER || MODE == GFX_WS_CHEBYSHEV;
    extern __shared__ __attribute__((aligned(16))) float os_lds[];
    __shared__ float sw[WS_MAX_K];
    __shared__ float red[4][NA];
    __shared__ float tot[NA];
    float* hp = os_lds;                  // h_up, phase-major: u from x
    float* hd = hp + a.up.words;         // h_dn reversed, phase-major: gv from gy
    float* hh = hd + a.dn.words;         // h_up as it is: gx from gu
    float* xs = hh + a.ND;
    float* gs = xs + a.xwords;
    float* vs = gs + a.gwords;           // gu, phase-major
    const int t = threadIdx.x, F = a.F, lane = t & 63, wave = t >> 6;
    const int64_t item = blockIdx.x;
    const int64_t rc = item / a.ntiles, tile = item - rc * a.ntiles;
    const int64_t r = rc / a.C;
    const int c = (int)(rc - r * a.C);
    os_stage_phases(hp, h_up, a.up, F);
    os_stage_phases(hd, h_dn, a.dn, F);
    for (int j = t; j < a.ND; j += OS_THREADS) hh[j] = h_up[j];
    WsRow q;
    ws_row_setup<MODE>(q, sw, r, a.K, a.inverse_post, log_pre, log_post, p0, p1);
    q.dc = 0.0f;

    const int64_t m0 = tile * a.T;
    const int left = (int)(a.L - m0 < a.T ? a.L - m0 : a.T);
    const int nv = left * F + a.ND - 1;
    const int64_t p_lo = m0 * F - a.o_lo;
    const int64_t kbx = os_span_base(a.up, F, p_lo), kbg = os_span_base(a.dn, F, p_lo);
    os_stage_span(xs, x + row_off(a.xmap, r, c), kbx, os_span_words(a.up.J, F, nv), a.L, dc ? dc[rc] : 0.0f);
    os_stage_span(gs, gy + row_off(a.gmap, r, c), kbg, os_span_words(a.dn.J, F, nv), a.L, 0.0f);
    __syncthreads();

    const int i_lo = p_lo < 0 ? (int)(-p_lo < nv ? -p_lo : nv) : 0;
    const int i_hi = (int)(a.FL - p_lo < nv ? a.FL - p_lo : nv);
    const int own_lo = a.o_lo;                                               // the tile's own samples: left F from here on
    const bool use_tanh = a.use_tanh != 0, want_par = a.want_par != 0;
    const float inv = a.inverse_post ? 1.0f : 0.0f;
    float acc[NA];
#pragma unroll
    for (int j = 0; j < NA; ++j) acc[j] = 0.0f;
    // the tile's own samples, all inside [0, F L): `left` of every phase, four to a lane where that many are left -- they
    // share the taps, and bwd_samples walks the K terms once for the four (one sample at a time the recurrences are a
    // single dependent chain: 4.0 ms against 2.8 ms for the Chebyshev shaper of order 10 on 256 x 2 x 131072 samples, F = 4)
    for (int ph = 0; ph < F; ++ph) {
        const OsPhase Pu = os_phase(hp, a.up, F, p_lo + ph, kbx), Pg = os_phase(hd, a.dn, F, p_lo + ph, kbg);
        const int b_lo = (own_lo - ph + F - 1) / F;                          // the first b with b F + ph >= own_lo
        float* vrow = vs + ph * a.vpitch + b_lo;
        int b = t;
        for (; b + 3 * OS_THREADS < left; b += 4 * OS_THREADS) {
            float u[4], g[4], go[4];
            os_dots<4>(Pu, xs, b_lo + b, a.up.J, u);
            os_dots<4>(Pg, gs, b_lo + b, a.dn.J, g);
            bwd_samples<MODE, 4>(u, g, go, q, a.K, use_tanh, inv, want_par, acc);
#pragma unroll
            for (int k = 0; k < 4; ++k) vrow[b + k * OS_THREADS] = go[k];
        }
        for (; b < left; b += OS_THREADS) {
            float u[1], g[1], go[1];
            os_dots<1>(Pu, xs, b_lo + b, a.up.J, u);
            os_dots<1>(Pg, gs, b_lo + b, a.dn.J, g);
            bwd_samples<MODE, 1>(u, g, go, q, a.K, use_tanh, inv, want_par, acc);
            vrow[b] = go[0];
        }
    }
    // the halo, ND - 1 samples below and above the tile's own: for gx alone, every lane its own phase, zero outside [0, F L)
    if (gx) {
        for (int hI = t; hI < nv - left * F; hI += OS_THREADS) {
            const int i = hI < own_lo ? hI : hI + left * F;
            const int b = i / F, ph = i - b * F;
            float go[1] = {0.0f};
            if (i >= i_lo && i < i_hi) {
                const OsPhase Pu = os_phase(hp, a.up, F, p_lo + ph, kbx), Pg = os_phase(hd, a.dn, F, p_lo + ph, kbg);
                float u[1], g[1];
                os_dots<1>(Pu, xs, b, a.up.J, u);
                os_dots<1>(Pg, gs, b, a.dn.J, g);
                bwd_samples<MODE, 1>(u, g, go, q, a.K, use_tanh, inv, false, acc);
            }
            vs[ph * a.vpitch + b] = go[0];
        }
    }
    __syncthreads();

    if (gx) {
        float* orow = gx + row_off(a.ymap, r, c) + m0;
        float dsum = 0.0f;
        int tt = t;
        for (; tt + 3 * OS_THREADS < left; tt += 4 * OS_THREADS) {
            float o[4];
            os_decimate<4>(vs, hh, a.ND, F, a.vpitch, tt, o);
#pragma unroll
            for (int k = 0; k < 4; ++k) orow[tt + k * OS_THREADS] = o[k];
            dsum += (o[0] + o[1]) + (o[2] + o[3]);
        }
        for (; tt < left; tt += OS_THREADS) {
            float o[1];
            os_decimate<1>(vs, hh, a.ND, F, a.vpitch, tt, o);
            orow[tt] = o[0];
            dsum += o[0];
        }
        if (dcpart) {                                // sum over time of this tile's gx, for the centring's adjoint
            dsum = wave_sum(dsum);
            if (lane == 0) red[wave][0] = dsum;
            __syncthreads();
            if (t == 0) dcpart[item] = (red[0][0] + red[1][0]) + (red[2][0] + red[3][0]);
            __syncthreads();                         // red free again
        }
    }
    if (want_par) {
        // (waveshaper_bwd_kernel of nonlinear.hip ends alike: one shared function changed the code of both kernels)
        const int nsum = POLY ? 2 + a.K : NA;        // sums of this mode that are in use
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            if (j < nsum) {
                const float s = wave_sum(acc[j]);
                if (lane == 0) red[wave][j] = s;
            }
        }
        __syncthreads();
        if (t < nsum) {
            const int j = t;
            float s = (red[0][j] + red[1][j]) + (red[2][j] + red[3][j]);
            if (MODE == GFX_WS_PIECEWISE) {
                if (j == 2) s *= q.ap;
                if (j == 3) s *= q.an;
                if (j == 4) s *= q.kn * (1.0f - q.kn);
                if (j == 5) s *= q.kp * (1.0f - q.kp);
            }
            if (POLY && j == 2) s *= use_tanh ? tanhf(1.0f) : 1.0f;
            tot[j] = s;                              // polynomial: raw sums of G f(B_k) first, the output sum needs them
        }
        __syncthreads();
        if (t < nsum) {
            const int j = t;
            float s = tot[j];
            if (POLY) {
                if (j < 2) {                         // sum G s(u) = sum_k w_k sum G f(B_k)
                    float gys = 0.0f;
                    for (int k = 0; k < a.K; ++k) gys += sw[k] * tot[2 + k];
                    s = j == 0 ? s - inv * gys : gys;
                } else {
                    s *= 1.0f - sw[j - 2] * sw[j - 2];
                }
            }
            const int64_t nb = (int64_t)a.C * a.ntiles;
            part[(r * a.NS + j) * nb + c * a.ntiles + tile] = s;
        }
    }
}

// the adjoint of the centring x - mean(x): gx -= mean(gx) per row-channel, tile by tile
__global__ __launch_bounds__(OS_THREADS) void os_sub_mean_kernel(float* __restrict__ gx, gfx_rowmap_t omap,
                                                                 const float* __restrict__ gmean, int C, int64_t L, int T,
                                                                 int64_t ntiles) {
    const int64_t item = blockIdx.x;
    const int64_t rc = item / ntiles, tile = item - rc * ntiles;
    const int64_t r = rc / C;
    const int64_t m0 = tile * T;
    const int left = (int)(L - m0 < T ? L - m0 : T);
    float* orow = gx + row_off(omap, r, (int)(rc - r * C)) + m0;
    const float m = gmean[rc];
    for (int tt = threadIdx.x; tt < left; tt += OS_THREADS) orow[tt] -= m;
}

// the checks both entries share, then the tile geometry (the LDS words of the spans are the caller's: they differ)
static int os_prepare(const float* x, gfx_rowmap_t xmap, int64_t R, int64_t C, int64_t L, int64_t F, const float* h_up,
                      int64_t N_up, int64_t o_up, const float* h_dn, int64_t N_dn, int64_t o_dn, int mode, int use_tanh,
                      int inverse_post_gain, const float* log_pre_gain, const float* p0, const float* p1, int64_t& K, OsArgs& a) {
    if (!x || !h_up || !h_dn || R <= 0 || C <= 0 || L <= 0 || R > 0x7fffffffLL || xmap.inner <= 0) return GFX_EINVAL;
    if (F < 1 || F > OS_MAX_FACTOR || N_up < 1 || N_up > OS_MAX_TAPS || N_dn < 1 || N_dn > OS_MAX_TAPS || o_up < 0 ||
        o_up >= N_up || o_dn < 0 || o_dn >= N_dn)
        return GFX_EINVAL;
    if (ws_check_shaper(mode, inverse_post_gain, log_pre_gain, p0, p1, K) != GFX_OK) return GFX_EINVAL;
    if (C > 0x7fffffffLL || R * C > 0x7fffffffLL || L > INT64_MAX / (2 * OS_MAX_FACTOR)) return GFX_EINVAL;
    const int T = os_tile(F);
    const int64_t ntiles = (L + T - 1) / T;
    if (ntiles > MAX_GRID_X / (R * C)) return GFX_EINVAL;               // grid.x of the tile kernels
    a.xmap = a.ymap = a.gmap = xmap;
    a.L = L; a.FL = F * L; a.ntiles = ntiles;
    a.C = (int)C; a.F = (int)F; a.T = T; a.K = (int)K; a.NS = ws_nsums(K);
    a.use_tanh = use_tanh; a.inverse_post = inverse_post_gain; a.want_par = 0;
    a.up = os_fir(N_up, F, o_up, 0);
    a.dn = os_fir(N_dn, F, N_dn - 1 - o_dn, 1);
    a.gwords = 0;
    return GFX_OK;
}

// the stage-3 filter has ND taps and reaches o_lo samples below output m's own m F: the high-rate tile and the spans
static size_t os_layout(OsArgs& a, int ND, int o_lo, bool backward) {
    a.ND = ND;
    a.o_lo = o_lo;
    const int nv = a.T * a.F + ND - 1;
    a.vpitch = (nv - 1) / a.F + 1;
    a.xwords = os_span_words(a.up.J, a.F, nv);
    a.gwords = backward ? os_span_words(a.dn.J, a.F, nv) : 0;
    return sizeof(float) * ((size_t)a.up.words + (backward ? a.dn.words : 0) + ND + a.xwords + a.gwords + (size_t)a.F * a.vpitch);
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_oversampled_waveshaper_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C,
                                   int64_t L, int64_t factor, const float* h_up, int64_t N_up, int64_t offset_up,
                                   const float* h_dn, int64_t N_dn, int64_t offset_dn, int mode, int use_tanh,
                                   int inverse_post_gain, const float* log_pre_gain, const float* log_post_gain,
                                   const float* p0, const float* p1, int64_t K, const float* dc, void* stream) {
    OsArgs a;
    if (!y || ymap.inner <= 0) return GFX_EINVAL;
    const int rc = os_prepare(x, xmap, R, C, L, factor, h_up, N_up, offset_up, h_dn, N_dn, offset_dn, mode, use_tanh,
                              inverse_post_gain, log_pre_gain, p0, p1, K, a);
    if (rc != GFX_OK) return rc;
    // tiles read each other's halos of x: never in place
    if (map_negative(xmap) || map_negative(ymap) || signals_overlap(y, ymap, x, xmap, R, C, L)) return GFX_EINVAL;
    a.ymap = ymap;
    const size_t lds = os_layout(a, (int)N_dn, (int)(N_dn - 1 - offset_dn), false);
    const dim3 grid((unsigned)(R * C * a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    return with_ws_mode(mode, [&](auto m) {
        return launch(os_fwd_kernel<decltype(m)::value>, grid, dim3(OS_THREADS), lds, st, x, y, h_up, h_dn, log_pre_gain,
                      log_post_gain, p0, p1, dc, a);
    });
}

size_t gfx_oversampled_waveshaper_bwd_ws_bytes(int64_t R, int64_t C, int64_t L, int64_t K, int64_t factor) {
    if (R <= 0 || C <= 0 || L <= 0 || K < 0 || K > WS_MAX_K || factor < 1 || factor > OS_MAX_FACTOR) return 0;
    const int T = os_tile(factor);
    const size_t nt = (size_t)((L + T - 1) / T);
    return sizeof(float) * ws_bwd_floats(R, C, K, (size_t)C * nt, nt);
}

int gfx_oversampled_waveshaper_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R,
                                       int64_t C, int64_t L, int64_t factor, const float* h_up, int64_t N_up,
                                       int64_t offset_up, const float* h_dn, int64_t N_dn, int64_t offset_dn, int mode,
                                       int use_tanh, int inverse_post_gain, const float* log_pre_gain,
                                       const float* log_post_gain, const float* p0, const float* p1, int64_t K, const float* dc,
                                       float* gx, gfx_rowmap_t omap, float* g_log_pre_gain, float* g_log_post_gain, float* g_p0,
                                       float* g_p1, void* ws, size_t ws_bytes, void* stream) {
    OsArgs a;
    if (!gy || gmap.inner <= 0) return GFX_EINVAL;
    const int rc = os_prepare(x, xmap, R, C, L, factor, h_up, N_up, offset_up, h_dn, N_dn, offset_dn, mode, use_tanh,
                              inverse_post_gain, log_pre_gain, p0, p1, K, a);
    if (rc != GFX_OK) return rc;
    const WsGrads grads{g_log_pre_gain, g_log_post_gain, g_p0, g_p1};
    if (ws_check_grads(grads, gx, mode, inverse_post_gain, log_pre_gain, log_post_gain, p0) != GFX_OK) return GFX_EINVAL;
    const bool want_par = grads.any();
    if (gx && (map_negative(xmap) || map_negative(gmap))) return GFX_EINVAL;
    if (!grad_out_ok(gx, omap, x, xmap, gy, gmap, R, C, L)) return GFX_EINVAL;
    const bool center = dc && gx;
    const int64_t npart = C * a.ntiles;              // partials of a row's sum, of a row-channel's: a.ntiles
    WsBwdSpace sp;
    const int src = ws_bwd_carve(ws, ws_bytes, R, C, K, (size_t)npart, (size_t)a.ntiles, want_par, center, sp);
    if (src != GFX_OK) return src;
    a.gmap = gmap;
    a.ymap = gx ? omap : xmap;
    a.want_par = want_par;
    const size_t lds = os_layout(a, (int)N_up, (int)offset_up, true);
    const dim3 grid((unsigned)(R * C * a.ntiles));
    hipStream_t st = (hipStream_t)stream;
    const int lrc = with_ws_mode(mode, [&](auto m) {
        return launch(os_bwd_kernel<decltype(m)::value>, grid, dim3(OS_THREADS), lds, st, x, gy, gx, h_up, h_dn, log_pre_gain,
                      log_post_gain, p0, p1, dc, sp.part, sp.dcpart, a);
    });
    if (lrc != GFX_OK) return GFX_ELAUNCH;
    if (ws_bwd_finish(sp, grads, R, C, L, K, npart, a.ntiles, mode, st) != GFX_OK) return GFX_ELAUNCH;
    if (center) return launch(os_sub_mean_kernel, grid, dim3(OS_THREADS), 0, st, gx, omap, sp.gmean, (int)C, L, a.T, a.ntiles);
    return GFX_OK;
}

}  // extern "C"
