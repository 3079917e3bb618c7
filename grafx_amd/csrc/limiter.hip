// Look-ahead peak limiter with hold and FIR smoothing (gfx950): one fused tile kernel each way, the detector, the sliding
// maximum, the gains and their smoothing only ever in LDS.  For a row r of C channels, with
// T = exp(log_ceiling[r]), M = D + 1 + H, N taps w and sigma in {0, D}:
//
//     p[k]  = max_c |x[c, k]|                           zero outside [0, L) -- or the carried state below 0
//     pk[q] = max_{0 <= j < M} p[q - j]                 ties take the EARLIEST index a(q)
//     m[q]  = pk[q] > T ? T / pk[q] : 1
//     s[n]  = sum_{0 <= j < N} w[j] m[n - j]            float32, from 0.0, ascending j
//     y[c, n] = x[c, n + sigma - D] s[n + sigma]        0 <= n < L
//
// The adjoint, G[c, q] = gy[c, q - sigma] (zero outside its L samples):
//
//     gs[q] = sum_c G[c, q] x[c, q - D]
//     gm[q] = sum_j w[j] gs[q + j]
//     gx[c, k] = G[c, k + D] s[k + D] + [c = c*(k)] sign(x[c, k]) sum_{q : a(q) = k, pk[q] > T} gm[q] (-T / pk[q]^2)
//     g_log_ceiling = T sum_{q : pk[q] > T} gm[q] / pk[q]
//
// A tile is lim_tile(M) consecutive samples of one row, one workgroup of 512 lanes.  The sliding maximum is log2 M doubling
// passes between two LDS buffers, max_2v[i] = max(max_v[i - v], max_v[i]) with the LEFT operand on a tie, then one pass
// that joins two overlapping windows of P = the largest power of two <= M: every pass keeps all lanes busy at any M.  The
// backward carries the index of the maximum beside its value (16 bits: a tile's span is below 65536).  a(q) does not
// decrease with q, so {q : a(q) = k} is one run inside [k, k + M): its two ends are binary searches, and its sum is taken
// from the terms and their sums over blocks of 64 -- at most 63 + 64 + 63 additions for any run, in a fixed order.
// Every q adds to the ceiling sum in exactly one tile (the one that holds min(q, L - 1)); the tile sums go to a workspace
// and are added in double in a fixed order.  No atomics: equal bits from run to run.  Every s[n] is the same chain of fmaf
// over the same m whatever the tile, the block or the call it falls in: blocks concatenate to the one-call output bit for
// bit.  Base offsets are 64-bit, everything inside the tile 32-bit.
#include "common.hpp"

namespace gfx {

constexpr int LIM_THREADS = 512;
constexpr int LIM_WAVES = LIM_THREADS / 64;
constexpr int LIM_MAX_TAPS = 1024;
constexpr int LIM_MAX_WINDOW = 4096;
// the backward tile holds 12 (T + 2 M) + 4 (T + M) + 4 N <= 16 T + 32 M bytes: under 160 KiB with room for the static arrays
constexpr int64_t LIM_LDS_BUDGET = 155000;

static inline int lim_tile(int64_t M) {
    const int64_t t = (LIM_LDS_BUDGET - 32 * M) / 16 / 512 * 512;
    return (int)(t > 4096 ? 4096 : t < 1024 ? 1024 : t);
}

struct LimArgs {
    gfx_rowmap_t xmap, ymap, gmap;       // x, the output (y or gx), gy
    int64_t L, ntiles;
    int C, D, M, N, S, sigma, T, P;      // S = M + N - 2 carried samples, P = the largest power of two <= M
    int pwords, qwords;                  // LDS words of a peak buffer, of the backward's terms
};

// sample k of a row-channel: the signal inside [0, L), the carried state (S samples, oldest first) below 0, else zero
__device__ __forceinline__ float lim_sample(const float* __restrict__ xrow, const float* __restrict__ zrow, int64_t k,
                                            int64_t L, int S) {
    if (k >= 0) return k < L ? xrow[k] : 0.0f;
    return zrow && k >= -(int64_t)S ? zrow[S + k] : 0.0f;
}

// p[i] = max_c |x[c, kbase + i]|, 0 <= i < n
__device__ __forceinline__ void lim_stage_peaks(float* p, const float* __restrict__ xrow, int64_t sch,
                                                const float* __restrict__ zrow, int C, int S, int64_t kbase, int n, int64_t L) {
    for (int i = threadIdx.x; i < n; i += LIM_THREADS) {
        const int64_t k = kbase + i;
        float v = 0.0f;
        if (k >= 0 && k < L) {
            for (int c = 0; c < C; ++c) v = fmaxf(v, fabsf(xrow[c * sch + k]));
        } else if (k < 0 && zrow && k >= -(int64_t)S) {
            for (int c = 0; c < C; ++c) v = fmaxf(v, fabsf(zrow[(int64_t)c * S + S + k]));
        }
        p[i] = v;
    }
}

// dst[i] = max(src[i - v], src[i]), the left operand on a tie (the earlier index); with ARG the index travels along
template <bool ARG>
__device__ __forceinline__ void lim_max_pass(const float* src, float* dst, const uint16_t* isrc, uint16_t* idst, int n, int v) {
    for (int i = threadIdx.x; i < n; i += LIM_THREADS) {
        float b = src[i];
        unsigned ib = ARG ? isrc[i] : 0u;
        if (i >= v) {
            const float a = src[i - v];
            if (a >= b) {
                b = a;
                if (ARG) ib = isrc[i - v];
            }
        }
        dst[i] = b;
        if (ARG) idst[i] = (uint16_t)ib;
    }
    __syncthreads();
}

// the maximum of the M values ending at i, for every i >= M - 1 of the n staged values (with ARG: ia[i] = i on entry).
// Returns whether the result stands in the second pair of buffers.
template <bool ARG>
__device__ __forceinline__ bool lim_sliding_max(float* a, float* b, uint16_t* ia, uint16_t* ib, int n, int M, int P) {
    bool second = false;
    for (int v = 1; v < P; v <<= 1) {
        if (second) lim_max_pass<ARG>(b, a, ib, ia, n, v);
        else lim_max_pass<ARG>(a, b, ia, ib, n, v);
        second = !second;
    }
    if (M > P) {
        if (second) lim_max_pass<ARG>(b, a, ib, ia, n, M - P);
        else lim_max_pass<ARG>(a, b, ia, ib, n, M - P);
        second = !second;
    }
    return second;
}

// NB sums 512 apart sharing every tap: acc[k] = sum_j w[j] col[k 512 + DIR j], ascending j from 0.0
template <int NB, int DIR>
__device__ __forceinline__ void lim_fir(const float* w, int N, const float* col, float (&acc)[NB]) {
#pragma unroll
    for (int k = 0; k < NB; ++k) acc[k] = 0.0f;
#pragma unroll 4
    for (int j = 0; j < N; ++j) {
        const float h = w[j];
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = fmaf(h, col[k * LIM_THREADS + DIR * j], acc[k]);
    }
}

// The backward's gm[q] = sum_j w[j] gs[q + j], whose order is free: the taps in eight runs, each its own float chain, joined
// in double and handed on in double.  gs changes sign and gm is smooth in q, so the ceiling gradient is a sum of thousands
// of terms whose partial sums reach a thousand times the result: it is taken from these doubles and kept in double down to
// the workspace (with float partial sums it was 2.0e-5 off the reference at N = 1024, L = 2051).
template <int NB>
__device__ __forceinline__ void lim_fir_runs(const float* w, int N, const float* col, double (&tot)[NB]) {
#pragma unroll
    for (int k = 0; k < NB; ++k) tot[k] = 0.0;
    for (int c = 0; c < 8; ++c) {
        const int j0 = N * c / 8, j1 = N * (c + 1) / 8;
        float acc[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) acc[k] = 0.0f;
#pragma unroll 4
        for (int j = j0; j < j1; ++j) {
            const float h = w[j];
#pragma unroll
            for (int k = 0; k < NB; ++k) acc[k] = fmaf(h, col[k * LIM_THREADS + j], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) tot[k] += (double)acc[k];
    }
}

__global__ __launch_bounds__(LIM_THREADS) void lim_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              const float* __restrict__ log_ceiling,
                                                              const float* __restrict__ w, const float* __restrict__ zi,
                                                              float* __restrict__ gain, LimArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lim_lds[];
    float* ws = lim_lds;                 // the taps
    float* pa = ws + a.N;                // the peaks, and the other side of the doubling passes
    float* pb = pa + a.pwords;
    const int t = threadIdx.x, N = a.N, M = a.M;
    const int64_t item = blockIdx.x;
    const int64_t r = item / a.ntiles, tile = item - r * a.ntiles;
    for (int j = t; j < N; j += LIM_THREADS) ws[j] = w[j];
    const float Tc = expf(log_ceiling[r]);

    const int64_t n0 = tile * a.T;
    const int left = (int)(a.L - n0 < a.T ? a.L - n0 : a.T);
    const int nm = left + N - 1;                         // gains m[q], q from n0 + sigma - (N - 1)
    const int np = nm + M - 1;                           // peaks under them
    const int64_t kbase = n0 + a.sigma - (N - 1) - (M - 1);
    const float* xrow = x + row_off(a.xmap, r, 0);
    const int64_t sch = a.xmap.stride_ch;
    const float* zrow = zi ? zi + r * a.C * (int64_t)a.S : nullptr;
    lim_stage_peaks(pa, xrow, sch, zrow, a.C, a.S, kbase, np, a.L);
    __syncthreads();
    const bool second = lim_sliding_max<false>(pa, pb, nullptr, nullptr, np, M, a.P);
    const float* pk = second ? pb : pa;
    float* ms = second ? pa : pb;
    for (int i = t; i < nm; i += LIM_THREADS) {
        const float v = pk[i + M - 1];
        ms[i] = v > Tc ? Tc / v : 1.0f;
    }
    __syncthreads();

    float* yrow = y + row_off(a.ymap, r, 0);
    const int64_t ysch = a.ymap.stride_ch;
    const int shift = a.sigma - a.D;
    auto emit = [&](int tt, float s) {
        const int64_t n = n0 + tt;
        for (int c = 0; c < a.C; ++c)
            yrow[c * ysch + n] = lim_sample(xrow + c * sch, zrow ? zrow + (int64_t)c * a.S : nullptr, n + shift, a.L, a.S) * s;
        if (gain) gain[r * a.L + n] = s;
    };
    int tt = t;
    for (; tt + 3 * LIM_THREADS < left; tt += 4 * LIM_THREADS) {
        float s[4];
        lim_fir<4, -1>(ws, N, ms + tt + N - 1, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) emit(tt + k * LIM_THREADS, s[k]);
    }
    for (; tt < left; tt += LIM_THREADS) {
        float s[1];
        lim_fir<1, -1>(ws, N, ms + tt + N - 1, s);
        emit(tt, s[0]);
    }
}

// The backward tile: gx for T samples k0 .. k0 + left - 1 of a row.  Local q index j stands for q = k0 + j, 0 <= j < nq =
// left + M - 1 (every q whose window holds a sample of the tile); the peaks under them start M - 1 earlier, so q = k0 + j
// sits at peak index j + M - 1, and a(q) is kept as a peak index.
__global__ __launch_bounds__(LIM_THREADS) void lim_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                              float* __restrict__ gx, const float* __restrict__ log_ceiling,
                                                              const float* __restrict__ w, double* __restrict__ part,
                                                              LimArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lim_lds[];
    __shared__ double red[LIM_WAVES];
    float* ws = lim_lds;
    float* pa = ws + a.N;
    float* pb = pa + a.pwords;
    float* es = pb + a.pwords;           // gm, then the routed terms gm (-T / pk^2)
    uint16_t* ia = reinterpret_cast<uint16_t*>(es + a.qwords);
    uint16_t* ib = ia + a.pwords;
    const int t = threadIdx.x, N = a.N, M = a.M, D = a.D, lane = t & 63, wave = t >> 6;
    const int64_t item = blockIdx.x;
    const int64_t r = item / a.ntiles, tile = item - r * a.ntiles;
    for (int j = t; j < N; j += LIM_THREADS) ws[j] = w[j];
    const float Tc = expf(log_ceiling[r]);

    const int64_t k0 = tile * a.T;
    const int left = (int)(a.L - k0 < a.T ? a.L - k0 : a.T);
    const int nq = left + M - 1, np = nq + M - 1, ng = nq + N - 1;
    const float* xrow = x + row_off(a.xmap, r, 0);
    const float* grow = gy + row_off(a.gmap, r, 0);
    const int64_t sch = a.xmap.stride_ch, gsch = a.gmap.stride_ch;
    lim_stage_peaks(pa, xrow, sch, nullptr, a.C, 0, k0 - (M - 1), np, a.L);
    for (int i = t; i < np; i += LIM_THREADS) ia[i] = (uint16_t)i;
    __syncthreads();
    const bool second = lim_sliding_max<true>(pa, pb, ia, ib, np, M, a.P);
    float* pk = second ? pb : pa;        // pk, then m in its place
    float* gs = second ? pa : pb;        // gs, then the block sums of the routed terms
    const uint16_t* arg = second ? ib : ia;

    for (int j = t; j < ng; j += LIM_THREADS) {
        const int64_t q = k0 + j, n = q - a.sigma, kx = q - D;
        float v = 0.0f;
        if (n >= 0 && n < a.L && kx >= 0 && kx < a.L)
            for (int c = 0; c < a.C; ++c) v = fmaf(grow[c * gsch + n], xrow[c * sch + kx], v);
        gs[j] = v;
    }
    __syncthreads();
    // gm for every q of the tile's span; the ceiling sum takes the q this tile owns -- its own `left`, and in the last tile
    // everything beyond -- as gm T / pk with gm still in double
    const bool last = tile == a.ntiles - 1;
    double acc = 0.0;
    auto keep = [&](int j, double g) {
        es[j] = (float)g;
        const float v = pk[j + M - 1];
        if (v > Tc && (j < left || last)) acc += g * (double)(Tc / v);
    };
    {
        int j = t;
        for (; j + 3 * LIM_THREADS < nq; j += 4 * LIM_THREADS) {
            double g[4];
            lim_fir_runs<4>(ws, N, gs + j, g);
#pragma unroll
            for (int k = 0; k < 4; ++k) keep(j + k * LIM_THREADS, g[k]);
        }
        for (; j < nq; j += LIM_THREADS) {
            double g[1];
            lim_fir_runs<1>(ws, N, gs + j, g);
            keep(j, g[0]);
        }
    }
    __syncthreads();                     // (gs is free from here on)
    // its gain in the place of pk, its routed term in the place of gm
    for (int j = t; j < nq; j += LIM_THREADS) {
        const float v = pk[j + M - 1], g = es[j];
        const bool over = v > Tc;
        const float m = over ? Tc / v : 1.0f;
        pk[j + M - 1] = m;
        es[j] = over ? -g * m / v : 0.0f;
    }
    __syncthreads();
    float* bs = gs;
    for (int b = wave; b * 64 < nq; b += LIM_WAVES) {
        const int j = b * 64 + lane;
        const float s = wave_sum(j < nq ? es[j] : 0.0f);
        if (lane == 0) bs[b] = s;
    }
    if (part) {
        acc = wave_sum(acc);
        if (lane == 0) red[wave] = acc;
    }
    __syncthreads();
    if (part && t == 0) {
        double s = 0.0;
        for (int k = 0; k < LIM_WAVES; ++k) s += red[k];
        part[item] = s;
    }
    if (!gx) return;

    float* orow = gx + row_off(a.ymap, r, 0);
    const int64_t osch = a.ymap.stride_ch;
    auto emit = [&](int tt, float s) {
        const int64_t k = k0 + tt, n = k + D - a.sigma;
        const int ik = tt + M - 1;                       // the peak index of sample k
        // the run of q with a(q) = k: inside [k, k + M), where a(q) goes from <= k to > k
        const int hi = tt + M < nq ? tt + M : nq;
        int lo0 = tt, hi0 = hi;
        while (lo0 < hi0) {                              // the first j with a >= ik
            const int mid = (lo0 + hi0) >> 1;
            if (arg[mid + M - 1] >= ik) hi0 = mid; else lo0 = mid + 1;
        }
        int lo1 = lo0, hi1 = hi;
        while (lo1 < hi1) {                              // the first j with a > ik
            const int mid = (lo1 + hi1) >> 1;
            if (arg[mid + M - 1] > ik) hi1 = mid; else lo1 = mid + 1;
        }
        float routed = 0.0f;
        int j = lo0;
        while (j < lo1 && (j & 63)) routed += es[j++];
        while (j + 64 <= lo1) {
            routed += bs[j >> 6];
            j += 64;
        }
        while (j < lo1) routed += es[j++];
        float peak = 0.0f;
        for (int c = 0; c < a.C; ++c) peak = fmaxf(peak, fabsf(xrow[c * sch + k]));
        bool taken = lo1 == lo0;                         // nothing to route, or routed already: the lowest c takes it
        for (int c = 0; c < a.C; ++c) {
            const float xv = xrow[c * sch + k];
            float o = n < a.L ? grow[c * gsch + n] * s : 0.0f;
            if (!taken && fabsf(xv) == peak) {
                taken = true;
                o += xv > 0.0f ? routed : xv < 0.0f ? -routed : 0.0f;
            }
            orow[c * osch + k] = o;
        }
    };
    // s[k + D] = sum_j w[j] m[k + D - j]: q = k + D - j sits at peak index tt + D - j + M - 1
    int tt = t;
    for (; tt + 3 * LIM_THREADS < left; tt += 4 * LIM_THREADS) {
        float s[4];
        lim_fir<4, -1>(ws, N, pk + tt + D + M - 1, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) emit(tt + k * LIM_THREADS, s[k]);
    }
    for (; tt < left; tt += LIM_THREADS) {
        float s[1];
        lim_fir<1, -1>(ws, N, pk + tt + D + M - 1, s);
        emit(tt, s[0]);
    }
}

// a row's tile sums -> its ceiling gradient (tile_sums_finish_kernel): the one slot of a row
struct LimSlots {
    float* g_log_ceiling;
    __device__ float* dest(int64_t r, int64_t, double&) const { return g_log_ceiling + r; }
};

// the checks both entries share, then the tile geometry
static int lim_prepare(const float* x, gfx_rowmap_t xmap, int64_t R, int64_t C, int64_t L, const float* log_ceiling,
                       const float* w, int64_t N, int64_t D, int64_t H, int64_t sigma, LimArgs& a) {
    if (!x || !log_ceiling || !w || R <= 0 || C <= 0 || L <= 0 || R > 0x7fffffffLL || C > 0x7fffffffLL || xmap.inner <= 0)
        return GFX_EINVAL;
    if (D < 0 || H < 0 || D >= LIM_MAX_WINDOW || H >= LIM_MAX_WINDOW || D + 1 + H > LIM_MAX_WINDOW) return GFX_EINVAL;
    if (N < 1 || N > LIM_MAX_TAPS || N > D + 1) return GFX_EINVAL;
    if (sigma != 0 && sigma != D) return GFX_EINVAL;
    if (R * C > 0x7fffffffLL || L > INT64_MAX / 4) return GFX_EINVAL;
    const int64_t M = D + 1 + H;
    const int T = lim_tile(M);
    const int64_t ntiles = (L + T - 1) / T;
    if (ntiles > MAX_GRID_X / R) return GFX_EINVAL;                    // grid.x of the tile kernels
    a.xmap = a.ymap = a.gmap = xmap;
    a.L = L; a.ntiles = ntiles;
    a.C = (int)C; a.D = (int)D; a.M = (int)M; a.N = (int)N; a.S = (int)(M + N - 2); a.sigma = (int)sigma; a.T = T;
    a.P = 1;
    while (2 * a.P <= a.M) a.P *= 2;
    a.pwords = a.qwords = 0;
    return GFX_OK;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_limiter_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L,
                    const float* log_ceiling, const float* w, int64_t N, int64_t D, int64_t H, int64_t sigma, const float* zi,
                    float* zf, float* gain, void* stream) {
    LimArgs a;
    if (!y || ymap.inner <= 0) return GFX_EINVAL;
    const int rc = lim_prepare(x, xmap, R, C, L, log_ceiling, w, N, D, H, sigma, a);
    if (rc != GFX_OK) return rc;
    if ((zi || zf) && sigma > 0) return GFX_EINVAL;    // the compensated output needs samples the next block brings
    // tiles read each other's halos of x: never in place
    if (map_negative(xmap) || map_negative(ymap) || signals_overlap(y, ymap, x, xmap, R, C, L)) return GFX_EINVAL;
    if (!history_pair_ok(zi, zf, R, C, a.S)) return GFX_EINVAL;        // (past 2^30 state rows: refused before any launch)
    a.ymap = ymap;
    a.pwords = a.T + a.N - 1 + a.M - 1;
    const size_t lds = sizeof(float) * ((size_t)a.N + 2 * (size_t)a.pwords);
    hipStream_t st = (hipStream_t)stream;
    if (launch(lim_fwd_kernel, dim3((unsigned)(R * a.ntiles)), dim3(LIM_THREADS), lds, st, x, y, log_ceiling, w, zi, gain, a) !=
        GFX_OK)
        return GFX_ELAUNCH;
    if (zf && a.S > 0) return launch_history_tail(x, xmap, zi, zf, R, C, L, a.S, nullptr, nullptr, st);
    return GFX_OK;
}

size_t gfx_limiter_bwd_ws_bytes(int64_t R, int64_t L, int64_t D, int64_t H) {
    if (R <= 0 || L <= 0 || D < 0 || H < 0 || D >= LIM_MAX_WINDOW || H >= LIM_MAX_WINDOW || D + 1 + H > LIM_MAX_WINDOW) return 0;
    const int T = lim_tile(D + 1 + H);
    return sizeof(double) * (size_t)R * (size_t)((L + T - 1) / T);
}

int gfx_limiter_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R, int64_t C, int64_t L,
                        const float* log_ceiling, const float* w, int64_t N, int64_t D, int64_t H, int64_t sigma, float* gx,
                        gfx_rowmap_t omap, float* g_log_ceiling, void* ws, size_t ws_bytes, void* stream) {
    LimArgs a;
    if (!gy || gmap.inner <= 0) return GFX_EINVAL;
    const int rc = lim_prepare(x, xmap, R, C, L, log_ceiling, w, N, D, H, sigma, a);
    if (rc != GFX_OK) return rc;
    if (!gx && !g_log_ceiling) return GFX_EINVAL;
    if (map_negative(xmap) || map_negative(gmap)) return GFX_EINVAL;
    if (!grad_out_ok(gx, omap, x, xmap, gy, gmap, R, C, L)) return GFX_EINVAL;
    double* part = nullptr;
    if (g_log_ceiling) {
        const int wrc = workspace_ok(ws, ws_bytes, gfx_limiter_bwd_ws_bytes(R, L, D, H), alignof(double));
        if (wrc != GFX_OK) return wrc;
        part = static_cast<double*>(ws);
    }
    a.gmap = gmap;
    a.ymap = gx ? omap : xmap;
    a.pwords = a.T + 2 * (a.M - 1);
    a.pwords += a.pwords & 1;                            // (the 16-bit indices behind the floats stay 4-byte aligned)
    a.qwords = a.T + a.M - 1;
    const size_t lds = sizeof(float) * ((size_t)a.N + 2 * (size_t)a.pwords + (size_t)a.qwords) + 2 * sizeof(uint16_t) * (size_t)a.pwords;
    hipStream_t st = (hipStream_t)stream;
    if (launch(lim_bwd_kernel, dim3((unsigned)(R * a.ntiles)), dim3(LIM_THREADS), lds, st, x, gy, gx, log_ceiling, w, part, a) !=
        GFX_OK)
        return GFX_ELAUNCH;
    if (part) return finish_tile_sums(LimSlots{g_log_ceiling}, part, R, 1, a.ntiles, st);
    return GFX_OK;
}

}  // extern "C"
