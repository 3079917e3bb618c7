// Modulated delay line -- chorus, vibrato, doubling (gfx950): fused tile kernels each way.  For a
// row r of C channels and V voices, p = pos[r] + n the absolute position of sample n (pos = 0 without a state):
//
//     theta[v,c,n] = rate[r,v] p + phase[r,v,c]                           cycles; one double fma, reduced mod 1
//     d[v,c,n]     = clamp(delay[r,v] + depth[r,v] sin(2 pi theta), 1, Dmax)   samples; in double
//     i = floor(d),  f = float32(d - i)
//     u[v,c,n]     = sum_j l_j(f) x[c, n - i - j]                         x zero, or the carried history, below the row's start
//     y[c,n]       = dry[r] x[c,n] + sum_v gain[r,v,c] u[v,c,n]           one fmaf chain: dry, then v ascending, then j ascending
//
// with l_j the linear (j in {0, 1}) or third-order Lagrange (j in {-1, 0, 1, 2}) weights.  A sample's value depends on its
// position, its row's parameters and the samples it reads only: it has the same bits whatever tile, block or call it
// falls in.
//
// A tile is MD_TILE consecutive samples of one row, one workgroup of 256 lanes, the channels one after the other through
// the same LDS.  The forward stages the part of x its voices can reach (at most Dmax + 2 samples below the tile).  The
// backward is two kernels, each launched only when something it produces is asked for:
//   - md_bwd_x_kernel, gx for the tile's samples k.  With the contract 2 pi rate depth <= 1/2 the read position
//     m(n) = n - i(n) never decreases and takes each value at most twice, so the n that read k are one run of at most
//     2 taps samples.  Per voice and channel the tile recomputes m(n) (16 bits, relative) and f(n) for every n that can
//     reach it -- at most tile + 2 depth + 4 of them -- into LDS, finds the run's start by binary search and sums it in
//     ascending n.
//   - md_bwd_par_kernel, the six parameter gradients: the forward's gather again, with the derivative weights l'_j, summed
//     over the tile in double (g_rate carries the factor p, and the terms change sign).  The tile sums go to the
//     workspace, tile_sums_finish_kernel (common.hpp, with MdSlots) adds them per row in a fixed order.
// No atomics anywhere: equal bits from run to run, and a row's result does not depend on the other rows.  Outside the
// contract every index is still inside its buffer (d is clamped before it is split, the run walk is bounded); the values
// are unspecified.  Base offsets are 64-bit, everything inside the tile 32-bit.
#include "common.hpp"

namespace gfx {

constexpr int MD_THREADS = 256;
constexpr int MD_WAVES = MD_THREADS / 64;
constexpr int MD_TILE = 2048;
constexpr int MD_PER_LANE = MD_TILE / MD_THREADS;
constexpr int MD_MAX_DELAY = 8192;
constexpr int MD_MAX_VOICES = 8;
constexpr double MD_TWO_PI = 6.283185307179586476925286766559;

struct MdArgs {
    gfx_rowmap_t xmap, ymap, gmap;       // x, the output (y or gx), gy
    int64_t L, ntiles;
    int C, V, Dmax, S;                   // S = Dmax + 2 carried samples
};

// the phase of a voice at position p, in cycles, reduced to [0, 1)
__device__ __forceinline__ double md_phase(double rate, double phase, int64_t p) {
    const double th = fma(rate, (double)p, phase);
    return th - floor(th);
}

// the delay from the oscillator's sine -> its integer part (1 .. Dmax) and fraction; `open`: the clamp does not bind
__device__ __forceinline__ int md_split(double delay, double depth, double s, int Dmax, float& f, bool& open) {
    const double raw = fma(depth, s, delay);
    const double d = fmin(fmax(raw, 1.0), (double)Dmax);       // (a NaN comes out as 1)
    open = raw >= 1.0 && raw <= (double)Dmax;
    const double fl = floor(d);
    f = (float)(d - fl);
    return (int)fl;
}

// floor of the clamped delay at the ends of the oscillator's swing
__device__ __forceinline__ int md_floor_at(double delay, double swing, int Dmax) {
    return (int)floor(fmin(fmax(delay + swing, 1.0), (double)Dmax));
}

template <int CUBIC>
struct MdTaps {
    static constexpr int N = CUBIC ? 4 : 2;      // taps
    static constexpr int J0 = CUBIC ? -1 : 0;    // the first node
};

// l_j(f), j = J0 .. J0 + N - 1
template <int CUBIC>
__device__ __forceinline__ void md_weights(float f, float (&w)[MdTaps<CUBIC>::N]) {
    if constexpr (CUBIC) {
        const float sixth = 1.0f / 6.0f;
        w[0] = -f * (f - 1.0f) * (f - 2.0f) * sixth;
        w[1] = (f + 1.0f) * (f - 1.0f) * (f - 2.0f) * 0.5f;
        w[2] = -(f + 1.0f) * f * (f - 2.0f) * 0.5f;
        w[3] = (f + 1.0f) * f * (f - 1.0f) * sixth;
    } else {
        w[0] = 1.0f - f;
        w[1] = f;
    }
}

// l'_j(f)
template <int CUBIC>
__device__ __forceinline__ void md_slopes(float f, float (&w)[MdTaps<CUBIC>::N]) {
    if constexpr (CUBIC) {
        const float q = 3.0f * f * f, sixth = 1.0f / 6.0f;
        w[0] = -(q - 6.0f * f + 2.0f) * sixth;
        w[1] = (q - 4.0f * f - 1.0f) * 0.5f;
        w[2] = -(q - 2.0f * f - 2.0f) * 0.5f;
        w[3] = (q - 1.0f) * sixth;
    } else {
        w[0] = -1.0f;
        w[1] = 1.0f;
    }
}

// how far below a sample the row's voices read: the largest floor(d) + 2, at most S
__device__ __forceinline__ int md_reach(const float* __restrict__ delay, const float* __restrict__ depth, int64_t r, int V,
                                        int Dmax) {
    int h = 1;
    for (int v = 0; v < V; ++v) {
        const int i = md_floor_at((double)delay[r * V + v], fabs((double)depth[r * V + v]), Dmax);
        h = i > h ? i : h;
    }
    return h + 2;
}

// xs[idx] = sample n0 - H + idx of a row-channel, 0 <= idx < H + left: the state (S samples, oldest first) or zero below 0.
// Four loads per lane are in flight: each reads a clamped, always valid address of x without a branch, and only the
// tiles that reach below the row's start look at the state afterwards.
__device__ __forceinline__ void md_stage(float* xs, const float* __restrict__ xrow, const float* __restrict__ zrow, int S,
                                         int64_t n0, int H, int left) {
    const int n = H + left;
    const bool below = n0 < H;
    for (int base = threadIdx.x; base < n; base += 4 * MD_THREADS) {
        float v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * MD_THREADS;
            const int64_t k = n0 - H + (idx < n ? idx : n - 1);
            v[u] = xrow[k > 0 ? k : 0];
        }
        if (below) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + u * MD_THREADS;
                const int64_t k = n0 - H + (idx < n ? idx : n - 1);
                if (k < 0) v[u] = zrow ? zrow[S + k] : 0.0f;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int idx = base + u * MD_THREADS;
            if (idx < n) xs[idx] = v[u];
        }
    }
}

template <int CUBIC>
__global__ __launch_bounds__(MD_THREADS) void md_fwd_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                            const float* __restrict__ delay, const float* __restrict__ depth,
                                                            const float* __restrict__ rate, const float* __restrict__ phase,
                                                            const float* __restrict__ gain, const float* __restrict__ dry,
                                                            const float* __restrict__ zi, const int64_t* __restrict__ pos,
                                                            MdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float md_lds[];
    constexpr int NT = MdTaps<CUBIC>::N, J0 = MdTaps<CUBIC>::J0;
    float* xs = md_lds;
    const int t = threadIdx.x, V = a.V, C = a.C;
    const int64_t item = blockIdx.x;
    const int64_t r = item / a.ntiles, tile = item - r * a.ntiles;
    const int64_t n0 = tile * MD_TILE;
    const int left = (int)(a.L - n0 < MD_TILE ? a.L - n0 : MD_TILE);
    const int64_t p0 = (pos ? pos[r] : 0) + n0;
    const int H = md_reach(delay, depth, r, V, a.Dmax);
    const float dr = dry[r];
    for (int c = 0; c < C; ++c) {
        const float* xrow = x + row_off(a.xmap, r, c);
        const float* zrow = zi ? zi + (r * C + c) * (int64_t)a.S : nullptr;
        __syncthreads();                                 // (the channel before has been read)
        md_stage(xs, xrow, zrow, a.S, n0, H, left);
        __syncthreads();
        float acc[MD_PER_LANE];
#pragma unroll
        for (int q = 0; q < MD_PER_LANE; ++q) {
            const int tt = t + q * MD_THREADS;
            acc[q] = tt < left ? dr * xs[H + tt] : 0.0f;
        }
        for (int v = 0; v < V; ++v) {
            const double dl = (double)delay[r * V + v], dp = (double)depth[r * V + v], rt = (double)rate[r * V + v];
            const double ph = (double)phase[(r * V + v) * C + c];
            const float g = gain[(r * V + v) * C + c];
#pragma unroll
            for (int q = 0; q < MD_PER_LANE; ++q) {
                const int tt = t + q * MD_THREADS;
                if (tt >= left) continue;
                float f, w[NT];
                bool open;
                int i = md_split(dl, dp, sinpi(2.0 * md_phase(rt, ph, p0 + tt)), a.Dmax, f, open);
                i = i > H - 2 ? H - 2 : i;               // (never binds: H covers the swing)
                md_weights<CUBIC>(f, w);
                const float* at = xs + (H + tt - i - J0);   // x[n - i - J0], the first node
#pragma unroll
                for (int j = 0; j < NT; ++j) acc[q] = fmaf(g * w[j], at[-j], acc[q]);
            }
        }
        float* yrow = y + row_off(a.ymap, r, c);
#pragma unroll
        for (int q = 0; q < MD_PER_LANE; ++q) {
            const int tt = t + q * MD_THREADS;
            if (tt < left) yrow[n0 + tt] = acc[q];
        }
    }
}

// gx for the samples k0 .. k0 + left - 1 of a row.  Per voice and channel, local index idx stands for the output sample
// n = nlo + idx, nlo = k0 + J0 + imin the first n that can read the tile (imin, imax: floor(d) at the ends of the swing);
// ms[idx] = (n - i(n)) - (k0 + J0) + Dmax = idx + imin - i(n) + Dmax > 0.  Sample k = k0 + tt is read through node j by
// the n with ms = tt + Dmax + (j - J0), all of them inside idx in [tt, tt + (imax - imin) + taps).
template <int CUBIC>
__global__ __launch_bounds__(MD_THREADS) void md_bwd_x_kernel(const float* __restrict__ gy, float* __restrict__ gx,
                                                              const float* __restrict__ delay, const float* __restrict__ depth,
                                                              const float* __restrict__ rate, const float* __restrict__ phase,
                                                              const float* __restrict__ gain, const float* __restrict__ dry,
                                                              MdArgs a, int cap) {
    extern __shared__ __attribute__((aligned(16))) float md_lds[];
    constexpr int NT = MdTaps<CUBIC>::N, J0 = MdTaps<CUBIC>::J0;
    float* fs = md_lds;
    uint16_t* ms = reinterpret_cast<uint16_t*>(fs + cap);
    const int t = threadIdx.x, V = a.V, C = a.C, Dmax = a.Dmax;
    const int64_t item = blockIdx.x;
    const int64_t r = item / a.ntiles, tile = item - r * a.ntiles;
    const int64_t k0 = tile * MD_TILE;
    const int left = (int)(a.L - k0 < MD_TILE ? a.L - k0 : MD_TILE);
    const float dr = dry[r];
    for (int c = 0; c < C; ++c) {
        const float* grow = gy + row_off(a.gmap, r, c);
        float acc[MD_PER_LANE];
#pragma unroll
        for (int q = 0; q < MD_PER_LANE; ++q) {
            const int tt = t + q * MD_THREADS;
            acc[q] = tt < left ? dr * grow[k0 + tt] : 0.0f;
        }
        for (int v = 0; v < V; ++v) {
            const double dl = (double)delay[r * V + v], dp = (double)depth[r * V + v], rt = (double)rate[r * V + v];
            const double ph = (double)phase[(r * V + v) * C + c];
            const float g = gain[(r * V + v) * C + c];
            const int imin = md_floor_at(dl, -fabs(dp), Dmax), imax = md_floor_at(dl, fabs(dp), Dmax);
            const int64_t nlo = k0 + J0 + imin;          // >= 0: imin >= 1
            const int64_t room = a.L - nlo;
            int nn = left + NT - 1 + imax - imin;
            nn = nn > cap ? cap : nn;                    // (never binds: cap = tile + Dmax + 4)
            nn = room < nn ? (int)(room < 0 ? 0 : room) : nn;
            __syncthreads();                             // (the voice before has been read)
            for (int idx = t; idx < nn; idx += MD_THREADS) {
                float f;
                bool open;
                int i = md_split(dl, dp, sinpi(2.0 * md_phase(rt, ph, nlo + idx)), Dmax, f, open);
                i = i < imin ? imin : i > imax ? imax : i;   // (never binds)
                fs[idx] = f;
                ms[idx] = (uint16_t)(idx + imin - i + Dmax);
            }
            __syncthreads();
            const int span = imax - imin + NT;
#pragma unroll
            for (int q = 0; q < MD_PER_LANE; ++q) {
                const int tt = t + q * MD_THREADS;
                if (tt >= left) continue;
                const int key = tt + Dmax;
                int lo = tt < nn ? tt : nn, hi = tt + span < nn ? tt + span : nn;
                while (lo < hi) {                        // the first idx with ms >= key
                    const int mid = (lo + hi) >> 1;
                    if ((int)ms[mid] >= key) hi = mid; else lo = mid + 1;
                }
                for (int step = 0; step < 2 * NT && lo < nn; ++step, ++lo) {
                    const int jj = (int)ms[lo] - key;    // j - J0
                    if (jj >= NT) break;
                    if (jj < 0) continue;                // (only outside the contract)
                    float w[NT];
                    md_weights<CUBIC>(fs[lo], w);
                    float wj = w[0];
#pragma unroll
                    for (int j = 1; j < NT; ++j) wj = jj == j ? w[j] : wj;
                    acc[q] = fmaf(g * wj, grow[nlo + lo], acc[q]);
                }
            }
        }
        float* orow = gx + row_off(a.ymap, r, c);
#pragma unroll
        for (int q = 0; q < MD_PER_LANE; ++q) {
            const int tt = t + q * MD_THREADS;
            if (tt < left) orow[k0 + tt] = acc[q];
        }
    }
}

// The tile's share of the six parameter gradients, P = 1 + 3 V + 2 V C doubles at part[item P]:
// dry | delay[V] | depth[V] | rate[V] | phase[V, C] | gain[V, C].
template <int CUBIC>
__global__ __launch_bounds__(MD_THREADS) void md_bwd_par_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                                const float* __restrict__ delay, const float* __restrict__ depth,
                                                                const float* __restrict__ rate, const float* __restrict__ phase,
                                                                const float* __restrict__ gain, double* __restrict__ part,
                                                                MdArgs a) {
    extern __shared__ __attribute__((aligned(16))) float md_lds[];
    constexpr int NT = MdTaps<CUBIC>::N, J0 = MdTaps<CUBIC>::J0, K = 6;
    __shared__ double red[MD_WAVES][K];
    __shared__ double tot[3 * MD_MAX_VOICES + 1];        // delay, depth, rate per voice and dry, summed over the channels
    float* xs = md_lds;
    const int t = threadIdx.x, V = a.V, C = a.C, lane = t & 63, wave = t >> 6;
    const int64_t item = blockIdx.x;
    const int64_t r = item / a.ntiles, tile = item - r * a.ntiles;
    const int64_t n0 = tile * MD_TILE;
    const int left = (int)(a.L - n0 < MD_TILE ? a.L - n0 : MD_TILE);
    const int H = md_reach(delay, depth, r, V, a.Dmax);
    double* out = part + item * (int64_t)(1 + 3 * V + 2 * V * C);
    if (t < 3 * MD_MAX_VOICES + 1) tot[t] = 0.0;
    for (int c = 0; c < C; ++c) {
        const float* xrow = x + row_off(a.xmap, r, c);
        const float* grow = gy + row_off(a.gmap, r, c);
        __syncthreads();
        md_stage(xs, xrow, nullptr, a.S, n0, H, left);
        __syncthreads();
        for (int v = 0; v < V; ++v) {
            const double dl = (double)delay[r * V + v], dp = (double)depth[r * V + v], rt = (double)rate[r * V + v];
            const double ph = (double)phase[(r * V + v) * C + c];
            const double g = (double)gain[(r * V + v) * C + c];
            double s[K] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};        // delay, depth, rate, phase, gain, dry
            for (int tt = t; tt < left; tt += MD_THREADS) {
                float f, w[NT], dw[NT];
                bool open;
                double sn, cs;
                sincospi(2.0 * md_phase(rt, ph, n0 + tt), &sn, &cs);
                int i = md_split(dl, dp, sn, a.Dmax, f, open);
                i = i > H - 2 ? H - 2 : i;
                md_weights<CUBIC>(f, w);
                md_slopes<CUBIC>(f, dw);
                const float* at = xs + (H + tt - i - J0);
                float u = 0.0f, du = 0.0f;
#pragma unroll
                for (int j = 0; j < NT; ++j) {
                    u = fmaf(w[j], at[-j], u);
                    du = fmaf(dw[j], at[-j], du);
                }
                const double gg = (double)grow[n0 + tt];
                const double e = open ? gg * g * (double)du : 0.0;
                const double ec = e * dp * MD_TWO_PI * cs;
                s[0] += e;
                s[1] += e * sn;
                s[2] += ec * (double)(n0 + tt);
                s[3] += ec;
                s[4] += gg * (double)u;
                if (v == 0) s[5] += gg * (double)xs[H + tt];
            }
            block_sums<K, MD_WAVES>(s, red, lane, wave, [&](double sum) {
                if (t < 3) tot[t * MD_MAX_VOICES + v] += sum;
                else if (t == 3) out[1 + 3 * V + v * C + c] = sum;
                else if (t == 4) out[1 + 3 * V + V * C + v * C + c] = sum;
                else if (v == 0) tot[3 * MD_MAX_VOICES] += sum;
            });
            __syncthreads();
        }
    }
    if (t < 3 * V) out[1 + t] = tot[(t / V) * MD_MAX_VOICES + t % V];
    if (t == 0) out[0] = tot[3 * MD_MAX_VOICES];
}

// a row's tile sums -> its parameter gradients (tile_sums_finish_kernel): dry, three blocks of V, two blocks of V C; a null
// destination is skipped
struct MdSlots {
    float *g_delay, *g_depth, *g_rate, *g_phase, *g_gain, *g_dry;
    int V, C;
    __device__ float* dest(int64_t r, int64_t slot, double&) const {
        const int64_t VC = (int64_t)V * C;
        if (slot == 0) return g_dry ? g_dry + r : nullptr;
        if (slot <= 3 * V) {
            const int64_t which = (slot - 1) / V, v = (slot - 1) - which * V;
            float* base = which == 0 ? g_delay : which == 1 ? g_depth : g_rate;
            return base ? base + r * V + v : nullptr;
        }
        const int64_t q = slot - 1 - 3 * V;
        return q < VC ? (g_phase ? g_phase + r * VC + q : nullptr) : (g_gain ? g_gain + r * VC + (q - VC) : nullptr);
    }
};

// the checks both entries share, then the tile geometry
static int md_prepare(const float* x, gfx_rowmap_t xmap, int64_t R, int64_t C, int64_t L, int64_t V, int64_t interp,
                      int64_t max_delay, const float* delay, const float* depth, const float* rate, const float* phase,
                      const float* gain, const float* dry, MdArgs& a) {
    if (!x || !delay || !depth || !rate || !phase || !gain || !dry) return GFX_EINVAL;
    if (R <= 0 || C <= 0 || L <= 0 || R > 0x7fffffffLL || C > 0x7fffffffLL || xmap.inner <= 0) return GFX_EINVAL;
    if (V < 1 || V > MD_MAX_VOICES || (interp != 0 && interp != 1) || max_delay < 2 || max_delay > MD_MAX_DELAY) return GFX_EINVAL;
    if (R * C > 0x7fffffffLL || L > INT64_MAX / 4) return GFX_EINVAL;
    const int64_t ntiles = (L + MD_TILE - 1) / MD_TILE;
    if (ntiles > MAX_GRID_X / R) return GFX_EINVAL;                    // grid.x of the tile kernels
    a.xmap = a.ymap = a.gmap = xmap;
    a.L = L; a.ntiles = ntiles;
    a.C = (int)C; a.V = (int)V; a.Dmax = (int)max_delay; a.S = (int)max_delay + 2;
    return GFX_OK;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_moddelay_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L, int64_t V,
                     int64_t interp, int64_t max_delay, const float* delay, const float* depth, const float* rate,
                     const float* phase, const float* gain, const float* dry, const float* zi, const int64_t* pos_in, float* zf,
                     int64_t* pos_out, void* stream) {
    MdArgs a;
    if (!y || ymap.inner <= 0) return GFX_EINVAL;
    const int rc = md_prepare(x, xmap, R, C, L, V, interp, max_delay, delay, depth, rate, phase, gain, dry, a);
    if (rc != GFX_OK) return rc;
    if (!zi != !pos_in || !zf != !pos_out) return GFX_EINVAL;          // a state is its history and its position
    // tiles read each other's halos of x: never in place
    if (map_negative(xmap) || map_negative(ymap) || signals_overlap(y, ymap, x, xmap, R, C, L)) return GFX_EINVAL;
    if (!history_pair_ok(zi, zf, R, C, a.S)) return GFX_EINVAL;        // (past 2^30 state rows: refused before any launch)
    if (zi && zf && pos_in < pos_out + R && pos_out < pos_in + R) return GFX_EINVAL;
    a.ymap = ymap;
    const size_t lds = sizeof(float) * (size_t)(MD_TILE + a.S);
    auto fwd = interp ? md_fwd_kernel<1> : md_fwd_kernel<0>;
    hipStream_t st = (hipStream_t)stream;
    if (launch(fwd, dim3((unsigned)(R * a.ntiles)), dim3(MD_THREADS), lds, st, x, y, delay, depth, rate, phase, gain, dry, zi,
               pos_in, a) != GFX_OK)
        return GFX_ELAUNCH;
    if (zf) return launch_history_tail(x, xmap, zi, zf, R, C, L, a.S, pos_in, pos_out, st);   // and the rows' positions, moved on by L
    return GFX_OK;
}

size_t gfx_moddelay_bwd_ws_bytes(int64_t R, int64_t C, int64_t L, int64_t V) {
    if (R <= 0 || C <= 0 || L <= 0 || V < 1 || V > MD_MAX_VOICES) return 0;
    return sizeof(double) * (size_t)R * (size_t)((L + MD_TILE - 1) / MD_TILE) * (size_t)(1 + 3 * V + 2 * V * C);
}

int gfx_moddelay_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R, int64_t C, int64_t L,
                         int64_t V, int64_t interp, int64_t max_delay, const float* delay, const float* depth, const float* rate,
                         const float* phase, const float* gain, const float* dry, float* gx, gfx_rowmap_t gxmap, float* g_delay,
                         float* g_depth, float* g_rate, float* g_phase, float* g_gain, float* g_dry, void* ws, size_t ws_bytes,
                         void* stream) {
    MdArgs a;
    if (!gy || gmap.inner <= 0) return GFX_EINVAL;
    const int rc = md_prepare(x, xmap, R, C, L, V, interp, max_delay, delay, depth, rate, phase, gain, dry, a);
    if (rc != GFX_OK) return rc;
    const bool params = g_delay || g_depth || g_rate || g_phase || g_gain || g_dry;
    if (!gx && !params) return GFX_EINVAL;
    if (map_negative(xmap) || map_negative(gmap)) return GFX_EINVAL;
    if (!grad_out_ok(gx, gxmap, x, xmap, gy, gmap, R, C, L)) return GFX_EINVAL;
    if (params) {
        const int wrc = workspace_ok(ws, ws_bytes, gfx_moddelay_bwd_ws_bytes(R, C, L, V), alignof(double));
        if (wrc != GFX_OK) return wrc;
    }
    a.gmap = gmap;
    a.ymap = gx ? gxmap : xmap;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(R * a.ntiles));
    if (gx) {
        const int cap = MD_TILE + a.Dmax + 4;            // even: the 16-bit positions behind the floats stay aligned
        const size_t lds = (sizeof(float) + sizeof(uint16_t)) * (size_t)cap;
        auto bx = interp ? md_bwd_x_kernel<1> : md_bwd_x_kernel<0>;
        if (launch(bx, grid, dim3(MD_THREADS), lds, st, gy, gx, delay, depth, rate, phase, gain, dry, a, cap) != GFX_OK)
            return GFX_ELAUNCH;
    }
    if (params) {
        double* part = static_cast<double*>(ws);
        const size_t lds = sizeof(float) * (size_t)(MD_TILE + a.S);
        auto bp = interp ? md_bwd_par_kernel<1> : md_bwd_par_kernel<0>;
        if (launch(bp, grid, dim3(MD_THREADS), lds, st, x, gy, delay, depth, rate, phase, gain, part, a) != GFX_OK)
            return GFX_ELAUNCH;
        return finish_tile_sums(MdSlots{g_delay, g_depth, g_rate, g_phase, g_gain, g_dry, (int)V, (int)C}, part, R,
                                1 + 3 * V + 2 * V * C, a.ntiles, st);
    }
    return GFX_OK;
}

}  // extern "C"
