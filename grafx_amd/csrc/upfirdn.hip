// Rational polyphase FIR ("upfirdn") of rows that share one set of taps, and the largest magnitude of its output (gfx950):
// sample-rate conversion, its adjoint, and the oversampled peak of a true-peak meter.
//
//     y[r, c, m] = sum_k x[r, c, k] h[m down + offset - k up],   0 <= m < M,   x zero outside [0, L), h zero outside [0, N)
//
// With p = m down + offset, q = floor(p / up) and ph = p mod up the sum runs over the taps of phase ph:
//     y[m] = sum_j h[ph + j up] x[q - j],   0 <= j <= (N - 1 - ph) / up,
// about N / up products per output.  The adjoint is the same formula with up and down exchanged, the taps reversed and
// offset' = N - 1 - offset, so one kernel serves forward and backward.
//
// A tile is GFX_UPFIRDN_TILE = 1024 consecutive outputs of one row-channel, one workgroup of 256 lanes, lane t owning the
// outputs t, t + 256, ... (coalesced stores).  The workgroup stages the taps in LDS once, then goes through the tile in
// passes of `sub` outputs: the span of x under a pass, ((sub - 1) down + N - 1) / up + 3 samples at most, is staged with
// zeros outside [0, L), so the inner loop has no bounds to check.  sub is the whole tile whenever that span is within
// 8192 samples (every ratio a resampler meets: 1144 samples for 147/160 with 1939 taps, 2857 for 441/160 with 5345) and
// halves until it is; a pass of one output always fits, whatever the ratio (N / up + 3 <= 16387 samples).
//
// The taps sit PHASE-MAJOR in LDS, every phase reversed and padded to J = ceil(N / up) slots: slot s of phase ph holds
// h[ph + (J - 1 - s) up], and slot 0 is 0 for the phases that have J - 1 taps (or none, where N < up).  An output then reads
// two runs of consecutive words, g[0 .. J) of its phase and x[q - (J - 1) .. q], in ascending k: the addresses inside a run
// are immediates of ds_read(2)_b32, the trip count is the same for every lane, and a product costs its two LDS reads and
// one fused multiply-add (with the taps in their natural order, h[ph + j up] and a skew against bank conflicts cost twelve
// vector instructions a product: 0.48 ms against 0.36 ms for 256 x 2 x 131072 samples, 147/160).  Slot 0 is used
// under a select, not multiplied by its zero, so a sample outside an output's window never reaches it.  A phase's row starts
// at ph (J | 1) + ph / 32: the odd pitch spreads neighbouring lanes' phases (which advance by down mod up) over the banks,
// and the second term does when that step is a multiple of 32 (441/160: 160).  x is staged as it is: neighbouring lanes
// read it down / up words apart, which is conflict-free except for decimation by an even factor (2-way for 2, 4-way for 4).
// The first output's quotient and phase are the only divisions of a lane; the next ones follow by addition.
//
#include "common.hpp"

namespace gfx {

constexpr int UF_TILE = GFX_UPFIRDN_TILE;
constexpr int UF_THREADS = 256;
constexpr int UF_MAX_RATIO = 1024;
constexpr int UF_MAX_TAPS = 16384;
constexpr int UF_SPAN_PREF = 8192;               // samples of x a pass stages, where a pass of more than one output can choose
constexpr int UF_FIN_WAVES = 4;

struct UfPart {          // a tile's largest |y| and the lowest output index that attains it
    float v;
    int pad;
    int64_t m;
};
static_assert(sizeof(UfPart) == 16, "UfPart layout");

struct UfArgs {
    gfx_rowmap_t xmap, ymap;
    int64_t L, M, ntiles;
    int C, N, up, down, offset, sub, accumulate;
    int J, Jp, phs;          // slots per phase, the row pitch J | 1, the first phase whose slot 0 holds no tap
    int hwords;              // words of the tap table
};

// samples of x under `n` consecutive outputs, at most (one more than the taps reach: slot 0 of a short phase)
static inline int64_t uf_span(int64_t n, int64_t N, int64_t up, int64_t down) { return ((n - 1) * down + N - 1) / up + 3; }

template <bool PEAK>
__global__ __launch_bounds__(UF_THREADS) void upfirdn_kernel(const float* __restrict__ x, const float* __restrict__ h,
                                                            float* __restrict__ y, UfPart* __restrict__ part, UfArgs a) {
    extern __shared__ __attribute__((aligned(16))) float uf_lds[];
    float* hp = uf_lds;                 // the taps, phase-major
    float* xs = uf_lds + a.hwords;      // the pass's span of x
    const int t = threadIdx.x;
    const int64_t item = blockIdx.x;
    const int64_t rc = item / a.ntiles, tile = item - rc * a.ntiles;
    const int64_t r = rc / a.C;
    const int c = (int)(rc - r * a.C);
    const int J = a.J, up = a.up;
    for (int ph = a.phs + t; ph < up; ph += UF_THREADS) hp[ph * a.Jp + (ph >> 5)] = 0.0f;
    {
        const int dq = UF_THREADS / up, dr = UF_THREADS - dq * up;
        int jj = t / up, ph = t - jj * up;                        // tap i = ph + jj up
        for (int i = t; i < a.N; i += UF_THREADS) {
            hp[ph * a.Jp + (ph >> 5) + (J - 1 - jj)] = h[i];
            ph += dr;
            jj += dq;
            if (ph >= up) {
                ph -= up;
                ++jj;
            }
        }
    }

    const int64_t m0 = tile * UF_TILE;
    // k up of the sample before the first one any output of the tile can reach, split into kbase up + r0
    const int64_t lo = m0 * a.down + a.offset - (a.N - 1) - up;
    const int64_t kbase = floor_div(lo, up);
    const int r0 = (int)(lo - kbase * up);                        // 0 .. up - 1
    const int left = (int)(a.M - m0 < UF_TILE ? a.M - m0 : UF_TILE);
    const float* xrow = x + row_off(a.xmap, r, c);
    float* yrow = PEAK ? nullptr : y + row_off(a.ymap, r, c) + m0;
    const int sq = UF_THREADS * a.down / up, sr = UF_THREADS * a.down - sq * up;   // a lane's next output: 256 down further
    float bv = -1.0f;
    int bi = 0x7fffffff;

    for (int ia = 0; ia < left; ia += a.sub) {
        const int n = left - ia < a.sub ? left - ia : a.sub;
        const int kw0 = (ia * a.down + r0) / up;                                // first and last sample of the pass, from kbase
        const int kw1 = ((ia + n - 1) * a.down + a.N - 1 + up + r0) / up;
        __syncthreads();                                                        // the pass before has read its span
        for (int w = t; w <= kw1 - kw0; w += UF_THREADS) {
            const int64_t k = kbase + kw0 + w;
            xs[w] = k >= 0 && k < a.L ? xrow[k] : 0.0f;
        }
        __syncthreads();
        int i = ia + t;
        if (i < ia + n) {
            const int p = i * a.down + a.N - 1 + up + r0;                       // m down + offset - kbase up
            int q = p / up, ph = p - q * up;
            for (; i < ia + n; i += UF_THREADS) {
                const float* g = hp + ph * a.Jp + (ph >> 5);
                const float* xv = xs + (q - (J - 1) - kw0);                     // ascending k: g[s] x[q - (J - 1) + s]
                float acc = ph < a.phs ? fmaf(g[0], xv[0], 0.0f) : 0.0f;
#pragma unroll 4
                for (int s = 1; s < J; ++s) acc = fmaf(g[s], xv[s], acc);
                if (PEAK) {
                    const float v = fabsf(acc);
                    if (v > bv) {                                               // (i ascends: the lowest index stays)
                        bv = v;
                        bi = i;
                    }
                } else {
                    yrow[i] = a.accumulate ? yrow[i] + acc : acc;
                }
                ph += sr;
                q += sq;
                if (ph >= up) {
                    ph -= up;
                    ++q;
                }
            }
        }
    }
    if (PEAK) {
        __shared__ float rv[UF_THREADS];
        __shared__ int ri[UF_THREADS];
        rv[t] = bv;
        ri[t] = bi;
        __syncthreads();
        for (int s = UF_THREADS / 2; s > 0; s >>= 1) {
            if (t < s) {
                const float v = rv[t + s];
                const int i = ri[t + s];
                if (v > rv[t] || (v == rv[t] && i < ri[t])) {
                    rv[t] = v;
                    ri[t] = i;
                }
            }
            __syncthreads();
        }
        if (t == 0) part[item] = UfPart{rv[0], 0, m0 + ri[0]};
    }
}

// one wave per row-channel: a lane takes every 64th tile, then the wave's pairs meet in a butterfly
__global__ __launch_bounds__(64 * UF_FIN_WAVES) void uf_absmax_finish_kernel(const UfPart* __restrict__ part,
                                                                           float* __restrict__ peak, int64_t* __restrict__ index,
                                                                           int64_t rcs, int64_t ntiles) {
    const int64_t rc = (int64_t)blockIdx.x * UF_FIN_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (rc >= rcs) return;   // (a whole wave; the kernel has no barrier)
    const UfPart* row = part + rc * ntiles;
    float bv = -1.0f;
    int64_t bm = INT64_MAX;
    for (int64_t q = lane; q < ntiles; q += 64) {
        const UfPart p = row[q];
        if (p.v > bv || (p.v == bv && p.m < bm)) {
            bv = p.v;
            bm = p.m;
        }
    }
#pragma unroll
    for (int d = 1; d < 64; d *= 2) {
        const float v = __shfl_xor(bv, d);
        const int64_t m = __shfl_xor((long long)bm, d);
        if (v > bv || (v == bv && m < bm)) {
            bv = v;
            bm = m;
        }
    }
    if (lane == 0) {
        peak[rc] = bv;
        index[rc] = bm;
    }
}

static inline int64_t uf_tiles(int64_t M) { return (M + UF_TILE - 1) / UF_TILE; }

// the checks both entries share, then the geometry and the LDS the tile kernel needs
static int uf_prepare(const float* x, gfx_rowmap_t xmap, const float* h, int64_t N, int64_t up, int64_t down, int64_t offset,
                      int64_t R, int64_t C, int64_t L, int64_t M, UfArgs& a, size_t& lds) {
    if (!x || !h || R <= 0 || C <= 0 || L <= 0 || M <= 0 || xmap.inner <= 0) return GFX_EINVAL;
    if (up < 1 || up > UF_MAX_RATIO || down < 1 || down > UF_MAX_RATIO || N < 1 || N > UF_MAX_TAPS || offset < 0 || offset >= N)
        return GFX_EINVAL;
    if (R > 0x7fffffffLL || C > 0x7fffffffLL || R * C > 0x7fffffffLL) return GFX_EINVAL;
    if (M > INT64_MAX / (2 * UF_MAX_RATIO)) return GFX_EINVAL;             // m down + offset stays in 64 bits
    const int64_t ntiles = uf_tiles(M);
    if (ntiles > MAX_GRID_X / (R * C)) return GFX_EINVAL;               // grid.x of the tile kernel
    int64_t sub = UF_TILE;
    while (sub > 1 && uf_span(sub, N, up, down) > UF_SPAN_PREF) sub /= 2;
    a.xmap = xmap;
    a.ymap = xmap;
    a.L = L; a.M = M; a.ntiles = ntiles;
    a.C = (int)C; a.N = (int)N; a.up = (int)up; a.down = (int)down; a.offset = (int)offset; a.sub = (int)sub;
    a.accumulate = 0;
    a.J = (int)((N + up - 1) / up);
    a.Jp = a.J | 1;
    a.phs = (int)(N - (a.J - 1) * up);
    a.hwords = (int)(up * a.Jp + (up >> 5) + 1);
    lds = sizeof(float) * (size_t)(a.hwords + uf_span(sub, N, up, down));
    return GFX_OK;
}

template <bool PEAK>
static int uf_launch(const float* x, const float* h, float* y, UfPart* part, const UfArgs& a, int64_t rcs, size_t lds,
                     hipStream_t s) {
    if (allow_lds(upfirdn_kernel<PEAK>, lds) != GFX_OK) return GFX_ELAUNCH;
    hipLaunchKernelGGL(upfirdn_kernel<PEAK>, dim3((unsigned)(rcs * a.ntiles)), dim3(UF_THREADS), lds, s, x, h, y, part, a);
    return GFX_OK;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_upfirdn_f32(const float* x, gfx_rowmap_t xmap, const float* h, int64_t N, int64_t up, int64_t down, int64_t offset,
                    float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L, int64_t M, int accumulate, void* stream) {
    UfArgs a;
    size_t lds;
    if (!y || ymap.inner <= 0) return GFX_EINVAL;
    const int rc = uf_prepare(x, xmap, h, N, up, down, offset, R, C, L, M, a, lds);
    if (rc != GFX_OK) return rc;
    a.ymap = ymap;
    a.accumulate = accumulate != 0;
    if (uf_launch<false>(x, h, y, nullptr, a, R * C, lds, (hipStream_t)stream) != GFX_OK) return GFX_ELAUNCH;
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

size_t gfx_upfirdn_absmax_ws_bytes(int64_t R, int64_t C, int64_t M) {
    if (R <= 0 || C <= 0 || M <= 0) return 0;
    return (size_t)R * (size_t)C * (size_t)uf_tiles(M) * sizeof(UfPart);
}

int gfx_upfirdn_absmax_f32(const float* x, gfx_rowmap_t xmap, const float* h, int64_t N, int64_t up, int64_t down,
                           int64_t offset, float* peak, int64_t* index, int64_t R, int64_t C, int64_t L, int64_t M, void* ws,
                           size_t ws_bytes, void* stream) {
    UfArgs a;
    size_t lds;
    if (!peak || !index || !ws || (reinterpret_cast<uintptr_t>(ws) & 15) || (reinterpret_cast<uintptr_t>(index) & 7))
        return GFX_EINVAL;
    const int rc = uf_prepare(x, xmap, h, N, up, down, offset, R, C, L, M, a, lds);
    if (rc != GFX_OK) return rc;
    if (ws_bytes < gfx_upfirdn_absmax_ws_bytes(R, C, M)) return GFX_ENOSPC;
    hipStream_t s = (hipStream_t)stream;
    UfPart* part = reinterpret_cast<UfPart*>(ws);
    const int64_t rcs = R * C;
    if (uf_launch<true>(x, h, nullptr, part, a, rcs, lds, s) != GFX_OK) return GFX_ELAUNCH;
    hipLaunchKernelGGL(uf_absmax_finish_kernel, dim3((unsigned)((rcs + UF_FIN_WAVES - 1) / UF_FIN_WAVES)),
                       dim3(64 * UF_FIN_WAVES), 0, s, part, peak, index, rcs, a.ntiles);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
