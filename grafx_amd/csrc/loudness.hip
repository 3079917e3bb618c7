// Block energies of a two-section biquad cascade whose coefficients are shared by every row of the call -- the K-weighting of
// ITU-R BS.1770 in front of a loudness meter -- and the gradient of those energies with respect to the signal (gfx950).
// Recursion, states, squares and sums in double: the second K-weighting section is a 38 Hz high-pass with poles at radius
// 0.995 and a double zero at DC, and a float32 recursion misses 1e-5 on its block energies by a factor of 50 on bass-heavy
// material.
//
// Per row-channel, a0-normalised, from silence:
//     w1[n] = x[n] - a11 w1[n-1] - a12 w1[n-2],   u[n] = b10 w1[n] + b11 w1[n-1] + b12 w1[n-2]
//     w2[n] = u[n] - a21 w2[n-1] - a22 w2[n-2],   y[n] = b20 w2[n] + b21 w2[n-1] + b22 w2[n-2]
//     energy[k] = sum of y[n]^2 over k hop <= n < (k + 1) hop,   k < n_sub = L / hop.
// The cascade is one linear system on the state s = (w1[n-1], w1[n-2], w2[n-1], w2[n-2]): s' = A s + (x, 0, b10 x, 0), and A
// is the same for every row.  So nothing has to be walked from start to end: a run of samples started from silence ends in a
// state z, and started from s it ends in A^len s + z.  The powers of A that this needs are constants of the call, built on
// the host in extended precision (KwConst).
//
// A tile is 1024 samples of one row-channel, one wave: 64 lanes x 16 samples (with 8 the scans weigh twice as much per
// sample: measured 0.29 against 0.20 ms forward, 0.64 against 0.43 ms backward for 512 row-channels of 131072 samples).
// Forward, four launches:
//   1. kw_tile_state_kernel   every tile from silence: the lanes' z, combined over the wave by a shift-and-add scan with
//                             A^(16 * 2^d), d < 6 (kw_scan); the tile's end state goes to the workspace.
//   2. kw_carry_kernel        one wave per row-channel turns the tiles' end states into the states ENTERING the tiles: the
//                             same scan over 64 tiles at a time with A^(1024 * 2^d), the carry from group to group.
//   3. kw_main_kernel<0>      every tile again, from its entering state: y, y^2 and the sums per sub-block.  A sub-block
//                             inside one tile is stored; of one that crosses a tile edge the tile stores its part.
//   4. kw_energy_finish_kernel  adds the parts of every sub-block that crosses a tile edge, in the order of the tiles.
// Backward (the gradient of sum genergy * energy): v[n] = 2 genergy[n / hop] y[n] (0 from n_sub hop on), and gx is the
// adjoint cascade applied to v -- the same recursion run over the reversed signal.  Launches 1 and 2 rebuild the entering
// states from x; kw_main_kernel<1> recomputes y and v per tile and runs the recursion over v backwards from silence (the
// lanes from 63 down, kw_scan<-1>), leaving the tile's adjoint end state; kw_carry_kernel over the tiles from the last to
// the first; kw_main_kernel<2> recomputes y and v once more and runs the adjoint from its entering state into gx, every
// sample stored once (or added to what gx holds).  Nothing of the signal's size is kept between forward and backward, and
// the workspace is 64 bytes per tile: the forward state (32 B) and the adjoint state or the two energy parts.
// No atomics, every sum in a fixed order: two calls give the same bits, and a tile's arithmetic depends on its own
// row-channel alone.
#include "common.hpp"

namespace gfx {

constexpr int KW_E = 16;                  // samples per lane
constexpr int KW_TILE = 64 * KW_E;        // 1024 samples: one wave
constexpr int KW_WAVES = 4;               // tiles per workgroup, one wave each
constexpr int KW_WS = 8;                  // doubles per tile in the workspace: [0, 4) forward state, [4, 8) adjoint state / parts

struct S4 {
    double a, b, c, d;   // w1[n-1], w1[n-2], w2[n-1], w2[n-2]
};
// a power of A: block lower triangular, rows 0 and 1 hold two entries, rows 2 and 3 four
struct KwMat {
    double m[12];
};
struct KwConst {
    double b10, b11, b12, a11, a12, b20, b21, b22, a21, a22;
    KwMat lane[6];   // A^(16 * 2^d)
    KwMat tile[6];   // A^(1024 * 2^d)
};
struct KwArgs {
    gfx_rowmap_t xmap, gmap;
    int64_t L, Lv, hop, n_sub, ntiles, items, rcs;   // Lv = n_sub * hop; items = rcs * ntiles
    int C, xvec, gvec, accumulate;
};

__device__ __forceinline__ S4 kw_apply(const KwMat& M, const S4& s) {
    return {fma(M.m[0], s.a, M.m[1] * s.b), fma(M.m[2], s.a, M.m[3] * s.b),
            fma(M.m[4], s.a, fma(M.m[5], s.b, fma(M.m[6], s.c, M.m[7] * s.d))),
            fma(M.m[8], s.a, fma(M.m[9], s.b, fma(M.m[10], s.c, M.m[11] * s.d)))};
}
__device__ __forceinline__ void kw_add(S4& s, const S4& o) {
    s.a += o.a;
    s.b += o.b;
    s.c += o.c;
    s.d += o.d;
}
// one sample through both sections
__device__ __forceinline__ double kw_step(const KwConst& k, S4& s, double x) {
    const double w1 = fma(-k.a12, s.b, fma(-k.a11, s.a, x));
    const double u = fma(k.b10, w1, fma(k.b11, s.a, k.b12 * s.b));
    const double w2 = fma(-k.a22, s.d, fma(-k.a21, s.c, u));
    const double y = fma(k.b20, w2, fma(k.b21, s.c, k.b22 * s.d));
    s = {w1, s.a, w2, s.c};
    return y;
}
// the value of the lane `delta` before this one in the scan's direction, zero where there is none
template <int DIR>
__device__ __forceinline__ S4 kw_shift(const S4& v, int delta, int lane) {
    const int src = lane - DIR * delta;
    const bool ok = src >= 0 && src < 64;
    const S4 r = {__shfl(v.a, src & 63), __shfl(v.b, src & 63), __shfl(v.c, src & 63), __shfl(v.d, src & 63)};
    return ok ? r : S4{0.0, 0.0, 0.0, 0.0};
}
// z in: the end state of this lane's run from silence; out: the state ENTERING the lane's run, given c, the state entering
// the first lane (wave-uniform).  total: the state after the last lane.  P[d] = (the run's A^len)^(2^d).  DIR = 1: the runs
// follow each other from lane 0 up, DIR = -1: from lane 63 down.
template <int DIR>
__device__ __forceinline__ void kw_scan(const KwMat (&P)[6], const S4& c, int lane, S4& z, S4& total) {
    const int first = DIR > 0 ? 0 : 63;
    S4 inc = z;
    if (lane == first) kw_add(inc, kw_apply(P[0], c));
#pragma unroll
    for (int d = 0; d < 6; ++d) kw_add(inc, kw_apply(P[d], kw_shift<DIR>(inc, 1 << d, lane)));
    total = {__shfl(inc.a, 63 - first), __shfl(inc.b, 63 - first), __shfl(inc.c, 63 - first), __shfl(inc.d, 63 - first)};
    z = kw_shift<DIR>(inc, 1, lane);
    if (lane == first) z = c;
}
// the wave's sum, in every lane: a fixed tree
__device__ __forceinline__ double kw_wave_sum(double v) {
#pragma unroll
    for (int d = 1; d < 64; d *= 2) v += __shfl_xor(v, d);
    return v;
}

using kw_f4 = float __attribute__((ext_vector_type(4)));

// KW_E consecutive samples from n of a row, zeros from L on
__device__ __forceinline__ void kw_load(const float* row, int64_t n, int64_t L, bool vec, float (&e)[KW_E]) {
    if (vec && n + KW_E <= L) {
#pragma unroll
        for (int j = 0; j < KW_E / 4; ++j) {
            const kw_f4 q = *reinterpret_cast<const kw_f4*>(row + n + 4 * j);
            e[4 * j] = q.x; e[4 * j + 1] = q.y; e[4 * j + 2] = q.z; e[4 * j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < KW_E; ++i) e[i] = n + i < L ? row[n + i] : 0.0f;
    }
}

struct KwTile {
    bool live;
    int64_t rc, t, n;   // row-channel, tile, this lane's first sample
    int c;
    int64_t r;
};
__device__ __forceinline__ KwTile kw_tile(const KwArgs& a) {
    KwTile w;
    const int64_t item = (int64_t)blockIdx.x * KW_WAVES + (threadIdx.x >> 6);
    w.live = item < a.items;
    const int64_t it = w.live ? item : 0;
    w.rc = it / a.ntiles;
    w.t = it - w.rc * a.ntiles;
    w.r = w.rc / a.C;
    w.c = (int)(w.rc - w.r * a.C);
    w.n = w.t * KW_TILE + KW_E * (threadIdx.x & 63);
    return w;
}
__device__ __forceinline__ S4 kw_ws_load(const double* p) { return {p[0], p[1], p[2], p[3]}; }
__device__ __forceinline__ void kw_ws_store(double* p, const S4& s) {
    p[0] = s.a; p[1] = s.b; p[2] = s.c; p[3] = s.d;
}

// ------------------------------------------------------------------------------------ 1. the tiles' end states from silence
__global__ __launch_bounds__(64 * KW_WAVES) void kw_tile_state_kernel(const float* __restrict__ x, double* __restrict__ ws,
                                                                     KwArgs a, KwConst k) {
    const KwTile w = kw_tile(a);
    if (!w.live) return;   // (a whole wave; the kernel has no barrier)
    const int lane = threadIdx.x & 63;
    float e[KW_E];
    kw_load(x + row_off(a.xmap, w.r, w.c), w.n, a.L, a.xvec, e);
    S4 z = {0.0, 0.0, 0.0, 0.0}, total;
#pragma unroll
    for (int i = 0; i < KW_E; ++i) kw_step(k, z, (double)e[i]);
    kw_scan<1>(k.lane, S4{0.0, 0.0, 0.0, 0.0}, lane, z, total);
    if (lane == 0) kw_ws_store(ws + (w.rc * a.ntiles + w.t) * KW_WS, total);
}

// ------------------------------------------------------------------------------------ 2. end states -> entering states
// ws points at the forward states (rev = 0: tiles from the first up) or at the adjoint states (+ 4; rev = 1: from the last down)
__global__ __launch_bounds__(64) void kw_carry_kernel(double* __restrict__ ws, KwArgs a, KwConst k, int rev) {
    const int lane = threadIdx.x;
    double* row = ws + (int64_t)blockIdx.x * a.ntiles * KW_WS;
    S4 c = {0.0, 0.0, 0.0, 0.0};
    for (int64_t q0 = 0; q0 < a.ntiles; q0 += 64) {
        const int64_t q = q0 + lane;
        const bool live = q < a.ntiles;
        double* p = row + (rev ? a.ntiles - 1 - q : q) * KW_WS;
        S4 z = live ? kw_ws_load(p) : S4{0.0, 0.0, 0.0, 0.0}, total;
        kw_scan<1>(k.tile, c, lane, z, total);
        if (live) kw_ws_store(p, z);
        c = total;
    }
}

// ------------------------------------------------------------------------------------ 3. the tiles from their entering states
// MODE 0: the sums of y^2 per sub-block; 1: the tile's adjoint end state from silence; 2: the adjoint into gx
template <int MODE>
__global__ __launch_bounds__(64 * KW_WAVES) void kw_main_kernel(const float* __restrict__ x, const double* __restrict__ genergy,
                                                               double* __restrict__ energy, float* __restrict__ gx,
                                                               double* __restrict__ ws, KwArgs a, KwConst k) {
    __shared__ double sq[MODE == 0 ? KW_WAVES * KW_TILE : 1];
    const KwTile w = kw_tile(a);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* wst = ws + (w.rc * a.ntiles + w.t) * KW_WS;
    float e[KW_E];
    kw_load(x + row_off(a.xmap, w.r, w.c), w.n, a.L, a.xvec, e);
    S4 z = {0.0, 0.0, 0.0, 0.0}, total;
#pragma unroll
    for (int i = 0; i < KW_E; ++i) kw_step(k, z, (double)e[i]);
    kw_scan<1>(k.lane, kw_ws_load(wst), lane, z, total);
    double y[KW_E];
#pragma unroll
    for (int i = 0; i < KW_E; ++i) y[i] = kw_step(k, z, (double)e[i]);

    if (MODE == 0) {
        const int64_t n0 = w.t * KW_TILE, kb = n0 / a.hop;   // kb: the sub-block of the tile's first sample
        double* part = wst + 4;
        double* out = energy + w.rc * a.n_sub;
        // where the tile's sum of sub-block kk goes: a sub-block inside the tile is finished, of another the tile holds the
        // first part it is asked for (the sub-block of its first sample) or the second (the one that runs on into the next tile)
        auto put = [&](int64_t kk, double s) {
            if (kk >= a.n_sub || !w.live) return;
            if (kk * a.hop >= n0 && (kk + 1) * a.hop <= n0 + KW_TILE)
                out[kk] = s;
            else
                part[kk == kb ? 0 : 1] = s;
        };
        if (a.hop >= KW_TILE) {   // at most two sub-blocks meet the tile
            const int64_t edge = (kb + 1) * a.hop;
            double s0 = 0.0, s1 = 0.0;
#pragma unroll
            for (int i = 0; i < KW_E; ++i) {
                const int64_t n = w.n + i;
                const double v = n < a.Lv ? y[i] * y[i] : 0.0;
                if (n < edge) s0 += v; else s1 += v;
            }
            s0 = kw_wave_sum(s0);
            s1 = kw_wave_sum(s1);
            if (lane == 0) {
                put(kb, s0);
                if (edge < n0 + KW_TILE) put(kb + 1, s1);
            }
        } else {                  // many: the squares through LDS, a lane per sub-block in the order of the samples
            double* mine = sq + wave * KW_TILE;
#pragma unroll
            for (int i = 0; i < KW_E; ++i) mine[KW_E * lane + i] = w.n + i < a.Lv ? y[i] * y[i] : 0.0;
            __syncthreads();
            const int hop = (int)a.hop, rem0 = (int)(n0 - kb * a.hop);
            const int nseg = (rem0 + KW_TILE - 1) / hop + 1;
            for (int j = lane; j < nseg; j += 64) {
                const int lo = j * hop - rem0 < 0 ? 0 : j * hop - rem0;
                const int hi = (j + 1) * hop - rem0 > KW_TILE ? KW_TILE : (j + 1) * hop - rem0;
                double s = 0.0;
                for (int m = lo; m < hi; ++m) s += mine[m];
                put(kb + j, s);
            }
        }
        return;
    }
    if (!w.live) return;   // (a whole wave; modes 1 and 2 have no barrier)

    // v = 2 genergy[n / hop] y, zero from Lv on
    {
        int64_t kk = w.n / a.hop, rem = w.n - kk * a.hop;
        const double* g = genergy + w.rc * a.n_sub;
        double gk = kk < a.n_sub ? g[kk] : 0.0;
#pragma unroll
        for (int i = 0; i < KW_E; ++i) {
            y[i] *= 2.0 * gk;
            if (++rem == a.hop) {
                rem = 0;
                ++kk;
                gk = kk < a.n_sub ? g[kk] : 0.0;
            }
        }
    }
    // the recursion over v from the tile's last sample down
    z = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int i = KW_E - 1; i >= 0; --i) kw_step(k, z, y[i]);
    if (MODE == 1) {
        kw_scan<-1>(k.lane, S4{0.0, 0.0, 0.0, 0.0}, lane, z, total);
        if (lane == 0) kw_ws_store(wst + 4, total);
        return;
    }
    kw_scan<-1>(k.lane, kw_ws_load(wst + 4), lane, z, total);
    float o[KW_E];
#pragma unroll
    for (int i = KW_E - 1; i >= 0; --i) o[i] = (float)kw_step(k, z, y[i]);
    float* dst = gx + row_off(a.gmap, w.r, w.c);
    if (a.gvec && w.n + KW_E <= a.L) {
#pragma unroll
        for (int j = 0; j < KW_E / 4; ++j) {
            kw_f4* p = reinterpret_cast<kw_f4*>(dst + w.n + 4 * j);
            kw_f4 q = {o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]};
            if (a.accumulate) q += *p;
            *p = q;
        }
    } else {
#pragma unroll
        for (int i = 0; i < KW_E; ++i)
            if (w.n + i < a.L) dst[w.n + i] = a.accumulate ? dst[w.n + i] + o[i] : o[i];
    }
}

// ------------------------------------------------------------------------------------ 4. sub-blocks that cross a tile edge
// One wave per row-channel and tile edge t * 1024, t = 1 .. ntiles - 1: the sub-block that holds the sample before the edge
// and the one after it, if this is the first edge it crosses, is the sum of its tiles' parts in the order of the tiles (a
// lane takes every 64th, then the fixed tree).
__global__ __launch_bounds__(64 * KW_WAVES) void kw_energy_finish_kernel(const double* __restrict__ ws,
                                                                        double* __restrict__ energy, KwArgs a) {
    const int64_t item = (int64_t)blockIdx.x * KW_WAVES + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    const int64_t edges = a.ntiles - 1;
    if (item >= a.rcs * edges) return;
    const int64_t rc = item / edges, t = item - rc * edges + 1;
    const int64_t b = t * KW_TILE, kk = b / a.hop;
    if (kk >= a.n_sub || kk * a.hop == b || (kk * a.hop) / KW_TILE != t - 1) return;
    const int64_t t1 = ((kk + 1) * a.hop - 1) / KW_TILE;
    const double* row = ws + rc * a.ntiles * KW_WS;
    double s = 0.0;
    for (int64_t tt = t - 1 + lane; tt <= t1; tt += 64) s += row[tt * KW_WS + 4 + ((tt * KW_TILE) / a.hop == kk ? 0 : 1)];
    s = kw_wave_sum(s);
    if (lane == 0) energy[rc * a.n_sub + kk] = s;
}

// ------------------------------------------------------------------------------------ host
struct KwMatL {
    long double m[4][4];
};
static KwMatL kw_mul(const KwMatL& x, const KwMatL& y) {
    KwMatL r;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            long double s = 0.0L;
            for (int q = 0; q < 4; ++q) s += x.m[i][q] * y.m[q][j];
            r.m[i][j] = s;
        }
    return r;
}
static bool kw_pack(const KwMatL& x, KwMat& o) {
    const double v[12] = {(double)x.m[0][0], (double)x.m[0][1], (double)x.m[1][0], (double)x.m[1][1],
                          (double)x.m[2][0], (double)x.m[2][1], (double)x.m[2][2], (double)x.m[2][3],
                          (double)x.m[3][0], (double)x.m[3][1], (double)x.m[3][2], (double)x.m[3][3]};
    bool finite = true;
    for (int i = 0; i < 12; ++i) {
        o.m[i] = v[i];
        finite = finite && v[i] - v[i] == 0.0;
    }
    return finite;
}
// the constants of a call from its ten coefficients; false for a coefficient, or a power of A, that is not finite
static bool kw_constants(const double* coef, KwConst& k) {
    for (int i = 0; i < 10; ++i)
        if (!(coef[i] - coef[i] == 0.0)) return false;
    k.b10 = coef[0]; k.b11 = coef[1]; k.b12 = coef[2]; k.a11 = coef[3]; k.a12 = coef[4];
    k.b20 = coef[5]; k.b21 = coef[6]; k.b22 = coef[7]; k.a21 = coef[8]; k.a22 = coef[9];
    // kw_step with x = 0
    KwMatL p = {{{-(long double)k.a11, -(long double)k.a12, 0.0L, 0.0L},
                 {1.0L, 0.0L, 0.0L, 0.0L},
                 {(long double)k.b11 - (long double)k.b10 * k.a11, (long double)k.b12 - (long double)k.b10 * k.a12,
                  -(long double)k.a21, -(long double)k.a22},
                 {0.0L, 0.0L, 1.0L, 0.0L}}};
    for (int e = 1; e < KW_E; e *= 2) p = kw_mul(p, p);   // A^16
    bool finite = true;
    for (int d = 0; d < 12; ++d) {                         // A^(16 * 2^d): the lanes' six, then the tiles' six
        finite = kw_pack(p, d < 6 ? k.lane[d] : k.tile[d - 6]) && finite;
        p = kw_mul(p, p);
    }
    return finite;
}
static inline int64_t kw_tiles(int64_t L) { return (L + KW_TILE - 1) / KW_TILE; }
static inline bool kw_aligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) == 0; }
static inline bool kw_map_vec(const void* p, const gfx_rowmap_t& m) {
    return aligned16(p) && map_vec(m);
}

// the checks both entries share, then the constants and the geometry; what the signal's rows need is left to the caller
static int kw_prepare(const float* x, gfx_rowmap_t xmap, const double* coef, int64_t R, int64_t C, int64_t L, int64_t hop,
                      void* ws, size_t ws_bytes, KwArgs& a, KwConst& k) {
    if (!x || !coef || !ws || R <= 0 || C <= 0 || L <= 0 || hop < 1 || hop > L || xmap.inner <= 0) return GFX_EINVAL;
    if (R > 0x7fffffffLL || C > 0x7fffffffLL || !kw_aligned(ws, 16)) return GFX_EINVAL;
    const int64_t ntiles = kw_tiles(L);
    if (R * C > MAX_GRID_X || ntiles > MAX_GRID_X * KW_WAVES / (R * C)) return GFX_EINVAL;   // grid.x of every launch
    if (!kw_constants(coef, k)) return GFX_EINVAL;
    if (ws_bytes < gfx_kweight_energy_ws_bytes(R, C, L)) return GFX_ENOSPC;
    a.xmap = xmap;
    a.gmap = xmap;
    a.L = L; a.hop = hop; a.n_sub = L / hop; a.Lv = a.n_sub * hop;
    a.ntiles = ntiles; a.rcs = R * C; a.items = a.rcs * ntiles;
    a.C = (int)C; a.xvec = kw_map_vec(x, xmap); a.gvec = 0; a.accumulate = 0;
    return GFX_OK;
}
static inline unsigned kw_blocks(int64_t items) { return (unsigned)((items + KW_WAVES - 1) / KW_WAVES); }

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_kweight_energy_ws_bytes(int64_t R, int64_t C, int64_t L) {
    if (R <= 0 || C <= 0 || L <= 0) return 0;
    return (size_t)R * (size_t)C * (size_t)kw_tiles(L) * KW_WS * sizeof(double);
}

int gfx_kweight_energy_f32(const float* x, gfx_rowmap_t xmap, const double* coef, double* energy, int64_t R, int64_t C,
                           int64_t L, int64_t hop, void* ws, size_t ws_bytes, void* stream) {
    KwArgs a;
    KwConst k;
    if (!energy || !kw_aligned(energy, 8)) return GFX_EINVAL;
    const int rc = kw_prepare(x, xmap, coef, R, C, L, hop, ws, ws_bytes, a, k);
    if (rc != GFX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
    double* w = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(kw_tile_state_kernel, dim3(kw_blocks(a.items)), dim3(64 * KW_WAVES), 0, s, x, w, a, k);
    hipLaunchKernelGGL(kw_carry_kernel, dim3((unsigned)a.rcs), dim3(64), 0, s, w, a, k, 0);
    hipLaunchKernelGGL(kw_main_kernel<0>, dim3(kw_blocks(a.items)), dim3(64 * KW_WAVES), 0, s, x,
                       static_cast<const double*>(nullptr), energy, static_cast<float*>(nullptr), w, a, k);
    if (a.ntiles > 1)
        hipLaunchKernelGGL(kw_energy_finish_kernel, dim3(kw_blocks(a.rcs * (a.ntiles - 1))), dim3(64 * KW_WAVES), 0, s, w,
                           energy, a);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_kweight_energy_bwd_f32(const float* x, gfx_rowmap_t xmap, const double* coef, const double* genergy, float* gx,
                               gfx_rowmap_t gmap, int64_t R, int64_t C, int64_t L, int64_t hop, int accumulate, void* ws,
                               size_t ws_bytes, void* stream) {
    KwArgs a;
    KwConst k;
    if (!genergy || !kw_aligned(genergy, 8) || !gx || gmap.inner <= 0) return GFX_EINVAL;
    const int rc = kw_prepare(x, xmap, coef, R, C, L, hop, ws, ws_bytes, a, k);
    if (rc != GFX_OK) return rc;
    a.gmap = gmap;
    a.gvec = kw_map_vec(gx, gmap);
    a.accumulate = accumulate != 0;
    hipStream_t s = (hipStream_t)stream;
    double* w = reinterpret_cast<double*>(ws);
    const dim3 grid(kw_blocks(a.items)), block(64 * KW_WAVES);
    hipLaunchKernelGGL(kw_tile_state_kernel, grid, block, 0, s, x, w, a, k);
    hipLaunchKernelGGL(kw_carry_kernel, dim3((unsigned)a.rcs), dim3(64), 0, s, w, a, k, 0);
    hipLaunchKernelGGL(kw_main_kernel<1>, grid, block, 0, s, x, genergy, static_cast<double*>(nullptr),
                       static_cast<float*>(nullptr), w, a, k);
    hipLaunchKernelGGL(kw_carry_kernel, dim3((unsigned)a.rcs), dim3(64), 0, s, w + 4, a, k, 1);
    hipLaunchKernelGGL(kw_main_kernel<2>, grid, block, 0, s, x, genergy, static_cast<double*>(nullptr), gx, w, a, k);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
