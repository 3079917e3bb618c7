// Shared pieces of the chirp-z transforms (czt.hip: one real row per transform; czt_pair.hpp: two real rows packed
// into one complex transform): precision traits, the geometry, the vocabulary the column and radix-4 passes of both forms
// are written in, and the host launchers of the kernels that both forms run (compiled in czt.hip, once).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "fft_tile.hpp"
#include "fft_tile_f64.hpp"
#include "small_dft.hpp"

namespace gfx {

// the workspace streams through every pass once: non-temporal accesses (__builtin_nontemporal_*, or these aux bits on a
// descriptor access) keep it from evicting what IS reused (the chirp spectrum, the twiddle tables)
constexpr int CZT_NT = 2;

constexpr int CZT_MAXC = 32;
// tiles per (sub-)transform: every size up to 32 with prime factors up to 7 (czt_geom picks the smallest that covers P)
#define GFX_CZT_SIZES(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(12) X(14) X(15) X(16) X(18) X(20) X(21) X(24) \
    X(25) X(27) X(28) X(30) X(32)

// Working precision of the transforms (the data in and out is fp32 either way): float = the packed-FP32 tile, double =
// the `precise` form for the energy envelope (fft_tile_f64.hpp).  Tables, spectra and the workspace are T2 per point.
template <typename T> struct Prec;
template <> struct Prec<float> {
    using cxt = cx;
    using T2 = float2;
    static constexpr int lds_bytes = TILE_LDS_BYTES;
    static __device__ __forceinline__ T2 make(float x, float y) { return make_float2(x, y); }
};
template <> struct Prec<double> {
    using cxt = cxd;
    using T2 = double2;
    static constexpr int lds_bytes = TILE_LDS_BYTES_F64;
    static __device__ __forceinline__ T2 make(double x, double y) { return make_double2(x, y); }
};

struct CztGeom {
    int64_t P, Q, K, NFFT;   // NFFT = S * C * 8192
    int C, S;                // C <= 32 columns per sub-transform; S = 4^levels sub-transforms under `levels` outer radix-4 levels
    int levels;
    // where the real output rows go: row r of the call at y + r * ldy (yC == 0), or -- the entries' ymap -- row
    // (row0 + r) of a (rows / yC, yC, len) signal addressed through a row map (a strided view of the render's buffer)
    int yC;
    int64_t row0;
    gfx_rowmap_t ymap;
    // two rows per transform (czt_pair.hip): bits of max |z| of every row of the launch chain, or null -- the second row
    // of a pair goes through scaled by the power of two that brings it to the first row's binade (pair_scale)
    const uint32_t* rmax;
    int relu;                // the last pass stores max(y, 0) (the envelope smoother's relu, core/envelope.py:48, fused in)
};

__device__ __forceinline__ float* czt_out_row(const CztGeom& g, float* y, int64_t ldy, int64_t row) {
    if (g.yC == 0) return y + row * ldy;
    const int64_t q = g.row0 + row;
    const unsigned r = (unsigned)(q / g.yC);
    const int c = (int)(q - (int64_t)r * g.yC);
    const unsigned inner = (unsigned)g.ymap.inner, o = r / inner, rem = r - o * inner;
    return y + (int64_t)o * g.ymap.stride_outer + (int64_t)rem * g.ymap.stride_inner + (int64_t)c * g.ymap.stride_ch;
}

constexpr int CZT_MAX_LEVELS = 3;   // NFFT <= 2^24: P <= 11,184,811 (233 s of audio at 48 kHz plus the filter)

// the pair form's column passes take up to 63 tiles at once (their kernels of more than 32 are czt_pair.hpp's)
constexpr int CZT_PAIR_MAXC = 63;
#define GFX_CZT_PAIR_SIZES(X) GFX_CZT_SIZES(X) X(35) X(36) X(40) X(42) X(45) X(48) X(49) X(50) X(54) X(56) X(60) X(63)

// the pair's middle pass keeps two columns of C points in registers when fused with the next column pass: above 48 tiles
// (36 in double precision) that no longer fits two waves per SIMD and it goes in two passes instead (one more sweep over the
// buffer): czt_pair_mid_kernel, then this file's forward column pass
template <typename T, int C> constexpr bool pair_mid_fused() { return sizeof(T) == 4 ? C <= 48 : C <= 36; }

// The geometry of a transform of odd length P whose convolutions span `points`: up to `one_pass` tiles in one column
// pass; beyond, outer radix-4 levels around sub-transforms of C <= 32 tiles.  C is rounded up to a count with prime factors
// up to 7 (small_dft.hpp; 32 and 63 = 3 * 3 * 7 are supported: the loop ends at or below them).
static inline bool czt_geom_points(int64_t P, int64_t points, int one_pass, CztGeom& g) {
    g.yC = 0;
    g.row0 = 0;
    g.rmax = nullptr;
    g.relu = 0;
    g.ymap = gfx_rowmap_t{1, 0, 0, 0};
    g.P = P;
    g.Q = P - 1;
    g.K = (P + 1) / 2;
    g.levels = 0;
    int64_t per = (points + TILE_M - 1) / TILE_M;
    if (per > one_pass)
        while (per > CZT_MAXC) {
            per = (per + 3) / 4;
            ++g.levels;
        }
    if (g.levels > CZT_MAX_LEVELS) return false;
    int C = (int)per;
    while (!sd_supported(C) || C == 64) ++C;
    g.S = 1 << (2 * g.levels);
    g.C = C;
    g.NFFT = (int64_t)g.S * C * TILE_M;
    return true;
}
// one row per transform: P inputs and K outputs (or the other way round) under one circular convolution
static inline bool czt_geom(int64_t P, CztGeom& g) {
    return P >= 3 && (P & 1) && czt_geom_points(P, P + (P + 1) / 2 - 1, CZT_MAXC, g);
}
// two rows per transform: the bins on both sides, 2P - 1 points
static inline bool czt_pair_geom(int64_t P, CztGeom& g) {
    return P >= 3 && (P & 1) && czt_geom_points(P, 2 * P - 1, CZT_PAIR_MAXC, g);
}

// where the output goes: the slice [lo, lo + len) of the Q grid, rows ldy apart or (ymap) through a row map
static inline bool czt_output_args(CztGeom& g, const gfx_rowmap_t* ymap, int yC, int64_t row0, int64_t rows, int64_t lo,
                                   int64_t len, int64_t ldy) {
    if (ymap) {
        if (yC < 1 || row0 < 0 || ymap->inner <= 0 || ymap->inner > 0x7fffffffLL || (row0 + rows) / yC > 0x7fffffffLL)
            return false;
        g.yC = yC;
        g.ymap = *ymap;
    }
    return lo >= 0 && len >= 1 && lo + len <= g.Q && ldy >= len;
}

// plan layout (float2 units): cP[P] | cQ[Q] | spectra [NFFT] each of bP, bQ (forward) and of bQ, bP placed for the
// adjoint (same chirps, mirrored support: the adjoint's first transform has Q inputs and K outputs, its second K
// inputs and P outputs)
static inline size_t czt_plan_f2(const CztGeom& g) { return (size_t)(g.P + g.Q + 4 * g.NFFT); }

// Tile accesses through a buffer descriptor: base in SGPRs, one lane offset, the register row as the scalar offset -- a
// global access with a 2048 a byte offset needs a 64-bit VGPR address per row (the immediate field ends at 4095), 64
// registers of addresses per phase.  AUX 2 = non-temporal.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tile_rsrc(const void* base, uint32_t bytes) {
    const uint64_t p = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, bytes, 0x00020000);
}
template <int AUX> __device__ __forceinline__ cx tile_ld(__amdgpu_buffer_rsrc_t r, int t, int row, cx*) {
    return __builtin_bit_cast(cx, __builtin_amdgcn_raw_buffer_load_b64(r, 8u * (uint32_t)t, (uint32_t)(row * 256 * 8), AUX));
}
template <int AUX> __device__ __forceinline__ cxd tile_ld(__amdgpu_buffer_rsrc_t r, int t, int row, cxd*) {
    return __builtin_bit_cast(cxd, __builtin_amdgcn_raw_buffer_load_b128(r, 16u * (uint32_t)t, (uint32_t)(row * 256 * 16), AUX));
}
template <int AUX> __device__ __forceinline__ void tile_st(__amdgpu_buffer_rsrc_t r, int t, int row, cx v) {
    using u2 = unsigned __attribute__((ext_vector_type(2)));
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, 8u * (uint32_t)t, (uint32_t)(row * 256 * 8), AUX);
}
template <int AUX> __device__ __forceinline__ void tile_st(__amdgpu_buffer_rsrc_t r, int t, int row, cxd v) {
    using u4 = unsigned __attribute__((ext_vector_type(4)));
    __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u4, v), r, 16u * (uint32_t)t, (uint32_t)(row * 256 * 16), AUX);
}

// the workspace's points in the column passes (T2 in memory, the tile's complex type in registers)
template <typename T>
__device__ __forceinline__ typename Prec<T>::cxt buf_load(const typename Prec<T>::T2* p) {
    return __builtin_nontemporal_load(reinterpret_cast<const typename Prec<T>::cxt*>(p));
}
template <typename T>
__device__ __forceinline__ void buf_store(typename Prec<T>::T2* p, typename Prec<T>::cxt v) {
    __builtin_nontemporal_store(v, reinterpret_cast<typename Prec<T>::cxt*>(p));
}

// A column pass's view of one transform's points: point (k1, n2) = b[k1 * 8192 + n2].  float: through a descriptor (lane
// offset 8 n2, row k1 as the scalar offset) -- a global access per row costs a 64-bit VGPR address and its carry chain per
// point, in kernels that are bound by vector-memory issue and the vector ALU; double: global accesses (measured equal).
template <typename T> struct ColBuf {
    using cx = typename Prec<T>::cxt;
    typename Prec<T>::T2* b;
    __amdgpu_buffer_rsrc_t r;
    __device__ __forceinline__ ColBuf(const typename Prec<T>::T2* base, int64_t points)
        : b(const_cast<typename Prec<T>::T2*>(base)), r(tile_rsrc(base, (uint32_t)(points * (int64_t)sizeof(typename Prec<T>::T2)))) {}
    __device__ __forceinline__ cx ld(int k1, int n2) const {
        if constexpr (sizeof(T) == 4)
            return __builtin_bit_cast(cx, __builtin_amdgcn_raw_buffer_load_b64(r, 8u * (uint32_t)n2, (uint32_t)k1 * (TILE_M * 8u), CZT_NT));
        else
            return buf_load<T>(&b[(int64_t)k1 * TILE_M + n2]);
    }
    __device__ __forceinline__ void st(int k1, int n2, cx v) const {
        if constexpr (sizeof(T) == 4) {
            using u2 = unsigned __attribute__((ext_vector_type(2)));
            __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u2, v), r, 8u * (uint32_t)n2, (uint32_t)k1 * (TILE_M * 8u), CZT_NT);
        } else {
            buf_store<T>(&b[(int64_t)k1 * TILE_M + n2], v);
        }
    }
};

// b[j] = exp(sign i pi j^2 / den) at circular index j mod NFFT for j in [-lo, hi], zero elsewhere
struct ChirpSeq {
    int64_t lo, hi, den;
    double sign;
};

template <typename T>
__device__ __forceinline__ typename Prec<T>::T2 chirp_d(int64_t j, int64_t den, double sign) {   // exp(sign i pi j^2 / den)
    const int64_t r = (j * j) % (2 * den);
    double s, c;
    sincospi((double)r / (double)den, &s, &c);
    return Prec<T>::make((T)c, (T)(sign * s));
}

// e^{-+ 2 pi i r / N} for 0 <= r < N, N a multiple of 4 (N = C x 8192, not a power of two in general): the quarter turn is
// taken off in integers and the rest, rem / (N / 2) <= 1/2 half-turns with rem < 2^24 exact, goes to sincospif -- the phase
// is good to 1e-7 rad whatever N (for a power of two the quotient is exact, as before).
__device__ __forceinline__ cx unit_root_f(int r, int N, bool conj) {
    const int quarter = N >> 2;
    const int q = r / quarter, rem = r - q * quarter;
    float s, c;
    sincospif((float)rem / (float)(N >> 1), &s, &c);
    const float cr = (q & 1) ? ((q & 2) ? s : -s) : ((q & 2) ? -c : c);     // cos of the full angle
    const float sr = (q & 1) ? ((q & 2) ? -c : c) : ((q & 2) ? -s : s);     // sin of the full angle
    return cx{cr, conj ? sr : -sr};
}
__device__ __forceinline__ cxd col_twiddle(int n2, int k1, double inv_half_nfft, bool conj) {
    double s, c;
    sincospi((double)(n2 * k1) * inv_half_nfft, &s, &c);
    return cxd{c, conj ? s : -s};
}

// The column twiddles W_NS^(n2 k1), k1 = 1 .. C-1 (asked for in turn, k1 a constant after unrolling).  float: two digits,
// k1 = 8 a + b -- W^(n2 b) for b < 8 and W^(8 n2 a), each one sincospif on an exactly reduced phase, and one complex product
// for the rest: 11 evaluations instead of 34 at 35 tiles (one per point made the float column passes instruction-bound:
// ~50 of ~80 instructions per point; one more rounding, 6e-8).  double: powers of W^(n2) by repeated multiplication (31 steps
// lose ~1e-15, and a double sincospi per point would make the column kernels compute-bound).
template <typename T, int C> struct ColTw;
template <int C> struct ColTw<float, C> {
    static constexpr int NLO = C < 8 ? C : 8, NHI = (C - 1) / 8 + 1;
    cx lo[NLO], hi[NHI];
    __device__ __forceinline__ ColTw(int n2, int NS, bool conj) {
        lo[0] = hi[0] = cx{1.0f, 0.0f};
        int r = 0;
#pragma unroll
        for (int b = 1; b < NLO; ++b) {
            r += n2;                                       // n2 b < 8 x 8192 <= NS whenever C >= 8; below, b < C keeps it under NS
            lo[b] = unit_root_f(r, NS, conj);
        }
        r = 0;
#pragma unroll
        for (int a = 1; a < NHI; ++a) {
            r += 8 * n2;                                   // (8 n2 < 65536 <= NS here: one subtraction reduces)
            r -= r >= NS ? NS : 0;
            hi[a] = unit_root_f(r, NS, conj);
        }
    }
    __device__ __forceinline__ cx at(int k1) const {
        const int a = k1 >> 3, b = k1 & 7;
        return a == 0 ? lo[b] : b == 0 ? hi[a] : cmul(hi[a], lo[b]);
    }
};
template <int C> struct ColTw<double, C> {
    cxd w1, w;
    __device__ __forceinline__ ColTw(int n2, int NS, bool conj) : w1(col_twiddle(n2, 1, 2.0 / (double)NS, conj)), w(cxd{1.0, 0.0}) {}
    __device__ __forceinline__ cxd at(int) { w = cmul(w, w1); return w; }
};

// C-point DFT of a column in registers: the power-of-two sizes on the tile's radix-2 codelet (bit-identical with the
// rounds before), the others on small_dft.hpp; either way frequency k ends up at v[spos(C, k)].
template <int C, bool INV, typename V>
__device__ __forceinline__ void col_dft(V (&v)[C]) {
    if constexpr ((C & (C - 1)) == 0) dif<C, INV>(v);
    else sdft<C, INV>(v);
}

// ---- the passes' vocabulary, one point at a time (the loops stay in the kernels: as functions of the register array the
// same passes compile to other schedules, EXPERIMENTS.md "Chirp-z transforms: every kernel compiled once") ---------------
// A column pass's two ends for point k1 of the thread's column n2 (rows row0 + k1 of cb): in, the point times the
// conjugate twiddle (tw built with conj) -- what col_dft<C, true> inverts; out, what col_dft<C, false> left at
// v[spos(C, k1)] times the forward twiddle.  Call for k1 = 0 .. C-1 in turn: ColTw<double> counts on it.
template <typename T, int C>
__device__ __forceinline__ typename Prec<T>::cxt col_in(const ColBuf<T>& cb, ColTw<T, C>& tw, int k1, int n2, int row0 = 0) {
    const typename Prec<T>::cxt e = cb.ld(row0 + k1, n2);
    return k1 == 0 ? e : cmul(e, tw.at(k1));
}
template <typename T, int C>
__device__ __forceinline__ void col_out(const ColBuf<T>& cb, ColTw<T, C>& tw, int k1, int n2, typename Prec<T>::cxt e, int row0 = 0) {
    const typename Prec<T>::cxt o = k1 == 0 ? e : cmul(e, tw.at(k1));
    cb.st(row0 + k1, n2, o);
}
// the one-row form between its convolutions: bin i < K times cP[i] w_i cQ[i], zero beyond
template <typename T>
__device__ __forceinline__ typename Prec<T>::cxt bin_factor(typename Prec<T>::cxt e, int64_t i, const CztGeom& g,
                                                            const typename Prec<T>::T2* cP,
                                                            const typename Prec<T>::T2* cQ, T sc = (T)1) {
    typename Prec<T>::cxt o = {0, 0};
    if (i < g.K) {
        const T wk = (i == 0 || i == g.K - 1) ? (T)1 : (T)2;
        o = cmul(cmul(e * sc, to_cx(cP[i])), to_cx(cQ[i])) * wk;
    }
    return o;
}
// the one-row form's last step: y[row, i - lo] <- Re(e cQ[i]) / Q for lo <= i < lo + len
template <typename T>
__device__ __forceinline__ void real_out(typename Prec<T>::cxt e, int64_t i, const CztGeom& g,
                                         const typename Prec<T>::T2* cQ, float* y, int64_t ldy,
                                         int64_t lo, int64_t len, int64_t row) {
    if (i >= lo && i < lo + len) {
        const typename Prec<T>::cxt c = to_cx(cQ[i]);
        czt_out_row(g, y, ldy, row)[i - lo] = (float)((e.x * c.x - e.y * c.y) / (T)g.Q);
    }
}

// ---- outer radix-4 levels (NFFT = 4 NS, n = n3 NS + n', k = k3 + 4 k'): the twiddle W_NFFT^(n' k3) --------------------
template <typename T>
__device__ __forceinline__ typename Prec<T>::cxt outer_twiddle(int64_t np, int k3, int64_t NFFT, bool conj) {
    // W_NFFT^(np k3), np k3 < NFFT <= 2^24
    if constexpr (sizeof(T) == 4) {
        return unit_root_f((int)(np * k3), (int)NFFT, conj);
    } else {
        double s, c;
        sincospi(2.0 * (double)(np * k3) / (double)NFFT, &s, &c);
        return cxd{c, conj ? s : -s};
    }
}

// a radix-4 pass's two ends for the thread's point np + k3 NS of the buffer b, as col_in / col_out (out: the result for k3
// is what dif<4, false> left at v[brev(k3, 2)])
template <typename T>
__device__ __forceinline__ typename Prec<T>::cxt r4_in(const typename Prec<T>::T2* b, int64_t NS, int64_t np, int64_t NFFT, int k3) {
    const typename Prec<T>::cxt e = buf_load<T>(&b[k3 * NS + np]);
    return k3 == 0 ? e : cmul(e, outer_twiddle<T>(np, k3, NFFT, true));
}
template <typename T>
__device__ __forceinline__ void r4_out(typename Prec<T>::T2* b, int64_t NS, int64_t np, int64_t NFFT, int k3, typename Prec<T>::cxt e) {
    const typename Prec<T>::cxt o = k3 == 0 ? e : cmul(e, outer_twiddle<T>(np, k3, NFFT, false));
    buf_store<T>(&b[k3 * NS + np], o);
}
// ---- the kernels both forms run, compiled once: their host launchers (czt.hip), per working precision ------------------
// the passes below the outermost level of a transform, in place on `rows` buffers of g.NFFT points: inner radix-4 levels
// and the column pass (forward; with no levels just that column pass, of up to 63 tiles where the pair form takes its
// middle step in two passes), the inverse column pass and the inner levels (inverse, scaled by 4^(levels-1) / NFFT: the
// outermost level's 1/4 is the caller's)
void czt_levels_fwd(const CztGeom& g, float2* buf, int64_t rows, hipStream_t st);
void czt_levels_fwd(const CztGeom& g, double2* buf, int64_t rows, hipStream_t st);
void czt_levels_inv(const CztGeom& g, float2* buf, int64_t rows, hipStream_t st);
void czt_levels_inv(const CztGeom& g, double2* buf, int64_t rows, hipStream_t st);
// the tile pass: its twiddle table (null: not to be had) with the LDS it needs allowed -- `plan`: for czt_chirp_spectrum
const float2* czt_tile_setup(bool plan, hipStream_t st, const float2*);
const double2* czt_tile_setup(bool plan, hipStream_t st, const double2*);
// `tiles` tiles of buf, ctot per transform: forward, times spec, inverse
void czt_tile_pass(float2* buf, const float2* spec, int64_t tiles, int ctot, const float2* tw, hipStream_t st);
void czt_tile_pass(double2* buf, const double2* spec, int64_t tiles, int ctot, const double2* tw, hipStream_t st);
// cP[i] = e^{-i pi i^2 / P}, i < P, and cQ[i] = e^{+i pi i^2 / Q}, i < Q = P - 1
void czt_chirp_tables(float2* cP, float2* cQ, int64_t P, hipStream_t st);
void czt_chirp_tables(double2* cP, double2* cQ, int64_t P, hipStream_t st);
// a chirp sequence's spectrum in the tile pass's layout (buf: g.NFFT points of scratch), with or without outer levels
void czt_chirp_spectrum(const CztGeom& g, ChirpSeq cs, float2* buf, float2* spec, const float2* tw, hipStream_t st);
void czt_chirp_spectrum(const CztGeom& g, ChirpSeq cs, double2* buf, double2* spec, const double2* tw, hipStream_t st);

}  // namespace gfx
