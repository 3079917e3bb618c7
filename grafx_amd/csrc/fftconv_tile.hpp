// What the FFT-tile convolution's translation units share: the tile geometry and the argument blocks of the kernels (plain
// structs and a host function, usable from host-only code), the raw-buffer loads and stores of a tile's window, the
// per-row maximum, and the NAT indexing of a transformed tile.  Included by fftconv.hip (the convolution and its filter
// gradient), fir_spectrum.hip (the filter spectra) and fftconv_pipe.hip (the launchers of the hand-scheduled kernels); it
// defines no kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "fft_tile.hpp"

namespace gfx {

struct ConvGeom {
    int64_t nparts, part_len, O, V, ntiles, hop;
    bool ok;
};

// part_len = 0: the default geometry (one tile-sized filter up to 8193 taps, else 8192-tap partitions with windows
// hopping by 8192).  A longer partition (8192 < part_len <= 16384 - Lout, even) is legal when one output tile covers
// all Lout samples: the windows of the partitions then hop by part_len while the tile keeps 16384 - part_len valid
// samples -- fewer partitions and windows for "long filter, short output" problems (the filter gradient).
static inline ConvGeom conv_geom(int64_t N, int64_t Lout, int64_t part_len = 0) {
    ConvGeom g;
    g.ok = true;
    if (N <= TILE_M + 1) {
        g.nparts = 1;
        g.part_len = N;
        // overlap >= N-1, rounded up to whole 512-sample register rows: loads and stores of a tile then need no per-lane
        // masks (load_window / store_valid), ~15 % fewer vector-ALU instructions per tile for <1 % more tiles
        g.O = (N - 1 + 511) & ~int64_t(511);
        g.ok = part_len == 0;
    } else if (part_len == 0 || part_len == TILE_M) {
        g.part_len = TILE_M;
        g.nparts = (N + TILE_M - 1) / TILE_M;
        g.O = TILE_M;
    } else {
        g.ok = part_len > TILE_M && (part_len & 1) == 0 && part_len + Lout <= TILE_F;
        g.part_len = part_len;
        g.nparts = (N + part_len - 1) / part_len;
        g.O = part_len;
    }
    g.V = TILE_F - g.O;
    g.hop = g.nparts == 1 ? g.V : g.part_len;
    g.ntiles = (Lout + g.V - 1) / g.V;
    if (g.hop != g.V && g.ntiles != 1) g.ok = false;
    return g;
}

struct ConvArgs {
    gfx_rowmap_t xmap, ymap, cmap;  // cmap: rows of the optional input copy (fftconv1 only)
    int64_t L, Lout, off;    // signal length, outputs per row, output offset into the full convolution
    int64_t O, V, hop;       // overlap and valid samples per tile; start-to-start distance of the partition windows
    int64_t ntiles, nblocks; // tiles per row-channel, total workgroups of real work
    int nparts;
    int Cin, Cf, Cout;
    unsigned hrows;          // filter rows: row r convolves with filter r % hrows (batch-major rows sharing filters)
};

// workgroup b runs on XCD b % 8 (observed): give each XCD a contiguous run of logical
// indices so tiles of one row-channel (which share the filter spectrum) meet in one L2.
__device__ __forceinline__ unsigned xcd_logical_block() {
    const unsigned per_xcd = gridDim.x >> 3;
    return (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
}

// ---- raw buffer access (SRSRC descriptor in SGPRs + one 32-bit lane offset) --------------------------
// All per-tile traffic goes through buffer instructions: the row base and the per-`a` strides live in
// SGPRs, every lane carries ONE 32-bit byte offset, and the hardware range check supplies the zeros
// outside [0, L) / drops the stores past the row end — no 64-bit per-lane addresses, no bounds code.
using rsrc_t = __amdgpu_buffer_rsrc_t;

__device__ __forceinline__ rsrc_t make_rsrc(const void* base, int64_t bytes) {
    // descriptor inputs must be provably wave-uniform (else hipcc wraps every access in a waterfall loop)
    const uint64_t p = reinterpret_cast<uint64_t>(base);
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p), hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    const int64_t nb = bytes < 0 ? 0 : (bytes > 0x7fffffffLL ? 0x7fffffffLL : bytes);
    const uint32_t n = __builtin_amdgcn_readfirstlane((uint32_t)nb);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), 0, n, 0x00020000);
}
__device__ __forceinline__ cx buf_load_f2(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(cx, __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, 0));
}
__device__ __forceinline__ f4v buf_load_f4(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(f4v, __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, 0));
}
// outputs are streamed: written once, read by a later stage long after they left the 4 MB L2s.  The
// non-temporal hint keeps them from evicting the window overlaps and filter spectra the tiles re-read
// (tee kernel at 8192 rows: 7.3 -> 6.5 ms).
constexpr int STORE_AUX_NT = 2;   // the buffer store's aux bits: non-temporal
__device__ __forceinline__ void buf_store_f2(rsrc_t r, uint32_t voff, uint32_t soff, cx e) {
    using u32x2 = __attribute__((ext_vector_type(2))) unsigned;
    __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(u32x2, e), r, voff, soff, STORE_AUX_NT);
}
constexpr uint32_t OOB = 0xffffffffu;  // lane offset that the range check always rejects

// v[a] = (x[s + 2m], x[s + 2m + 1]), m = t + 256 a; x is zero outside [0, L).  `row` = start of the signal row.
// Straight-line in the common case: the two special cases (a window starting before the row, a pair straddling
// sample 0) sit behind one wave-uniform branch after all 32 loads have been issued.
template <bool FAST = true>
__device__ __forceinline__ void load_window(cx (&v)[32], const float* __restrict__ row, int64_t s, int64_t L,
                                            int t, float gain) {
    // descriptor starts at the window (possibly before the row for the first tile: those lanes are masked)
    const rsrc_t r = make_rsrc(row + s, (L - s) * 4);
    if (FAST && (s >= 0 || (s & 511) == 0)) {
        // No per-lane clipping (uniform test): the window starts inside the row, or a whole number of 512-sample register
        // rows before it (tile geometry with O a multiple of 512) -- every load is "lane offset 8 t" or skipped as a
        // row, and the range check supplies the zeros past the row end.  Saves ~100 compare / select instructions
        // per window on the vector ALU, which is what bounds these kernels.
        const int a_lo = s < 0 ? (int)((-s) >> 9) : 0;
#pragma unroll
        for (int a = 0; a < 32; ++a) {
            if (a < a_lo) v[a] = cx{0.0f, 0.0f};
            else v[a] = buf_load_f2(r, 8u * (uint32_t)t, 2048u * a);
        }
        if (gain != 1.0f) {
#pragma unroll
            for (int a = 0; a < 32; ++a) v[a] *= gain;
        }
        return;
    }
    const bool clip = s < 0;                                   // uniform; only a first tile can start before the row
    const int s32 = clip ? (int)s : 0;                         // |s| <= 16384 there
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int n = s32 + 2 * (t + 256 * a);                 // sample index of the pair's first element (if clip)
        const uint32_t voff = (clip && n < 0) ? OOB : 8u * (uint32_t)t;
        v[a] = buf_load_f2(r, voff, 2048u * a);
    }
    if (clip && (s32 & 1)) {                                   // odd start: the pair (x[-1], x[0]) was masked as a whole
        const float x0 = row[0];
#pragma unroll
        for (int a = 0; a < 32; ++a)
            if (s32 + 2 * (t + 256 * a) == -1) v[a] = cx{0.0f, x0};
    }
    if (gain != 1.0f) {
#pragma unroll
        for (int a = 0; a < 32; ++a) v[a] *= gain;
    }
}

// The window of a streamed block (gfx_fftconv_state_f32): load_window, with the N - 1 samples before the row taken from the
// row's carried history -- v holds hist[n + N - 1] for sample indices -(N-1) <= n < 0 and zero below that.  The windows of
// the tile geometry start a whole number of 512-sample register rows before (or after) sample 0, so a register row lies
// wholly in the history or wholly in the signal: one uniform test per row, the signal rows exactly as load_window's fast
// form reads them.  History rows are read as single dwords with a mask per dword: N - 1 may be odd, so a history pair is
// only 4-byte aligned (8-byte loads would be misaligned on every other row-channel), and when N is even the pair
// (n, n + 1) = (-N, -(N-1)) straddles the start of the history -- its first half is zero, its second hist[0].  No pair
// reaches past the end of the history: n is even and below 0, so n + 1 <= -1.
__device__ __forceinline__ float buf_load_f1(rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0));
}
__device__ __forceinline__ void load_window_hist(cx (&v)[32], const float* __restrict__ row, const float* __restrict__ hist,
                                                 int64_t s, int64_t L, int64_t N, int t) {
    const rsrc_t r = make_rsrc(row + s, (L - s) * 4);
    const rsrc_t hr = make_rsrc(hist, (N - 1) * 4);
    const int a_lo = s < 0 ? (int)((-s) >> 9) : 0;             // register rows before sample 0 (uniform)
    const int h0 = (int)(s + N - 1) + 2 * t;                   // history index of this lane's pair in register row 0
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        if (a < a_lo) {
            const int h = h0 + 512 * a;                        // -16384 < h: a negative index never wraps into the range
            const uint32_t lo = h >= 0 ? 4u * (uint32_t)h : OOB, hi = h >= -1 ? 4u * (uint32_t)(h + 1) : OOB;
            v[a] = cx{buf_load_f1(hr, lo, 0), buf_load_f1(hr, hi, 0)};
        } else {
            v[a] = buf_load_f2(r, 8u * (uint32_t)t, 2048u * a);
        }
    }
}

// Time-reversed window of a segment of `len` (<= 16384) samples: v[a] = (seg[len-1-2m], seg[len-2-2m]), m = t + 256 a,
// zero below the segment.  Lets the filter-gradient correlation use the signal as its own "filter" without a flipped
// copy of it.
__device__ __forceinline__ void load_window_rev(cx (&v)[32], const float* __restrict__ seg, int64_t len, int t) {
    const rsrc_t r = make_rsrc(seg, len * 4);
    const int base = (int)len - 2;
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int e = base - 2 * (t + 256 * a);                // index of the pair's lower sample
        v[a] = cswap(buf_load_f2(r, e < 0 ? OOB : 4u * (uint32_t)e, 0));
    }
    if (len & 1) {                                             // uniform: the pair (seg[-1], seg[0]) was masked as a whole
        const float x0 = seg[0];
#pragma unroll
        for (int a = 0; a < 32; ++a)
            if (base - 2 * (t + 256 * a) == -1) v[a] = cx{x0, 0.0f};
    }
}

// y[n0 + (2m - O)] for 2m >= O, n < Lout;  v[brev5(a)] = (z'[2m], z'[2m+1])  (NATURAL: v[a] instead)
template <bool NATURAL = false>
__device__ __forceinline__ void store_valid(const cx (&v)[32], float* __restrict__ row, int64_t n0, int64_t O,
                                            int64_t Lout, int t) {
    // opaque copy of the lane index: the tee store (before the transforms) and the output store (after them) use
    // the same 32 lane masks, and without this the compiler keeps them alive across the whole kernel (16 spilled
    // dwords = 2.8 GB of scratch write-back per 8192-row launch) instead of recomputing 32 compares
    asm volatile("" : "+v"(t));
    const int64_t room = Lout - (n0 - O);                      // samples from the descriptor base to the row end
    const rsrc_t r = make_rsrc(row + (n0 - O), room * 4);
    if ((O & 511) == 0 && !((room & 1) && room < TILE_F)) {
        // Row-uniform form (uniform test): the overlap is a whole number of 512-sample register rows and no sample pair
        // straddles the row end, so a row is either skipped or stored with "lane offset 8 t" (pairs past the row end
        // are dropped by the range check): no per-lane masks.
        const int a_lo = (int)(O >> 9);
#pragma unroll
        for (int a = 0; a < 32; ++a)
            if (a >= a_lo) buf_store_f2(r, 8u * (uint32_t)t, 2048u * a, v[NATURAL ? a : brev(a, 5)]);
        return;
    }
    const int o32 = (int)O;
    const int tail = (room & 1) && room < TILE_F ? (int)room - 1 : -1;  // a pair straddling the row end starts here
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int q = 2 * (t + 256 * a);
        const uint32_t voff = (q < o32 || q == tail) ? OOB : 8u * (uint32_t)t;
        buf_store_f2(r, voff, 2048u * a, v[NATURAL ? a : brev(a, 5)]);
    }
    if (tail >= o32) {                                         // uniform: single trailing sample of an odd-length row
        float last = 0.0f;
        bool mine = false;
#pragma unroll
        for (int a = 0; a < 32; ++a)
            if (2 * (t + 256 * a) == tail) {
                last = v[NATURAL ? a : brev(a, 5)].x;
                mine = true;
            }
        if (mine) row[n0 - O + tail] = last;
    }
}

// max |y| over what store_valid has just stored of this tile (positions O <= q < room of the tile), into rowmax[rco]: the
// by-product for the odd-length aliasing's pair scaling (round 6; gfx_fftconv_f32's rowmax).  Non-negative floats order like
// their bit patterns: a wave reduction and one atomic maximum per wave and tile.
__device__ __forceinline__ void tile_rowmax(const cx (&v)[32], uint32_t* __restrict__ rowmax, unsigned rco, int64_t n0, int64_t O,
                                            int64_t Lout, int t) {
    const int64_t room = Lout - (n0 - O);
    uint32_t m = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        const int64_t q = 2 * (t + 256 * k);
        const cx e = v[brev(k, 5)];
        const uint32_t ex = __float_as_uint(e.x) & 0x7fffffffu, ey = __float_as_uint(e.y) & 0x7fffffffu;
        if (q >= O && q < room) m = ex > m ? ex : m;
        if (q >= O && q + 1 < room) m = ey > m ? ey : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t u = (uint32_t)__shfl_xor((int)m, o);
        m = u > m ? u : m;
    }
    if ((t & 63) == 0 && m) atomicMax(rowmax + rco, m);
}

#define NAT(arr, i) arr[(i) >> 4][brev((i) & 15, 4)]

// the argument block of the filter-gradient kernels (fftconv.hip: corr1_kernel; fftconv_pipe.hip: its hand-scheduled form)
struct CorrArgs {
    gfx_rowmap_t xmap, gmap;
    int64_t L, Lg, off, N, V, ntiles, nblocks;
    int Cx, Cg, Cout;
};

// grids are whole multiples of 8 workgroups, one share per XCD (xcd_logical_block)
static inline unsigned pad8(int64_t n) { return (unsigned)(((n + 7) / 8) * 8); }

}  // namespace gfx
