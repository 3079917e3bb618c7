// What every kernel file may need and no operation owns: the offset of a mapped row, the wave-wide sum, the floor of a
// division, and on the host the dynamic-LDS opt-in and the checks on mapped signals (negative strides, shared elements).
// A new kernel file starts from this header; it includes no other operation's header to reach one of these.
// Device code is __forceinline__, host code static inline, the rest constexpr; the one kernel every streaming operation
// shares (the history tail) is defined in common.hip and declared here by its launcher.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/grafx_amd.h"

namespace gfx {

constexpr int64_t MAX_GRID_X = 0x7fffffffLL;     // workgroups of a one-dimensional launch

// rows and row counts fit 32 bits (checked by the launchers): 32-bit division is ~5x cheaper than
// the 64-bit software divide and stays on the scalar unit.
__device__ __forceinline__ int64_t row_off(const gfx_rowmap_t& m, int64_t r, int c) {
    const unsigned inner = (unsigned)m.inner, rr = (unsigned)r;
    const unsigned q = rr / inner, rem = rr - q * inner;
    return (int64_t)q * m.stride_outer + (int64_t)rem * m.stride_inner + (int64_t)c * m.stride_ch;
}

// the same with the 64-bit divide, for the kernels that were written and measured with it
__device__ __forceinline__ int64_t row_off64(const gfx_rowmap_t& m, int64_t r, int c) {
    const int64_t q = r / m.inner, rem = r - q * m.inner;
    return q * m.stride_outer + rem * m.stride_inner + (int64_t)c * m.stride_ch;
}

// the sum over the 64 lanes of a wave, in lane 0
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// floor(e / F), also below zero
__device__ __forceinline__ int64_t floor_div(int64_t e, int F) {
    int64_t q = e / F;
    if (q * F > e) --q;
    return q;
}

// ---- host side ---------------------------------------------------------------------------------------------------
// Let `kernel` be launched with `bytes` of dynamic LDS.  A launch needs the opt-in only above 48 KiB, so below that no call
// is made.  What the call costs has not been measured: it is host-only and lies outside every timed region of bench.py.
template <typename K>
static inline int allow_lds(K kernel, size_t bytes) {
    if (bytes <= 48 * 1024) return GFX_OK;
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)bytes) == hipSuccess
               ? GFX_OK
               : GFX_ELAUNCH;
}

// rows that whole 16-byte accesses may address: the base 16-byte aligned, every stride a multiple of four floats
static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
static inline bool map_vec(const gfx_rowmap_t& m) {
    return m.stride_outer % 4 == 0 && m.stride_inner % 4 == 0 && m.stride_ch % 4 == 0;
}

static inline bool map_negative(const gfx_rowmap_t& m) { return m.stride_outer < 0 || m.stride_inner < 0 || m.stride_ch < 0; }

// do [a, a + na) and [b, b + nb) share an element?
static inline bool ranges_meet(const float* a, int64_t na, const float* b, int64_t nb) { return a < b + nb && b < a + na; }

// [lo, hi) in floats that a mapped (R, C, L) signal covers (strides >= 0)
static inline void map_span(const float* p, const gfx_rowmap_t& m, int64_t R, int64_t C, int64_t L, const float*& lo,
                            const float*& hi) {
    const int64_t nin = R < m.inner ? R : m.inner;
    lo = p;
    hi = p + ((R - 1) / m.inner) * m.stride_outer + (nin - 1) * m.stride_inner + (C - 1) * m.stride_ch + L;
}

// Is `delta` a sum of d_i * stride_i with |d_i| < n_i over the dimensions from i on (strides sorted, largest first)?
static inline bool map_reachable(int64_t delta, const int64_t (*dims)[2], int nd, int i) {
    if (i == nd) return delta == 0;
    const int64_t st = dims[i][0], n = dims[i][1], qd = delta / st;
    for (int64_t c = qd; c <= qd + 1; ++c) {
        if (c >= n) continue;
        const int64_t rest = delta - c * st;
        if (map_reachable(rest < 0 ? -rest : rest, dims, nd, i + 1)) return true;
    }
    return false;
}

// Do two mapped signals share an element?  Exact for two views with the same positive strides (two node ranges of one
// render buffer interleave in memory without touching), the covered ranges otherwise.
static inline bool signals_overlap(const float* a, const gfx_rowmap_t& am, const float* b, const gfx_rowmap_t& bm, int64_t R,
                                   int64_t C, int64_t L) {
    const float *alo, *ahi, *blo, *bhi;
    map_span(a, am, R, C, L, alo, ahi);
    map_span(b, bm, R, C, L, blo, bhi);
    if (!(alo < bhi && blo < ahi)) return false;
    const int64_t nin = R < am.inner ? R : am.inner, nout = (R + am.inner - 1) / am.inner;
    const bool same = am.inner == bm.inner && am.stride_outer == bm.stride_outer && am.stride_inner == bm.stride_inner &&
                      am.stride_ch == bm.stride_ch && (nout == 1 || am.stride_outer > 0) &&
                      (nin == 1 || am.stride_inner > 0) && (C == 1 || am.stride_ch > 0) && R % am.inner == 0;
    if (!same) return true;
    int64_t dims[4][2] = {{am.stride_outer, nout}, {am.stride_inner, nin}, {am.stride_ch, C}, {1, L}};
    int nd = 0;
    for (int i = 0; i < 4; ++i)
        if (dims[i][1] > 1) { dims[nd][0] = dims[i][0]; dims[nd][1] = dims[i][1]; ++nd; }
    for (int i = 1; i < nd; ++i)                       // insertion sort, largest stride first
        for (int j = i; j > 0 && dims[j][0] > dims[j - 1][0]; --j) {
            const int64_t s0 = dims[j][0], s1 = dims[j][1];
            dims[j][0] = dims[j - 1][0]; dims[j][1] = dims[j - 1][1];
            dims[j - 1][0] = s0; dims[j - 1][1] = s1;
        }
    const int64_t delta = a > b ? a - b : b - a;
    return map_reachable(delta, dims, nd, 0);
}

// ---- the history a streamed block leaves behind (common.hip: history_tail_kernel) ------------------------------------------
// zf (R, C, S) = the last S samples of zi || x per row-channel, zi (R, C, S) nullable (zeros): zf[i] = k >= 0 ? x[k] :
// zi[S + k] with k = L - S + i.  A copy, so bit-exact; for L < S the old history shifts down by L.  pos_in / pos_out
// (nullable, one per row): pos_out[r] = (pos_in ? pos_in[r] : 0) + L, the row's running sample count.  One launch, of one
// workgroup per HISTORY_CHUNK state samples; GFX_EINVAL when that grid does not fit (an entry that must refuse before
// its first launch tests history_tail_blocks itself).
constexpr int64_t HISTORY_CHUNK = 1024;
static inline int64_t history_tail_blocks(int64_t R, int64_t C, int64_t S) {
    return R * C * ((S + HISTORY_CHUNK - 1) / HISTORY_CHUNK);
}
int launch_history_tail(const float* x, gfx_rowmap_t xmap, const float* zi, float* zf, int64_t R, int64_t C, int64_t L,
                        int64_t S, const int64_t* pos_in, int64_t* pos_out, hipStream_t stream);

}  // namespace gfx
