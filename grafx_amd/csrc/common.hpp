// What every kernel file may need and no operation owns.  On the device: the offset of a mapped row, the wave-wide sum, the
// floor of a division, the workgroup's fixed-order sums of K doubles (block_sums) and the kernel that adds a row's tile
// sums (tile_sums_finish_kernel).  On the host: launch() -- the dynamic-LDS opt-in, the launch and its check in one --, the
// checks on mapped signals (negative strides, shared elements), on a gradient output (grad_out_ok), on a workspace
// (workspace_ok) and on a pair of state buffers (history_pair_ok), and finish_tile_sums.
// A new kernel file, a new effect above all, starts from these helpers: it launches through launch(), tests its arguments
// with the *_ok functions and sums its parameter gradients through block_sums and finish_tile_sums; it includes no other
// operation's header to reach one of these.
// Device code is __forceinline__, host code static inline, the rest constexpr; the one kernel every streaming operation
// shares (the history tail) is defined in common.hip and declared here by its launcher, the one kernel template (the
// finish) is instantiated by the file that owns its slot map.
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

// The workgroup's sum of each of K doubles, in a fixed order: the wave sums, lane 0 of every wave to red[wave][k], one
// barrier, then thread k adds the WAVES waves in ascending order and hands sum k to f(sum) -- f runs in threads 0 .. K - 1
// only.  Every thread of the workgroup calls it, with its lane and wave as the kernel computed them at its head.  s is
// clobbered: on return s[k] holds the wave's sum in lane 0 and partial sums in the other lanes.  red may be written again
// only behind a barrier of the caller's.  (The callback and the two arguments keep the machine code of the
// kernels that use it: with the sum returned to an `if (t < K)` of the caller's, or with lane and wave computed in here,
// they compiled to other code than before, see EXPERIMENTS.md.)
template <int K, int WAVES, typename F>
__device__ __forceinline__ void block_sums(double (&s)[K], double (&red)[WAVES][K], int lane, int wave, F&& f) {
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        s[k] = wave_sum(s[k]);
        if (lane == 0) red[wave][k] = s[k];
    }
    __syncthreads();
    if (t < K) {
        double sum = 0.0;
        for (int w = 0; w < WAVES; ++w) sum += red[w][t];
        f(sum);
    }
}

// A row's tile sums -> its parameter gradients: part holds P doubles per (row, tile), slot `slot` of tile b of row r at
// part[(r ntiles + b) P + slot]; they are added over b in double, in ascending order, and stored once as a float.  No
// atomics: equal bits from run to run.  `Slots` is the operation's map, passed by value:
//     float* dest(int64_t r, int64_t slot, double& scale) const      where the sum goes (null: nobody asked for it), and
//                                                                    what it is multiplied by first (1.0 on entry)
template <typename Slots>
__global__ __launch_bounds__(256) void tile_sums_finish_kernel(const double* __restrict__ part, Slots slots, int64_t R,
                                                               int64_t P, int64_t ntiles) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    for (int64_t e = tid; e < R * P; e += nthr) {
        const int64_t r = e / P, slot = e - r * P;
        double scale = 1.0;
        float* dst = slots.dest(r, slot, scale);
        if (!dst) continue;
        double s = 0.0;
        for (int64_t b = 0; b < ntiles; ++b) s += part[(r * ntiles + b) * P + slot];
        *dst = (float)(s * scale);
    }
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

// One launch: the opt-in for its dynamic LDS, the launch, its check.  GFX_OK or GFX_ELAUNCH.  A kernel that is only ever
// launched through here never runs without its opt-in.
template <typename K, typename... Args>
static inline int launch(K kernel, dim3 grid, dim3 block, size_t lds, hipStream_t stream, Args... args) {
    if (allow_lds(kernel, lds) != GFX_OK) return GFX_ELAUNCH;
    hipLaunchKernelGGL(kernel, grid, block, lds, stream, args...);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

// see tile_sums_finish_kernel: one thread per (row, slot), at most 65535 workgroups
template <typename Slots>
static inline int finish_tile_sums(const Slots& slots, const double* part, int64_t R, int64_t P, int64_t ntiles,
                                   hipStream_t stream) {
    const int64_t nb = (R * P + 255) / 256;
    return launch(tile_sums_finish_kernel<Slots>, dim3((unsigned)(nb > 65535 ? 65535 : nb)), dim3(256), 0, stream, part, slots,
                  R, P, ntiles);
}

// a workspace of `need` bytes for elements of alignment `align`: GFX_EINVAL for none or a misaligned one, else GFX_ENOSPC
// for a short one
static inline int workspace_ok(const void* ws, size_t ws_bytes, size_t need, size_t align) {
    if (!ws || reinterpret_cast<uintptr_t>(ws) % align) return GFX_EINVAL;
    return ws_bytes < need ? GFX_ENOSPC : GFX_OK;
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

// May a backward entry write the input gradient gx (nullable: nothing to test)?  Its map is valid and has no negative
// stride, and it shares no element with x or gy, which the kernels read while they write it.  (xmap and gmap without
// negative strides: the caller's test, the entries differ in when they make it.)
static inline bool grad_out_ok(const float* gx, const gfx_rowmap_t& gxmap, const float* x, const gfx_rowmap_t& xmap,
                               const float* gy, const gfx_rowmap_t& gmap, int64_t R, int64_t C, int64_t L) {
    if (!gx) return true;
    if (gxmap.inner <= 0 || map_negative(gxmap)) return false;
    return !signals_overlap(gx, gxmap, x, xmap, R, C, L) && !signals_overlap(gx, gxmap, gy, gmap, R, C, L);
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
// May a streaming entry read the state zi and write the state zf (both nullable, (R, C, S))?  The block's kernels read zi
// after zf's rows may have been written, so the two share no element (empty ranges never do), and the tail's grid fits:
// what an entry tests before its first launch.
static inline bool history_pair_ok(const float* zi, const float* zf, int64_t R, int64_t C, int64_t S) {
    const int64_t n = R * C * S;
    if (zi && zf && ranges_meet(zi, n, zf, n)) return false;
    return !zf || history_tail_blocks(R, C, S) <= MAX_GRID_X;
}

}  // namespace gfx
