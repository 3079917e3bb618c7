// What the dynamics files share -- dynamics.hip (the fused forward), dynamics_bwd.hpp (its backward), dyn_elementwise.hpp
// (the standalone stages) and ballistics_bwd.hpp (the ballistics adjoint): the tile geometry, the workgroup-wide one-pole
// scan, the bounded 4-sample loads / stores, the launch arguments, the pole-table layout and the host-side launch helpers.
// Device code is __forceinline__, host code static inline, the rest constexpr.
#pragma once
#include <type_traits>

#include "common.hpp"
#include "dyn_gain.hpp"

namespace gfx {

constexpr int DT = 256;            // threads per workgroup
constexpr int DE = 4;              // samples per thread per tile
constexpr int DTILE = DT * DE;     // 1024 samples per tile
constexpr int OS_HMAX = 256;       // taps of history a one-shot tile may re-read (tile: 1024 samples)
// per-parameter-row pole table (dyn_pole_table_kernel), floats per row:
//   a^(4 l) l < 64 | a_step[6] | a_wave | a_N | ap[0..4] | a | 1 - a | trunc | one-shot | H | look-back | M | a^(512 i) i < 64
constexpr int DP_TAB = 148;
constexpr int DP_ONESHOT = 80, DP_HIST = 81, DP_LOOKBACK = 82, DP_LB_TILES = 83, DP_LB_W = 84;

// the one-shot tiles of the forward and of the backward
constexpr int OS_SUB = 2;                  // 256-sample sub-tiles per wave tile (1: 5.1, 2: 6.0, 4: 5.6 TB/s -- profiles/r3/dyn_oneshot_ablation.txt)
constexpr int OS_WTILE = 64 * DE * OS_SUB; // 512 samples per wave (a multiple of 256: the history offsets assume it)
constexpr int OS_GTILE = OS_WTILE * (DT / 64);   // 2048 samples per workgroup

// a^k for integer k >= 0, rounded once from double (keeps long decays accurate)
__device__ __forceinline__ float powk(double log_a, double k) { return (float)exp(k * log_a); }

struct OnePole {
    float a;          // pole (already clamped)
    float one_m_a;    // 1 - a
    float ap[DE + 1]; // a^0 .. a^DE
    float a_lane;     // a^(DE * lane)
    float a_step[6];  // a^(DE * 2^d), d = 0..5 (in-wave scan offsets)
    float a_wave;     // a^(DE * 64)
    float a_N;        // a^N
    bool trunc;       // a^N not negligible
};

__device__ __forceinline__ void onepole_setup(OnePole& p, float z_alpha, int64_t N, int lane) {
    // core/envelope.py:51-54: alpha = clamp(sigmoid(z), max = 1 - 1e-5)
    p.a = fminf(sigmoidf(z_alpha), 1.0f - 1e-5f);
    p.one_m_a = 1.0f - p.a;
    const double la = log((double)p.a);
#pragma unroll
    for (int i = 0; i <= DE; ++i) p.ap[i] = powk(la, i);
    p.a_lane = powk(la, DE * lane);
#pragma unroll
    for (int d = 0; d < 6; ++d) p.a_step[d] = powk(la, DE << d);
    p.a_wave = powk(la, DE * 64);
    p.a_N = powk(la, (double)N);
    p.trunc = p.a_N > 1e-9f;
}

// One tile of the recursion u[n] = a u[n-1] + e[n] across the workgroup.
//   e[0..DE)  : this thread's inputs (tile-local positions DE*t .. DE*t+DE-1)
//   carry     : u at the end of the previous tile (same in every thread); updated
//   slots     : 4 floats of LDS for this tile parity
// returns u for the thread's DE positions.
__device__ __forceinline__ void scan_tile(const OnePole& p, const float (&e)[DE], float (&u)[DE], float& carry,
                                          float* slots, int lane, int wave) {
    float loc[DE];
    float s = 0.0f;
#pragma unroll
    for (int i = 0; i < DE; ++i) {
        s = fmaf(p.a, s, e[i]);
        loc[i] = s;
    }
    // inclusive scan of thread totals inside the wave: S_t += a^(DE*2^d) * S_(t - 2^d)
    float inc = s;
#pragma unroll
    for (int d = 0; d < 6; ++d) {
        const float up = __shfl_up(inc, 1 << d, 64);
        if (lane >= (1 << d)) inc = fmaf(p.a_step[d], up, inc);
    }
    if (lane == 63) slots[wave] = inc;
    float excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 0.0f;
    __syncthreads();
    float state = carry;  // u entering wave 0
    float entering = state;
#pragma unroll
    for (int w = 0; w < DT / 64; ++w) {
        if (w == wave) entering = state;
        state = fmaf(p.a_wave, state, slots[w]);
    }
    carry = state;
    const float pre = fmaf(p.a_lane, entering, excl);  // u just before this thread's first sample
#pragma unroll
    for (int i = 0; i < DE; ++i) u[i] = fmaf(p.ap[i + 1], pre, loc[i]);
}

// ---- loads / stores of 4 consecutive samples with bounds -----------------------------------------
// samples [n, n+4) of a row, zero outside [lo, L)
__device__ __forceinline__ void load4(const float* __restrict__ row, int64_t n, int64_t L, bool vec, float (&v)[DE],
                                      int64_t lo = 0) {
    if (vec && n + DE <= L && n >= lo) {
        const float4 q = *reinterpret_cast<const float4*>(row + n);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
        for (int i = 0; i < DE; ++i) v[i] = (n + i >= lo && n + i < L) ? row[n + i] : 0.0f;
    }
}
__device__ __forceinline__ void store4(float* __restrict__ row, int64_t n, int64_t L, bool vec, const float (&v)[DE]) {
    if (vec && n + DE <= L) {
        using f4 = float __attribute__((ext_vector_type(4)));
        __builtin_nontemporal_store(f4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f4*>(row + n));  // streamed output
    } else {
#pragma unroll
        for (int i = 0; i < DE; ++i)
            if (n + i < L) row[n + i] = v[i];
    }
}
__device__ __forceinline__ bool vec_ok(const float* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// the same for rows known to be 16-byte aligned with L % 4 == 0 and n % 4 == 0: one predicated 16-byte access, no
// element-wise path (which is most of the code of a kernel that inlines a dozen of these)
template <bool AL>
__device__ __forceinline__ void ld4(const float* __restrict__ row, int64_t n, int64_t L, bool vec, float (&v)[DE]) {
    if (AL) {
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (n >= 0 && n < L) q = *reinterpret_cast<const float4*>(row + n);
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
        load4(row, n, L, vec, v);
    }
}
template <bool AL>
__device__ __forceinline__ void st4(float* __restrict__ row, int64_t n, int64_t L, bool vec, const float (&v)[DE]) {
    if (AL) {
        using f4 = float __attribute__((ext_vector_type(4)));
        if (n < L) __builtin_nontemporal_store(f4{v[0], v[1], v[2], v[3]}, reinterpret_cast<f4*>(row + n));
    } else {
        store4(row, n, L, vec, v);
    }
}

struct DynArgs {
    gfx_rowmap_t xmap, ymap;
    int64_t R, L, N;       // rows, length, one-pole FIR length (iir smoother)
    int C;                 // channels
    int smoother;          // 0 none, 1 truncated one-pole
    int knee, gate;
    unsigned prows;        // parameter rows: row r uses parameters r % prows
    int nchunks;           // workgroups per row (time chunks; > 1 only with few rows, see the launcher)
    int64_t chunk_tiles;   // tiles per chunk
};

// ---- host side ---------------------------------------------------------------------------------------------------
static inline dim3 row_grid(int64_t R, int64_t L) {
    int64_t bx = (L + 255) / 256;
    if (bx > 64) bx = 64;
    return dim3((unsigned)bx, (unsigned)(R > 65535 ? 65535 : R));
}

// rows that whole 16-byte accesses may address: the base 16-byte aligned, every stride a multiple of four floats
static inline bool al16(const void* p, const gfx_rowmap_t& m) {
    return ((uintptr_t)p & 15) == 0 && ((m.stride_outer | m.stride_inner | m.stride_ch) & 3) == 0;
}

// Run-time choices as compile-time constants, for launchers of kernels that take them as template parameters: f is called
// with a std::bool_constant (with_bool) or with the knee kind as a std::integral_constant<int, 0..2> and compressor / gate
// as a std::bool_constant (with_knee), so the launcher names its kernel template once -- `kn()` is a constant expression
// -- and exactly the combinations it nests are instantiated.
template <typename F>
static inline void with_bool(bool b, F&& f) {
    if (b) f(std::true_type{});
    else f(std::false_type{});
}
template <typename F>
static inline void with_knee(int knee, bool gate, F&& f) {
    with_bool(gate, [&](auto gt) {
        if (knee == 0) f(std::integral_constant<int, 0>{}, gt);
        else if (knee == 1) f(std::integral_constant<int, 1>{}, gt);
        else f(std::integral_constant<int, 2>{}, gt);
    });
}

}  // namespace gfx

#define GFX_LAUNCH_OK() (hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH)
