// What the biquad cascade kernels share: biquad.hip (forward) and biquad_bwd.hip (backward) both include it.
#pragma once
#include "common.hpp"

namespace gfx {

constexpr int BQ_T = 64;             // threads per workgroup: one wave
constexpr int BQ_E = 8;              // samples per lane
constexpr int BQ_MAX_K = 32;
// Lanes per pair of row-channels, RL: 64 (the whole wave) or 16 (one DPP row; four pairs per wave) -- see the head of the file;
// 2048 stereo rows, K = 6: 1.5 ms with RL = 64 against 3.6 with RL = 16; 8192 rows, K = 2: 3.7 with RL = 16 against 4.5.

using f2 = float __attribute__((ext_vector_type(2)));   // (row-channel 2p, row-channel 2p + 1)
__device__ __forceinline__ f2 fma2(f2 a, f2 b, f2 c) { return __builtin_elementwise_fma(a, b, c); }

struct M2d {
    double a, b, c, d;
};
__device__ __forceinline__ M2d mul(const M2d& x, const M2d& y) {
    return {x.a * y.a + x.b * y.c, x.a * y.b + x.b * y.d, x.c * y.a + x.d * y.c, x.c * y.b + x.d * y.d};
}

struct SecConst {       // per (pair, section), in LDS; [4] = the matrix entries a, b, c, d
    f2 step[6][4];      // M^(E * 2^d)  (RL = 16 uses d < 4)
    f2 b0, b1, b2, a1, a2;
    f2 carry1, carry2;  // state (w[n-1], w[n-2]) entering the current tile
    f2 pad;
};
static_assert(sizeof(SecConst) == 256, "SecConst layout");
// LDS: SecConst sec[64 / RL][K]; for RL = 64 also f2 rowpow[K][16][4] = M^(E (j + 1)), j < 16

// (s1', s2') = M (s1, s2), the product rounded once before the fused multiply-add (as the scalar form did)
__device__ __forceinline__ void apply2(const f2 (&m)[4], f2 s1, f2 s2, f2& o1, f2& o2) {
    o1 = fma2(m[0], s1, m[1] * s2);
    o2 = fma2(m[2], s1, m[3] * s2);
}
// the value of the lane CTRL selects: 0x110 + n: n lanes below within the 16-lane row, 0x121: the row rotated right by one
// (lane 0 reads lane 15), 0x138: one lane below in the whole wave, 0x142 / 0x143: lane 15 of a row to the next row / lane 31
// to rows 2 and 3; zero where there is no such lane and in the rows ROWS (a mask of the wave's four) leaves out
template <int CTRL, int ROWS = 0xf>
__device__ __forceinline__ f2 dpp2(f2 v) {
    // (one 64-bit move, which the back end splits into two v_mov_b32_dpp: given two 32-bit builtins on .x and .y, hipcc
    // 7.2 folds the second into a copy of the first)
    const long long w = __builtin_amdgcn_update_dpp(0LL, __builtin_bit_cast(long long, v), CTRL, ROWS, 0xf, ROWS == 0xf);
    return __builtin_bit_cast(f2, w);
}

// lane 63's value, wave-uniform.  (The halves go through named floats: __builtin_bit_cast(int, v.y) of a vector element
// reads v.x with hipcc 7.2 -- the same front-end slip that made two 32-bit DPP builtins on .x / .y one.)
__device__ __forceinline__ f2 last_lane(f2 v) {
    const float x = v.x, y = v.y;
    return f2{__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x), 63)),
              __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), 63))};
}

}  // namespace gfx
