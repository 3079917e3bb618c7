// The float instances of czt_pair.hpp (gfx_odd_alias_pair_*) and what does not depend on the working precision: the
// pair form's sizes and the row maxima behind its per-row scaling.
#include "czt_pair.hpp"

namespace gfx {

// bits of max |z[r, :]| (non-negative floats order like their bit patterns; a NaN sorts above everything)
constexpr int RMAX_SPAN = 8192;     // samples of a row per workgroup: eight 16-byte loads per thread, all in flight
typedef float rmax_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t rmax_abs(float x) { return __float_as_uint(x) & 0x7fffffffu; }
__global__ __launch_bounds__(256) void czt_rowmax_kernel(const float* __restrict__ z, int64_t P, uint32_t* __restrict__ rmax) {
    const float* row = z + (int64_t)blockIdx.y * P;
    // rows of odd length start at any multiple of four bytes: quads are taken from the 16-byte boundary below the row,
    // the first and the last quad of a row element by element
    const int mis = (int)(((uintptr_t)row >> 2) & 3);
    const rmax_f4* quads = reinterpret_cast<const rmax_f4*>(row - mis);
    const int64_t nq = (P + mis + 3) >> 2, q0 = (int64_t)blockIdx.x * (RMAX_SPAN / 4) + threadIdx.x;
    rmax_f4 v[RMAX_SPAN / 1024];
#pragma unroll
    for (int j = 0; j < RMAX_SPAN / 1024; ++j) {
        const int64_t q = q0 + j * 256;
        v[j] = rmax_f4{0.f, 0.f, 0.f, 0.f};
        if (q > 0 && q < nq - 1) {
            v[j] = quads[q];
        } else if (q < nq) {
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int64_t i = 4 * q - mis + c;
                if (i >= 0 && i < P) v[j][c] = row[i];
            }
        }
    }
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < RMAX_SPAN / 1024; ++j) {
        const uint32_t a = rmax_abs(v[j][0]), b = rmax_abs(v[j][1]), c = rmax_abs(v[j][2]), d = rmax_abs(v[j][3]);
        const uint32_t ab = a > b ? a : b, cd = c > d ? c : d, e = ab > cd ? ab : cd;
        m = e > m ? e : m;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const uint32_t t = (uint32_t)__shfl_xor((int)m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0 && m) atomicMax(rmax + blockIdx.y, m);
}

int czt_pair_rowmax(const float* z, int64_t rows, int64_t P, uint32_t* rmax, hipStream_t st) {
    if (hipMemsetAsync(rmax, 0, (size_t)rows * sizeof(uint32_t), st) != hipSuccess) return GFX_ELAUNCH;
    for (int64_t r0 = 0; r0 < rows; r0 += 65535) {     // rows ride on a grid dimension
        const int64_t n = rows - r0 < 65535 ? rows - r0 : 65535;
        hipLaunchKernelGGL(czt_rowmax_kernel, dim3((unsigned)((P + 3 + RMAX_SPAN - 1) / RMAX_SPAN), (unsigned)n), dim3(256), 0, st,
                           z + r0 * P, P, rmax + r0);
    }
    return GFX_OK;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_odd_alias_pair_plan_bytes(int64_t P) {
    CztGeom g;
    return czt_pair_geom(P, g) ? czt_pair_plan_t2(g) * sizeof(float2) : 0;
}

size_t gfx_odd_alias_pair_workspace_bytes(int64_t rows, int64_t P) {
    CztGeom g;
    if (rows <= 0 || !czt_pair_geom(P, g)) return 0;
    return (size_t)((rows + 1) / 2) * g.NFFT * sizeof(float2) + pair_rmax_bytes(rows);
}

int gfx_odd_alias_pair_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream) {
    return czt_pair_plan<float>(plan, P, ws, ws_bytes, (hipStream_t)stream);
}

int gfx_odd_alias_pair_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                           const void* plan, void* ws, size_t ws_bytes, const gfx_rowmap_t* ymap, int64_t C, int64_t row0,
                           const uint32_t* rowmax, void* stream) {
    if (!ymap) return czt_pair_alias<float>(z, y, ldy, lo, len, rows, P, plan, ws, ws_bytes, stream, nullptr, 0, 0, rowmax);
    if (C < 1 || C > 0x7fffffffLL || (row0 & 1)) return GFX_EINVAL;
    return czt_pair_alias<float>(z, y, len, lo, len, rows, P, plan, ws, ws_bytes, stream, ymap, (int)C, row0, rowmax);
}

}  // extern "C"
