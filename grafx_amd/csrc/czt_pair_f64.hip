// The double-precision instances of czt_pair.hpp (gfx_odd_alias_pair_precise_*) as a translation unit of their own: the
// column kernels are instantiated per tile count (35 sizes) and precision, and one file with both took four minutes to build.
#include "czt_pair.hpp"

using namespace gfx;

extern "C" {

size_t gfx_odd_alias_pair_precise_plan_bytes(int64_t P) { return 2 * gfx_odd_alias_pair_plan_bytes(P); }

size_t gfx_odd_alias_pair_precise_workspace_bytes(int64_t rows, int64_t P) { return 2 * gfx_odd_alias_pair_workspace_bytes(rows, P); }

int gfx_odd_alias_pair_precise_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream) {
    return czt_pair_plan<double>(plan, P, ws, ws_bytes, (hipStream_t)stream);
}

int gfx_odd_alias_pair_precise_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                                   const void* plan, void* ws, size_t ws_bytes, const uint32_t* rowmax, int relu,
                                   void* stream) {
    return czt_pair_alias<double>(z, y, ldy, lo, len, rows, P, plan, ws, ws_bytes, stream, nullptr, 0, 0, rowmax, relu);
}

}  // extern "C"
