// Library-level entry points of the C ABI (include/grafx_amd.h).
#include <hip/hip_runtime.h>

#include <mutex>

#include "common.hpp"
#include "fft_tile.hpp"

namespace gfx {

__global__ void tile_twiddle_table_kernel(float2* __restrict__ table) {
    const int t = threadIdx.x;
    const int row = blockIdx.x;
    int num;
    double den;
    if (row < 4) { num = t * row; den = 8192.0; }
    else if (row < 12) { num = t * 4 * (row - 4); den = 8192.0; }
    else if (row < 16) { num = (t & 15) * (row - 12); den = 256.0; }
    else { num = (t & 15) * 4 * (row - 16); den = 256.0; }
    double s, c;
    sincospi(2.0 * (double)num / den, &s, &c);
    const float2 v = make_float2((float)c, (float)(-s));
    table[row * TILE_T + t] = v;
    table[TW_ROWS * TILE_T + (row >> 1) * 2 * TILE_T + 2 * t + (row & 1)] = v;   // the float4-pair copy
}

const float2* tile_twiddle_table(hipStream_t stream) {
    static std::mutex mu;
    static float2* tables[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tables[dev]) {
        float2* p = nullptr;
        if (hipMalloc(&p, sizeof(float2) * TW_TABLE_F2) != hipSuccess) return nullptr;
        // make the table visible to every stream before anyone else can use it
        if (launch(tile_twiddle_table_kernel, dim3(TW_ROWS), dim3(TILE_T), 0, stream, p) != GFX_OK ||
            hipStreamSynchronize(stream) != hipSuccess) {
            hipFree(p);
            return nullptr;
        }
        tables[dev] = p;
    }
    return tables[dev];
}

// see common.hpp (launch_history_tail).  Workgroup b copies chunk b % chunks of state row b / chunks.
__global__ __launch_bounds__(256) void history_tail_kernel(const float* __restrict__ x, gfx_rowmap_t xmap,
                                                           const float* __restrict__ zi, float* __restrict__ zf, int C,
                                                           int64_t L, int64_t S, unsigned chunks,
                                                           const int64_t* __restrict__ pos_in, int64_t* __restrict__ pos_out) {
    const unsigned rc = blockIdx.x / chunks, ch = blockIdx.x - rc * chunks;
    const unsigned r = rc / (unsigned)C;
    const int c = (int)(rc - r * (unsigned)C);
    const float* xrow = x + row_off(xmap, r, c);
    const float* zrow = zi ? zi + (int64_t)rc * S : nullptr;
    float* out = zf + (int64_t)rc * S;
#pragma unroll
    for (int q = 0; q < HISTORY_CHUNK / 256; ++q) {
        const int64_t i = (int64_t)ch * HISTORY_CHUNK + q * 256 + threadIdx.x;
        if (i >= S) continue;
        const int64_t k = i + L - S;                           // index into x; negative: still in the old history
        out[i] = k >= 0 ? xrow[k] : (zrow ? zrow[S + k] : 0.0f);
    }
    if (pos_out && c == 0 && ch == 0 && threadIdx.x == 0) pos_out[r] = (pos_in ? pos_in[r] : 0) + L;
}

int launch_history_tail(const float* x, gfx_rowmap_t xmap, const float* zi, float* zf, int64_t R, int64_t C, int64_t L,
                        int64_t S, const int64_t* pos_in, int64_t* pos_out, hipStream_t stream) {
    const int64_t blocks = history_tail_blocks(R, C, S);
    if (blocks <= 0 || blocks > MAX_GRID_X) return GFX_EINVAL;
    return launch(history_tail_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, x, xmap, zi, zf, (int)C, L, S,
                  (unsigned)((S + HISTORY_CHUNK - 1) / HISTORY_CHUNK), pos_in, pos_out);
}

}  // namespace gfx

extern "C" {

int gfx_abi_version(void) { return GFX_ABI_VERSION; }

int gfx_device_info(int* n_cu, size_t* lds_bytes) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return GFX_ELAUNCH;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return GFX_ELAUNCH;
    if (n_cu) *n_cu = prop.multiProcessorCount;
    if (lds_bytes) *lds_bytes = prop.maxSharedMemoryPerMultiProcessor;
    return GFX_OK;
}

}  // extern "C"
