// The filter spectra of the overlap-save convolution (fftconv.hip): taps -> per-partition tile spectra.
//
// Kernel
//   hspec_kernel    taps -> per-partition tile spectra (He, Ho pairs in thread layout); REV: the taps are a signal row
//                   read backwards (the filter gradient's "filter")
#include "fftconv_tile.hpp"

namespace gfx {

// ------------------------------------------------------------------------------------------------
// REV: the taps of filter (r, c) are row (r, c) of `h` read backwards through `hmap` (tap k = h[r, c, N-1-k]).
template <bool REV>
__global__ __launch_bounds__(TILE_T, 2) void hspec_kernel(const float* __restrict__ h, const float* __restrict__ gain,
                                                          int64_t gain_div, float4* __restrict__ Hs, int64_t N,
                                                          int nparts, int64_t part_len, gfx_rowmap_t hmap, int C,
                                                          const float2* __restrict__ twtab) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const unsigned b = blockIdx.x;
    const unsigned rc = b / (unsigned)nparts;
    const int p = (int)(b - rc * (unsigned)nparts);
    const int64_t start = (int64_t)p * part_len;
    const int64_t len = min(part_len, N - start);

    TileTw tw;
    cx v[32], w[2][16];
    if (REV) {
        const unsigned r = rc / (unsigned)C;
        load_window_rev(v, h + row_off(hmap, r, (int)(rc - r * (unsigned)C)) + (N - start - len), len, t);
    } else {
        load_window(v, h + (int64_t)rc * N + start, 0, len, t, gain ? gain[rc / (unsigned)gain_div] : 1.0f);
    }
    tile_twiddles(tw, twtab, t);
    tile_forward(v, w, tw, lds, t);

    f4v* out = reinterpret_cast<f4v*>(Hs) + (int64_t)b * H_TILE_F4;
    const float sc = 1.0f / (4.0f * TILE_M);
    for_each_pair(t, tw.base(), [&](int slot, int ia, int ib, cx, bool) {
        cx he, ho;
        pair_split(NAT(w, ia), NAT(w, ib), he, ho);
        out[slot * TILE_T + t] = __builtin_shufflevector(he * sc, ho * sc, 0, 1, 2, 3);
    });
}

// the geometry, the grid check and the launch of both entries: `rows` filters of N taps each
template <bool REV>
static int launch_hspec(const float* h, const float* gain, int64_t gain_div, void* Hs, int64_t rows, int64_t N,
                        int64_t part_len, gfx_rowmap_t hmap, int C, void* stream) {
    const ConvGeom g = conv_geom(N, 1, part_len);
    if (!g.ok) return GFX_EINVAL;
    if (rows * g.nparts > 0x7fffffffLL) return GFX_EINVAL;
    if (allow_lds(hspec_kernel<REV>, TILE_LDS_BYTES)) return GFX_ELAUNCH;
    const float2* tw = tile_twiddle_table((hipStream_t)stream);
    if (!tw) return GFX_ELAUNCH;
    hipLaunchKernelGGL(hspec_kernel<REV>, dim3((unsigned)(rows * g.nparts)), dim3(TILE_T), TILE_LDS_BYTES, (hipStream_t)stream,
                       h, gain, gain_div, (float4*)Hs, N, (int)g.nparts, g.part_len, hmap, C, tw);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_fir_spectrum_bytes(int64_t RCf, int64_t N, int64_t part_len) {
    if (RCf <= 0 || N <= 0) return 0;
    const ConvGeom g = conv_geom(N, 1, part_len);
    return g.ok ? (size_t)RCf * g.nparts * H_TILE_F4 * sizeof(float4) : 0;
}

int gfx_fir_spectrum_f32(const float* h, const float* gain, int64_t gain_div, void* Hs, int64_t RCf, int64_t N,
                         int64_t part_len, void* stream) {
    if (!h || !Hs || RCf <= 0 || N <= 0 || (gain && gain_div <= 0)) return GFX_EINVAL;
    return launch_hspec<false>(h, gain, gain_div, Hs, RCf, N, part_len, gfx_rowmap_t{1, 0, 0, 0}, 1, stream);
}

int gfx_fir_spectrum_rev_f32(const float* x, gfx_rowmap_t xmap, int64_t R, int64_t C, int64_t L, int64_t part_len,
                             void* Hs, void* stream) {
    if (!x || !Hs || R <= 0 || C <= 0 || L <= 0 || xmap.inner <= 0 || xmap.inner > 0x7fffffffLL) return GFX_EINVAL;
    return launch_hspec<true>(x, nullptr, 1, Hs, R * C, L, part_len, xmap, (int)C, stream);
}

}  // extern "C"
