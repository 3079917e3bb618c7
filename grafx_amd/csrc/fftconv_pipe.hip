// The hand-scheduled persistent kernels of the FFT-tile convolution and of its filter gradient
// (csrc/asm/gen_fftconv_pipe.py, gen_corr_pipe.py): assembled at build time into one gfx950 code object that is embedded
// here and loaded per device on first use (hipModuleLoadData: no file on disk, nothing to ship besides the library).
// Host code only: the module, the argument blocks and the launches.
#include "fftconv_pipe.hpp"

#include <cstdlib>
#include <cstring>
#include <mutex>

#include "fftconv_pipe_args.inc"
#include "fftconv_pipe_hsaco.inc"

namespace gfx {

struct PipeModule {
    hipModule_t mod = nullptr;
    hipFunction_t fn[sizeof(kPipeVariants) / sizeof(kPipeVariants[0])] = {};
    hipFunction_t corr = nullptr;
    int cus = 0;
    bool tried = false, ok = false;
};

PipeModule* pipe_module() {
    static std::mutex mu;
    static PipeModule mods[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    PipeModule& m = mods[dev];
    if (!m.tried) {
        m.tried = true;
        // GRAFX_PIPE_HSACO=<file>: load another build of the same kernels instead of the embedded one (schedule tuning:
        // `python -m grafx_amd.csrc.asm.gen_fftconv_pipe --hsaco f.hsaco <knobs>` needs no rebuild of the library)
        const char* alt = getenv("GRAFX_PIPE_HSACO");
        bool ok = (alt && *alt ? hipModuleLoad(&m.mod, alt) : hipModuleLoadData(&m.mod, kPipeCodeObject)) == hipSuccess;
        for (size_t i = 0; ok && i < sizeof(kPipeVariants) / sizeof(kPipeVariants[0]); ++i)
            ok = hipModuleGetFunction(&m.fn[i], m.mod, kPipeVariants[i].name) == hipSuccess;
        ok = ok && hipModuleGetFunction(&m.corr, m.mod, kCorrKernelName) == hipSuccess;
        ok = ok && hipDeviceGetAttribute(&m.cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && m.cus >= 8;
        m.ok = ok;
        (void)hipGetLastError();
    }
    return m.ok ? &m : nullptr;
}

int pipe_cus(const PipeModule* pm) { return pm->cus; }
const char* pipe_variant_name(int variant) { return kPipeVariants[variant].name; }

// q_est = mulhi(n, m) >> sh is floor(n / d) or one less for every 32-bit n (the kernel corrects by one)
static inline void pipe_magic(uint32_t d, uint32_t& m, uint32_t& sh) {
    sh = 31u - (uint32_t)__builtin_clz(d);
    const unsigned __int128 q = ((unsigned __int128)1 << (32 + sh)) / d;
    m = q > 0xffffffffu ? 0xffffffffu : (uint32_t)q;
}

// the kernel argument blocks are dwords: a pointer's halves, and a row map's strides in bytes (outer: 64 bits)
static inline uint32_t ptr_lo(const void* p) { return (uint32_t)reinterpret_cast<uint64_t>(p); }
static inline uint32_t ptr_hi(const void* p) { return (uint32_t)(reinterpret_cast<uint64_t>(p) >> 32); }
static inline bool pipe_strides_fit(const gfx_rowmap_t& mp) {
    return mp.stride_inner >= 0 && mp.stride_ch >= 0 && mp.stride_outer >= 0 && mp.stride_inner * 4 < (int64_t(1) << 32) &&
           mp.stride_ch * 4 < (int64_t(1) << 32);
}
static inline void pipe_strides(const gfx_rowmap_t& mp, uint32_t& olo, uint32_t& ohi, uint32_t& in, uint32_t& ch) {
    const uint64_t o = (uint64_t)mp.stride_outer * 4;
    olo = (uint32_t)o; ohi = (uint32_t)(o >> 32); in = (uint32_t)(mp.stride_inner * 4); ch = (uint32_t)(mp.stride_ch * 4);
}

// What the persistent kernels cover: one partition, no output offset, even row lengths (stores are whole sample pairs),
// the same batch-major row grouping on every tensor, byte strides inside 32 bits, and an overlap the build has a variant
// for.  Everything else runs on fftconv1_kernel.
int pipe_variant(const ConvArgs& a, const ConvGeom& g, bool tee, int64_t N) {
    if (g.nparts != 1 || a.off != 0 || (a.Lout & 1) || (tee && ((a.L & 1) || a.Lout != a.L)) || N > TILE_M + 1) return -1;
    if (a.L * 4 >= (int64_t(1) << 30) || a.Lout * 4 >= (int64_t(1) << 30)) return -1;
    if (a.xmap.inner != a.ymap.inner || (tee && a.cmap.inner != a.xmap.inner)) return -1;
    if (!pipe_strides_fit(a.xmap) || !pipe_strides_fit(a.ymap) || (tee && !pipe_strides_fit(a.cmap))) return -1;
    for (size_t i = 0; i < sizeof(kPipeVariants) / sizeof(kPipeVariants[0]); ++i)
        if (kPipeVariants[i].tee == tee && (int64_t)kPipeVariants[i].a_lo * 512 == a.O) return (int)i;
    return -1;
}

// (the argument block's rowmax descriptor, rm_*, stays all zeros: "not wanted".  The shipped code object is generated
// without that knob, see fftconv_sched.)
int launch_pipe(PipeModule* pm, int variant, const float* x, const void* Hs, float* y, float* xcopy, const ConvArgs& a,
                const float2* tw, hipStream_t st) {
    PipeKernArgs k;
    memset(&k, 0, sizeof(k));
    k.x_lo = ptr_lo(x); k.x_hi = ptr_hi(x); k.h_lo = ptr_lo(Hs); k.h_hi = ptr_hi(Hs); k.y_lo = ptr_lo(y); k.y_hi = ptr_hi(y);
    k.c_lo = ptr_lo(xcopy); k.c_hi = ptr_hi(xcopy); k.tw_lo = ptr_lo(tw); k.tw_hi = ptr_hi(tw);
    k.L_bytes = (uint32_t)(a.L * 4); k.Lout_bytes = (uint32_t)(a.Lout * 4);
    k.V_bytes = (uint32_t)(a.V * 4); k.O_bytes = (uint32_t)(a.O * 4);
    k.ntiles = (uint32_t)a.ntiles; k.nblocks = (uint32_t)a.nblocks;
    pipe_magic(k.ntiles, k.m_ntiles, k.sh_ntiles);
    k.inner = (uint32_t)a.xmap.inner;
    pipe_magic(k.inner, k.m_inner, k.sh_inner);
    k.hrows = a.hrows;
    pipe_magic(k.hrows, k.m_hrows, k.sh_hrows);
    k.cout_shift = a.Cout == 2 ? 1 : 0; k.cout_mask = a.Cout == 2 ? 1 : 0;
    k.cin_mask = a.Cin == 2 ? 1 : 0; k.cf_mask = a.Cf == 2 ? 1 : 0; k.Cf = (uint32_t)a.Cf;
    const unsigned grid = (unsigned)(2 * pm->cus) & ~7u;     // two resident workgroups per CU
    k.per_xcd = (uint32_t)((a.nblocks + grid - 1) / grid);   // tiles per workgroup: consecutive runs (the overlap is carried in registers)
    k.wgs_per_xcd = grid / 8;
    pipe_strides(a.xmap, k.xs_outer_lo, k.xs_outer_hi, k.xs_inner, k.xs_ch);
    pipe_strides(a.ymap, k.ys_outer_lo, k.ys_outer_hi, k.ys_inner, k.ys_ch);
    if (xcopy) pipe_strides(a.cmap, k.cs_outer_lo, k.cs_outer_hi, k.cs_inner, k.cs_ch);
    size_t size = sizeof(k);
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &k, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(pm->fn[variant], grid, 1, 1, TILE_T, 1, 1, 0, st, nullptr, config) == hipSuccess ? GFX_OK
                                                                                                              : GFX_ELAUNCH;
}

// The hand-scheduled form of corr1_kernel (csrc/asm/gen_corr_pipe.py) covers off = 0 with the same row grouping on x and
// g and byte strides inside 32 bits -- the equaliser's filter gradient; GRAFX_FFTCONV_SCHED=tile keeps corr1_kernel.
bool corr_pipe_ok(const CorrArgs& a) {
    if (a.off != 0 || a.N > TILE_M + 1 || a.xmap.inner != a.gmap.inner) return false;
    if (a.L * 4 >= (int64_t(1) << 30) || a.Lg * 4 >= (int64_t(1) << 30)) return false;
    return pipe_strides_fit(a.xmap) && pipe_strides_fit(a.gmap);
}

int launch_corr_pipe(PipeModule* pm, const float* x, const float* g, float* gh, const CorrArgs& a, const float2* tw,
                            hipStream_t st) {
    CorrKernArgs k;
    memset(&k, 0, sizeof(k));
    k.x_lo = ptr_lo(x); k.x_hi = ptr_hi(x); k.g_lo = ptr_lo(g); k.g_hi = ptr_hi(g); k.o_lo = ptr_lo(gh); k.o_hi = ptr_hi(gh);
    k.tw_lo = ptr_lo(tw); k.tw_hi = ptr_hi(tw);
    k.L_bytes = (uint32_t)(a.L * 4); k.Lg_bytes = (uint32_t)(a.Lg * 4); k.V_bytes = (uint32_t)(a.V * 4);
    k.N_even_bytes = (uint32_t)((a.N & ~int64_t(1)) * 4);
    k.ntiles = (uint32_t)a.ntiles; k.nblocks = (uint32_t)a.nblocks;
    k.inner = (uint32_t)a.xmap.inner;
    pipe_magic(k.inner, k.m_inner, k.sh_inner);
    k.cout_shift = a.Cout == 2 ? 1 : 0; k.cout_mask = a.Cout == 2 ? 1 : 0;
    k.cx_mask = a.Cx == 2 ? 1 : 0; k.cg_mask = a.Cg == 2 ? 1 : 0;
    k.out_row_bytes = (uint32_t)(a.N * 4);
    if (a.N & 1) {       // the last lag is half of a sample pair: stored on its own (row, lane, row offset of that pair)
        const uint32_t m = (uint32_t)((a.N - 1) / 2);
        k.tail_row = m >> 8; k.tail_lane = m & 255; k.tail_off = 2048u * (m >> 8);
    } else {
        k.tail_row = 255;
    }
    const float sc = 1.0f / (4.0f * TILE_M);
    memcpy(&k.scale, &sc, 4);
    const unsigned grid = pad8(a.nblocks);
    k.pad0 = grid / 8;
    pipe_strides(a.xmap, k.xs_outer_lo, k.xs_outer_hi, k.xs_inner, k.xs_ch);
    pipe_strides(a.gmap, k.gs_outer_lo, k.gs_outer_hi, k.gs_inner, k.gs_ch);
    size_t size = sizeof(k);
    void* config[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &k, HIP_LAUNCH_PARAM_BUFFER_SIZE, &size, HIP_LAUNCH_PARAM_END};
    return hipModuleLaunchKernel(pm->corr, grid, 1, 1, TILE_T, 1, 1, 0, st, nullptr, config) == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

// GFX_SCHED_AUTO: which of the two kernels a launch gets (the persistent kernel for large launches: decided by measurement,
// DESIGN.md section 4.2).  GRAFX_FFTCONV_SCHED=tile|pipe overrides (A/B measurements).
int auto_schedule() {
    static int cached = -1;
    if (cached < 0) {
        const char* e = getenv("GRAFX_FFTCONV_SCHED");
        cached = e && !strcmp(e, "pipe") ? GFX_SCHED_PIPE : (e && !strcmp(e, "tile") ? GFX_SCHED_TILE : GFX_SCHED_AUTO);
    }
    return cached;
}

}  // namespace gfx
