// The hand-scheduled persistent kernels (csrc/asm/gen_fftconv_pipe.py, gen_corr_pipe.py) as the convolution and the filter
// gradient see them: the per-device module, which launches it covers, and the launchers.  One definition of each in
// fftconv_pipe.hip -- the module and the environment switch are static state that must exist once in the library.
#pragma once
#include "fftconv_tile.hpp"

namespace gfx {

struct PipeModule;

// the device's module, loaded on the first call on that device; nullptr: the kernels are not available
PipeModule* pipe_module();
int pipe_cus(const PipeModule* pm);                // compute units of the module's device
const char* pipe_variant_name(int variant);        // the kernel's own name (gfx_fftconv_last_kernel)

// GFX_SCHED_AUTO, or what GRAFX_FFTCONV_SCHED=tile|pipe overrides it with
int auto_schedule();

// the build's variant for this launch (tee: with the input copy), -1: not covered, the launch runs on fftconv1_kernel
int pipe_variant(const ConvArgs& a, const ConvGeom& g, bool tee, int64_t N);
int launch_pipe(PipeModule* pm, int variant, const float* x, const void* Hs, float* y, float* xcopy, const ConvArgs& a,
                const float2* tw, hipStream_t st);

bool corr_pipe_ok(const CorrArgs& a);
int launch_corr_pipe(PipeModule* pm, const float* x, const float* g, float* gh, const CorrArgs& a, const float2* tw,
                     hipStream_t st);

}  // namespace gfx
