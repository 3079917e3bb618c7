// Multi-resolution STFT magnitude loss, one resolution per call: the four sums of a row
//     A = sum (|T| - |P|)^2,  B = sum |T|^2,  E = sum ||T| - |P||,  D = sum |log|T| - log|P||
// over the bins and frames of  P = stft(pred), T = stft(target)  (torch.stft: centred, reflect padding, one-sided), and
// the gradient of a linear combination of A, E, D with respect to pred.  Nothing of a spectrogram's size is ever written:
// the forward reads pred and target once and leaves 16 bytes per workgroup, the backward recomputes the frames and writes
// every gradient sample once.
//
// Frame transform.  A 256-thread workgroup holds SLOTS = 2048 complex points in LDS: 2048 / n_fft frames side by side
// (16 at n_fft = 128, one at 2048), so a thread owns 8 points whatever the size and takes three radix-2 stages per trip
// through LDS in registers: 4 passes at n_fft = 2048 instead of 11.  The kernels are compiled per n_fft (five sizes), so
// every index of a pass is a constant.  One complex transform carries the windowed pred frame in its real part and the
// target frame in its imaginary part; P and T are split by Z[k] +- conj(Z[n - k]).  Forward: decimation in frequency,
// natural order in, bit-reversed out.  The per-bin work runs on the bit-reversed positions (a thread owns the pair k,
// n - k), and the backward's inverse is decimation in time, bit-reversed in, natural out: no reordering pass.  Twiddles
// e^{-2 pi i j / n}, j < n / 2, are built once per workgroup from sincospi in double.  The samples are staged in LDS
// first (reflection applied there), in a ring over the positions: a workgroup takes consecutive batches, so each sample
// is read from memory once per workgroup, and in the forward the samples the next batch adds are in flight while this
// one is transformed.
//
// LDS per workgroup: 16.5 KB transform buffer (padded) + n_fft * 4 + 2 KB (twiddles, and again per stage for the fine
// stages) + n_fft * 4 (window) + 16 KB (the rings of pred and target, 2048 samples each) + 64 = 50.6 KB at n_fft = 2048,
// 35.6 KB at 128: three or four workgroups per CU.
//
// A batch whose staged pred and target samples are the same floats has |T| - |P| = 0 identically; the split above would
// return it as rounding noise, so such a batch contributes B only (forward) and no gradient (backward).
#include "stft_loss.hpp"

namespace gfx {
namespace stftloss {

template <int LOGN>
__global__ __launch_bounds__(THREADS) void stft_loss_sums_kernel(const float* __restrict__ pred, gfx_rowmap_t pmap,
                                                                 const float* __restrict__ target, gfx_rowmap_t tmap,
                                                                 const float* __restrict__ window,
                                                                 float4* __restrict__ partials, Geometry g, int chunks,
                                                                 float eps) {
    constexpr int NB = Size<LOGN>::NB;
    extern __shared__ __attribute__((aligned(16))) char stft_loss_lds[];
    const Image im = carve<LOGN>(stft_loss_lds);
    const int64_t row = blockIdx.x / (unsigned)chunks;
    const int chunk = (int)(blockIdx.x % (unsigned)chunks);
    const float* p = pred + sig_row_off(pmap, row);
    const float* t = target + sig_row_off(tmap, row);
    build_tables<LOGN>(im, window);
    Sums s = {0.0f, 0.0f, 0.0f, 0.0f};
    const int64_t m0 = (int64_t)chunk * RUN * NB;
    const int spanv = (NB - 1) * g.hop + Size<LOGN>::N, adv = NB * g.hop;      // positions of a batch, and from one to the next
    Fetch next;
    fetch<LOGN>(next, p, t, m0 * g.hop, spanv, g.L);
    commit(im, next, m0 * g.hop, spanv);
    for (int r = 0; r < RUN; ++r) {
        const int64_t mb = m0 + (int64_t)r * NB;
        if (mb >= g.frames) break;                           // (the same for every thread)
        __syncthreads();                                     // the ring holds the batch, the buffer is free
        int differ = fill<LOGN>(im, mb, g);
        const bool more = r + 1 < RUN && mb + NB < g.frames;
        if (more) fetch<LOGN>(next, p, t, mb * g.hop + spanv, adv, g.L);
        const bool same = !__syncthreads_or(differ);
        fft_dif<LOGN>(im.z, im.tw, im.fine);
        const int valid = (int)lo(NB, g.frames - mb);
#pragma unroll
        for (int q = 0; q < SLOTS / 2 / THREADS; ++q) {
            const Bins o = bins_of<LOGN>(threadIdx.x + q * THREADS);
            if (o.f >= valid) continue;
            float2 P, T;
            split(im.z[pad(o.pk)], im.z[pad(o.pm)], P, T);
            add_bin(s, P, T, eps, same);
            if (o.k == 0) {
                const float2 zh = im.z[pad(o.pk + 1)];       // bin n / 2
                add_bin(s, make_float2(zh.x, 0.0f), make_float2(zh.y, 0.0f), eps, same);
            }
        }
        if (more) commit(im, next, mb * g.hop + spanv, adv);
    }
    // one quadruple per workgroup: lanes, then waves, in a fixed order
    for (int o = 32; o >= 1; o >>= 1) {
        s.A += __shfl_down(s.A, o, 64);
        s.B += __shfl_down(s.B, o, 64);
        s.E += __shfl_down(s.E, o, 64);
        s.D += __shfl_down(s.D, o, 64);
    }
    __syncthreads();
    float4* red = reinterpret_cast<float4*>(im.red);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float4(s.A, s.B, s.E, s.D);
    __syncthreads();
    if (threadIdx.x == 0) {
        float4 a = red[0];
        for (int w = 1; w < THREADS / 64; ++w) {
            a.x += red[w].x;
            a.y += red[w].y;
            a.z += red[w].z;
            a.w += red[w].w;
        }
        partials[blockIdx.x] = a;
    }
}

// a row's partials in their order, in double
__global__ __launch_bounds__(THREADS) void stft_loss_finish_kernel(const float4* __restrict__ partials,
                                                                   float4* __restrict__ sums, int64_t R, int chunks) {
    const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (row >= R) return;
    double A = 0.0, B = 0.0, E = 0.0, D = 0.0;
    const float4* q = partials + row * chunks;
    for (int c = 0; c < chunks; ++c) {
        const float4 v = q[c];
        A += v.x;
        B += v.y;
        E += v.z;
        D += v.w;
    }
    sums[row] = make_float4((float)A, (float)B, (float)E, (float)D);
}

void finish_sums(const void* partials, float* sums, int64_t R, int64_t chunks, hipStream_t stream) {
    hipLaunchKernelGGL(stft_loss_finish_kernel, dim3((unsigned)((R + THREADS - 1) / THREADS)), dim3(THREADS), 0, stream,
                       (const float4*)partials, (float4*)sums, R, (int)chunks);
}

// Gather form: the workgroup owns samples [s0, s0 + SEG) of one row, transforms every frame that reaches them -- directly
// or through the reflection at either end -- and each thread adds, for its own CELLS samples, the windowed inverse of
// every such frame at the (up to three) padded positions that fold onto the sample.
template <int LOGN>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 8))) void stft_loss_bwd_kernel(
    const float* __restrict__ pred, gfx_rowmap_t pmap, const float* __restrict__ target, gfx_rowmap_t tmap,
    const float* __restrict__ window, const float* __restrict__ coef, float* __restrict__ gpred, gfx_rowmap_t gmap, Geometry g,
    int segs, float eps, int accumulate) {
    constexpr int N = Size<LOGN>::N, HALF = Size<LOGN>::HALF, NB = Size<LOGN>::NB;
    extern __shared__ __attribute__((aligned(16))) char stft_loss_lds[];
    const Image im = carve<LOGN>(stft_loss_lds);
    const int64_t row = blockIdx.x / (unsigned)segs;
    const int64_t s0 = (int64_t)(blockIdx.x % (unsigned)segs) * SEG;
    const int64_t s1 = lo(s0 + SEG, g.L);          // one past the last owned sample
    const float* p = pred + sig_row_off(pmap, row);
    const float* t = target + sig_row_off(tmap, row);
    float* out = gpred + sig_row_off(gmap, row);
    const float cA = coef[row * 3], cE = coef[row * 3 + 1], cD = coef[row * 3 + 2];
    const int64_t last = g.L - 1, half = HALF, n = N, hop = g.hop;

    // the hull of the frames that reach the segment (a frame inside it that reaches nothing adds nothing below)
    auto first_frame = [&](int64_t pq) { const int64_t a = pq - n + 1; return a <= 0 ? (int64_t)0 : (a + hop - 1) / hop; };
    int64_t mlo = first_frame(s0 + half), mhi = (s1 - 1 + half) / hop;
    if (s0 <= half && s1 - 1 >= 1) {                         // samples 1 .. half also stand at -1 .. -half
        mlo = 0;
        mhi = hi(mhi, (half - hi(1, s0)) / hop);
    }
    const int64_t ra = hi(s0, last - half), rb = lo(s1 - 1, last - 1);
    if (ra <= rb) {                                          // samples L-1-half .. L-2 also stand at L .. L-1+half
        mlo = lo(mlo, first_frame(2 * last - rb + half));
        mhi = hi(mhi, (2 * last - ra + half) / hop);
    }
    mhi = lo(mhi, g.frames - 1);

    build_tables<LOGN>(im, window);
    float acc[CELLS];
#pragma unroll
    for (int q = 0; q < CELLS; ++q) acc[q] = 0.0f;

    const int spanv = (NB - 1) * g.hop + N, adv = NB * g.hop;  // positions of a batch, and from one to the next
    Fetch next;
    fetch<LOGN>(next, p, t, mlo * hop, spanv, g.L);
    commit(im, next, mlo * hop, spanv);
    for (int64_t mb = mlo; mb <= mhi; mb += NB) {
        __syncthreads();                                     // the ring holds the batch, the buffer is free
        int differ = fill<LOGN>(im, mb, g);
        const bool more = mb + NB <= mhi;
        if (more) fetch<LOGN>(next, p, t, mb * hop + spanv, adv, g.L);
        const bool same = !__syncthreads_or(differ);
        // (committed before the transform, unlike the forward: this kernel has no registers to hold the samples through it)
        if (more) commit(im, next, mb * hop + spanv, adv);
        if (same) continue;                                  // pred is target here: no gradient (the same for every thread)
        fft_dif<LOGN>(im.z, im.tw, im.fine);
#pragma unroll
        for (int q = 0; q < SLOTS / 2 / THREADS; ++q) {
            const Bins o = bins_of<LOGN>(threadIdx.x + q * THREADS);
            float2 P, T;
            split(im.z[pad(o.pk)], im.z[pad(o.pm)], P, T);
            if (o.k == 0) {
                const float2 zh = im.z[pad(o.pk + 1)];
                im.z[pad(o.pk)] = bin_grad(P, T, eps, cA, cE, cD);
                im.z[pad(o.pk + 1)] = bin_grad(make_float2(zh.x, 0.0f), make_float2(zh.y, 0.0f), eps, cA, cE, cD);
            } else {
                im.z[pad(o.pk)] = bin_grad(P, T, eps, cA, cE, cD);
                im.z[pad(o.pm)] = make_float2(0.0f, 0.0f);   // bins above n / 2 are not part of the one-sided transform
            }
        }
        __syncthreads();
        ifft_dit<LOGN>(im.z, im.tw, im.fine);
        const int nbv = (int)lo(NB, g.frames - mb);          // frames of the batch
        const int64_t q0 = mb * hop - half;                  // sample index (before reflection) of the batch's first point
#pragma unroll
        for (int q = 0; q < CELLS; ++q) {
            const int64_t i = s0 + threadIdx.x + q * THREADS;
            if (i >= s1) continue;
            float a = acc[q];
#pragma unroll 1
            for (int e = 0; e < 3; ++e) {                    // the sample itself, its mirror before 0, its mirror beyond L - 1
                const int64_t u = e == 0 ? i : (e == 1 ? -i : 2 * last - i);
                const bool on = e == 0 || (e == 1 ? i >= 1 && i <= half : i <= last - 1 && i >= last - half);
                const int64_t d = u - q0;                    // position inside the batch's span
                if (!on || d < 0 || d >= spanv) continue;
#pragma unroll 1
                for (int f = 0; f < nbv; ++f) {
                    const int j = (int)d - f * g.hop;
                    if ((unsigned)j < (unsigned)N) a += im.win[j] * im.z[pad((f << LOGN) + j)].x;
                }
            }
            acc[q] = a;
        }
    }
#pragma unroll
    for (int q = 0; q < CELLS; ++q) {
        const int64_t i = s0 + threadIdx.x + q * THREADS;
        if (i < s1) out[i] = accumulate ? out[i] + acc[q] : acc[q];
    }
}

}  // namespace stftloss
}  // namespace gfx

extern "C" {

size_t gfx_stft_loss_ws_bytes(int64_t R, int64_t L, int64_t n_fft, int64_t hop) {
    gfx::stftloss::Geometry g;
    int logn;
    if (R <= 0 || !gfx::stftloss::geometry(g, logn, L, n_fft, hop)) return 0;
    return (size_t)R * (size_t)gfx::stftloss::chunks_of(g, n_fft) * 16;
}

int gfx_stft_loss_sums_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap, const float* window,
                           float* sums, int64_t R, int64_t L, int64_t n_fft, int64_t hop, float eps, void* ws,
                           size_t ws_bytes, void* stream) {
    using namespace gfx::stftloss;
    Geometry g;
    int logn;
    int64_t chunks;
    const int rc =
        check_entry(pred && target && window && sums, pmap, tmap, R, L, n_fft, hop, eps, ws, ws_bytes, g, logn, chunks);
    if (rc != GFX_OK) return rc;
    hipStream_t s = (hipStream_t)stream;
#define GFX_LAUNCH(LOGN)                                                                                                  \
    hipLaunchKernelGGL(stft_loss_sums_kernel<LOGN>, dim3((unsigned)(R * chunks)), dim3(THREADS), lds_bytes(n_fft), s, pred, \
                       pmap, target, tmap, window, (float4*)ws, g, (int)chunks, eps)
    GFX_STFT_LOSS_BY_SIZE(logn, GFX_LAUNCH)
#undef GFX_LAUNCH
    finish_sums(ws, sums, R, chunks, s);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_stft_loss_bwd_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap, const float* window,
                          const float* coef, float* gpred, gfx_rowmap_t gmap, int64_t R, int64_t L, int64_t n_fft,
                          int64_t hop, float eps, int accumulate, void* ws, size_t ws_bytes, void* stream) {
    using namespace gfx::stftloss;
    Geometry g;
    int logn;
    int64_t chunks, segs;
    const int rc = check_entry(pred && target && window && coef && gpred && gmap.inner > 0, pmap, tmap, R, L, n_fft, hop, eps,
                               ws, ws_bytes, g, logn, chunks, &segs);
    if (rc != GFX_OK) return rc;
#define GFX_LAUNCH(LOGN)                                                                                               \
    hipLaunchKernelGGL(stft_loss_bwd_kernel<LOGN>, dim3((unsigned)(R * segs)), dim3(THREADS), lds_bytes(n_fft),          \
                       (hipStream_t)stream, pred, pmap, target, tmap, window, coef, gpred, gmap, g, (int)segs, eps, accumulate)
    GFX_STFT_LOSS_BY_SIZE(logn, GFX_LAUNCH)
#undef GFX_LAUNCH
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
