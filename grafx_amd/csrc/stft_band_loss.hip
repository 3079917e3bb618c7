// The STFT magnitude loss of stft_loss.hip on a filterbank scale (mel, bark, third octaves, per-bin weights, a band limit):
// with W an (n_bins, n_fft / 2 + 1) matrix of non-negative weights,
//     Pm[m] = sum_k W[m, k] |P|_k,  Tm likewise,
//     A = sum (Tm - Pm)^2,  B = sum Tm^2,  E = sum |Tm - Pm|,  D = sum |log Tm - log Pm|
// over the n_bins bands of every frame, and the gradient of a linear combination of A, E, D with respect to pred.  The
// clamp stays on the bins, the logarithm moves to the bands.  Same tile, same transform, same sample ring and the same
// workspace as the plain loss (stft_loss.hpp); nothing of a spectrogram's size is written here either.
//
// W is staircase banded: the non-zeros of row m are the run [row_lo[m], row_hi[m]), both ends non-decreasing in m, so
// the rows that touch bin k are a run [col_lo[k], col_hi[k]) too.  W is read from global memory, dense and row-major, the
// band entries only (a mel bank has at most two per column: a few KB that stay in L2); the LDS image is the plain one.
//
// What a batch adds to the plain kernels.  The per-bin work runs on bit-reversed positions, a band sum wants consecutive
// bins, so after the transform every thread takes |P|, |T| of its bins into registers, a barrier ends all reads of the
// transform buffer, and the magnitudes go over it as float2(|P|, |T|) in natural order (frame f, bin k at
// nat(f (n/2 + 1) + k): 8.8 KB of the 16.5 KB that are free until the next fill).  After a second barrier a fixed group
// of 16 lanes reduces one band -- lane l takes the bins lo + l, lo + l + 16, ..., then four exchanges -- whatever its
// width (1 bin to all of them), in a fixed order: equal bits from run to run, no atomics.  The forward adds the band's
// terms to the four register sums of the group's first lane: two barriers more than the plain kernel per batch.  The
// backward keeps the complex P of its bins in registers meanwhile, has the groups write
//     g_m = 2 cA (Pm - Tm) + cE sign(Pm - Tm) + cD sign(log Pm - log Tm) / Pm
// behind the magnitudes (n_bins floats per frame), and after a barrier every bin gathers
//     G_k = live_k (sum_{m in [col_lo[k], col_hi[k])} W[m, k] g_m) P_k / |P|_k
// into the registers that held P; one more barrier frees the buffer, G goes to the bit-reversed slots (zeros above n / 2)
// and the inverse, the overlap-add and the fold run as in stft_loss_bwd_kernel: four barriers more per batch.
#include "stft_loss.hpp"

namespace gfx {
namespace stftloss {

constexpr int GROUP = 16;                    // lanes that reduce one band
constexpr int GROUPS = THREADS / GROUP;
constexpr int PER = SLOTS / 2 / THREADS;     // bin pairs (k, n - k) per thread

// Where natural-order entry i of the magnitudes lives: one float2 of padding after every 16.  A wave writes bins that are
// n / 128 apart (the bit reversal of consecutive positions), which at n = 2048 would all meet on one bank pair.
__device__ __forceinline__ constexpr int nat(int i) { return i + (i >> 4); }
constexpr int G_FLOATS = SLOTS / 2 + SLOTS / 128;            // up to 16 frames of n / 2 + 1 bins: 1040 entries at most,
constexpr int MAG_SLOTS = G_FLOATS + G_FLOATS / 16;          // and g_m: n_bins <= n / 2 + 1 per frame
static_assert(MAG_SLOTS * sizeof(float2) + G_FLOATS * sizeof(float) <= ZSIZE * sizeof(float2),
              "the magnitudes and the band gradients lie over the transform buffer");

struct Bands {
    const float* fb;
    const int32_t* row_lo;
    const int32_t* row_hi;
    const int32_t* col_lo;                   // (the backward only)
    const int32_t* col_hi;
    int n_bins;
};

// The thread's index as a value the compiler takes anew in every batch: the positions of the band stage are functions of
// it alone, and computed once before the loop over the batches they would occupy registers through both transforms.
__device__ __forceinline__ int per_batch(int tid) {
    asm volatile("" : "+v"(tid));
    return tid;
}

__device__ __forceinline__ float2 magnitudes(float2 P, float2 T, float eps) {
    return make_float2(__builtin_amdgcn_sqrtf(fmaxf(P.x * P.x + P.y * P.y, eps)),
                       __builtin_amdgcn_sqrtf(fmaxf(T.x * T.x + T.y * T.y, eps)));
}

// x of the lane the DPP control names, within the row of 16 lanes a group is
template <int CTRL>
__device__ __forceinline__ float row_lane(float x) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(x), CTRL, 0xF, 0xF, false));
}

// the sum over the group's 16 lanes, in every lane: neighbours, pairs, then the mirrored quad and the mirrored half
__device__ __forceinline__ float group_sum(float x) {
    x += row_lane<0xB1>(x);                  // quad_perm [1, 0, 3, 2]
    x += row_lane<0x4E>(x);                  // quad_perm [2, 3, 0, 1]
    x += row_lane<0x141>(x);                 // row_half_mirror
    x += row_lane<0x140>(x);                 // row_mirror
    return x;
}

// (Pm, Tm) of band m of frame f, in every lane of the group.  The run is cut to the bins that exist: what the band
// arrays hold is the caller's, what this kernel reads is not.
template <int LOGN>
__device__ __forceinline__ float2 band_sum(const float2* mag, const Bands& bd, int f, int m, int lane) {
    constexpr int BINS = Size<LOGN>::HALF + 1;
    const int k0 = max(bd.row_lo[m], 0), k1 = min(bd.row_hi[m], BINS);
    const float* __restrict__ w = bd.fb + (int64_t)m * BINS;
    float a = 0.0f, b = 0.0f;
    for (int k = k0 + lane; k < k1; k += GROUP) {
        const float wk = w[k];
        const float2 v = mag[nat(f * BINS + k)];
        a += wk * v.x;
        b += wk * v.y;
    }
    return make_float2(group_sum(a), group_sum(b));
}

__device__ __forceinline__ void add_band(Sums& s, float pm, float tm, bool same) {
    s.B += tm * tm;
    if (same) return;
    const float d = tm - pm;
    s.A += d * d;
    s.E += fabsf(d);
    s.D += fabsf(__logf(tm * __builtin_amdgcn_rcpf(pm)));
}

// Bin n / 2 of frame f stands at position 1 of the frame, real in both signals (pred in .x, target in .y).  The slot that
// owns k = 0 leaves it alone here: thread f < NB takes it, so that a thread carries one such bin, not one per slot.
template <int LOGN>
__device__ __forceinline__ constexpr int nyquist(int f) { return pad((f << LOGN) + 1); }

// |P|, |T| of this thread's bins k < n / 2 out of the transformed buffer (and P itself for the backward), and the raw
// bin n / 2 of frame tid
template <int LOGN, bool KEEP>
__device__ __forceinline__ void take_bins(const Image& im, int tid, float eps, float2 (&m)[PER], float2& zh, float2 (&P)[PER]) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const Bins o = bins_of<LOGN>(tid + q * THREADS);
        float2 p, t;
        split(im.z[pad(o.pk)], im.z[pad(o.pm)], p, t);
        m[q] = magnitudes(p, t, eps);
        if (KEEP) P[q] = p;
    }
    zh = tid < Size<LOGN>::NB ? im.z[nyquist<LOGN>(tid)] : make_float2(0.0f, 0.0f);
}

template <int LOGN>
__device__ __forceinline__ void put_magnitudes(float2* mag, int tid, float eps, const float2 (&m)[PER], float2 zh) {
    constexpr int HALF = Size<LOGN>::HALF, BINS = HALF + 1;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const Bins o = bins_of<LOGN>(tid + q * THREADS);
        mag[nat(o.f * BINS + o.k)] = m[q];
    }
    if (tid < Size<LOGN>::NB) mag[nat(tid * BINS + HALF)] = magnitudes(make_float2(zh.x, 0.0f), make_float2(zh.y, 0.0f), eps);
}

template <int LOGN>
__global__ __launch_bounds__(THREADS) void stft_band_loss_sums_kernel(const float* __restrict__ pred, gfx_rowmap_t pmap,
                                                                      const float* __restrict__ target, gfx_rowmap_t tmap,
                                                                      const float* __restrict__ window, Bands bd,
                                                                      float4* __restrict__ partials, Geometry g, int chunks,
                                                                      float eps) {
    constexpr int NB = Size<LOGN>::NB;
    extern __shared__ __attribute__((aligned(16))) char stft_loss_lds[];
    const Image im = carve<LOGN>(stft_loss_lds);
    float2* mag = im.z;
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
        const int tid = per_batch(threadIdx.x);
        const int lane = tid & (GROUP - 1), group = tid / GROUP;
        {
            float2 m[PER], none[PER], zh;
            take_bins<LOGN, false>(im, tid, eps, m, zh, none);
            __syncthreads();                                 // every read of the transform is done
            put_magnitudes<LOGN>(mag, tid, eps, m, zh);
        }
        __syncthreads();
        const int bands = (int)lo(NB, g.frames - mb) * bd.n_bins;
        for (int j = group, f = 0, m = group; j < bands; j += GROUPS, m += GROUPS) {        // (a group's lanes share j)
            for (; m >= bd.n_bins; m -= bd.n_bins) ++f;      // band j is band m = j % n_bins of frame f = j / n_bins
            const float2 b = band_sum<LOGN>(mag, bd, f, m, lane);
            if (lane == 0) add_band(s, b.x, b.y, same);
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

// G of bin k of frame f from the band gradients gm of the frame: P scaled by sum_m W[m, k] g_m / |P|, nothing where the
// bin is clamped or no row covers it
template <int LOGN>
__device__ __forceinline__ float2 gather_bin(const float* gm, const Bands& bd, int f, int k, float2 P, float eps) {
    constexpr int BINS = Size<LOGN>::HALF + 1;
    const float p2 = P.x * P.x + P.y * P.y;
    if (!(p2 > eps)) return make_float2(0.0f, 0.0f);
    const int m0 = max(bd.col_lo[k], 0), m1 = min(bd.col_hi[k], bd.n_bins);
    const float* __restrict__ w = bd.fb + k;
    float s = 0.0f;
    for (int m = m0; m < m1; ++m) s += w[(int64_t)m * BINS] * gm[f * bd.n_bins + m];
    s *= __builtin_amdgcn_rsqf(p2);
    return make_float2(s * P.x, s * P.y);
}

// stft_loss_bwd_kernel with the band stage between the two transforms
template <int LOGN>
__global__ __launch_bounds__(THREADS) __attribute__((amdgpu_waves_per_eu(3, 8))) void stft_band_loss_bwd_kernel(
    const float* __restrict__ pred, gfx_rowmap_t pmap, const float* __restrict__ target, gfx_rowmap_t tmap,
    const float* __restrict__ window, Bands bd, const float* __restrict__ coef, float* __restrict__ gpred, gfx_rowmap_t gmap,
    Geometry g, int segs, float eps, int accumulate) {
    constexpr int N = Size<LOGN>::N, HALF = Size<LOGN>::HALF, NB = Size<LOGN>::NB;
    extern __shared__ __attribute__((aligned(16))) char stft_loss_lds[];
    const Image im = carve<LOGN>(stft_loss_lds);
    float2* mag = im.z;
    float* gm = reinterpret_cast<float*>(im.z + MAG_SLOTS);
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
        const int at = per_batch(threadIdx.x);
        int differ = fill<LOGN>(im, mb, g, at);
        const bool more = mb + NB <= mhi;
        if (more) fetch<LOGN>(next, p, t, mb * hop + spanv, adv, g.L, at);
        const bool same = !__syncthreads_or(differ);
        if (more) commit(im, next, mb * hop + spanv, adv, at);
        if (same) continue;                                  // pred is target here: no gradient (the same for every thread)
        fft_dif<LOGN>(im.z, im.tw, im.fine);
        const int nbv = (int)lo(NB, g.frames - mb);          // frames of the batch
        const int tid = per_batch(threadIdx.x);
        const int lane = tid & (GROUP - 1), group = tid / GROUP;
        float2 P[PER], zh;
        {
            float2 m[PER];
            take_bins<LOGN, true>(im, tid, eps, m, zh, P);
            __syncthreads();                                 // every read of the transform is done
            put_magnitudes<LOGN>(mag, tid, eps, m, zh);
        }
        __syncthreads();
        for (int j = group, f = 0, m = group; j < NB * bd.n_bins; j += GROUPS, m += GROUPS) {      // (a group's lanes share j)
            for (; m >= bd.n_bins; m -= bd.n_bins) ++f;      // band j is band m = j % n_bins of frame f = j / n_bins
            float gj = 0.0f;                                 // frames that do not exist
            if (f < nbv) {
                const float2 b = band_sum<LOGN>(mag, bd, f, m, lane);
                const float d = b.x - b.y;
                const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
                gj = 2.0f * cA * d + sg * (cE + cD * __builtin_amdgcn_rcpf(b.x));
            }
            if (lane == 0) gm[j] = gj;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const Bins o = bins_of<LOGN>(tid + q * THREADS);
            P[q] = gather_bin<LOGN>(gm, bd, o.f, o.k, P[q], eps);
        }
        if (tid < NB) zh = gather_bin<LOGN>(gm, bd, tid, HALF, make_float2(zh.x, 0.0f), eps);
        __syncthreads();                                     // the band gradients are read: the buffer is the transform's again
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const Bins o = bins_of<LOGN>(tid + q * THREADS);
            im.z[pad(o.pk)] = P[q];
            if (o.k != 0) im.z[pad(o.pm)] = make_float2(0.0f, 0.0f);      // bins above n / 2: not part of the one-sided transform
        }
        if (tid < NB) im.z[nyquist<LOGN>(tid)] = zh;
        __syncthreads();
        ifft_dit<LOGN>(im.z, im.tw, im.fine);
        const int64_t q0 = mb * hop - half;                  // sample index (before reflection) of the batch's first point
        const int own = per_batch(threadIdx.x);
#pragma unroll
        for (int q = 0; q < CELLS; ++q) {
            const int64_t i = s0 + own + q * THREADS;
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

int gfx_stft_band_loss_sums_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap,
                                const float* window, const float* fb, const int32_t* row_lo, const int32_t* row_hi,
                                int64_t n_bins, float* sums, int64_t R, int64_t L, int64_t n_fft, int64_t hop, float eps,
                                void* ws, size_t ws_bytes, void* stream) {
    using namespace gfx::stftloss;
    Geometry g;
    int logn;
    int64_t chunks;
    const int rc =
        check_entry(pred && target && window && fb && row_lo && row_hi && sums && n_bins >= 1 && n_bins <= n_fft / 2 + 1, pmap,
                    tmap, R, L, n_fft, hop, eps, ws, ws_bytes, g, logn, chunks);
    if (rc != GFX_OK) return rc;
    const Bands bd = {fb, row_lo, row_hi, nullptr, nullptr, (int)n_bins};
    hipStream_t s = (hipStream_t)stream;
#define GFX_LAUNCH(LOGN)                                                                                                       \
    hipLaunchKernelGGL(stft_band_loss_sums_kernel<LOGN>, dim3((unsigned)(R * chunks)), dim3(THREADS), lds_bytes(n_fft), s, pred, \
                       pmap, target, tmap, window, bd, (float4*)ws, g, (int)chunks, eps)
    GFX_STFT_LOSS_BY_SIZE(logn, GFX_LAUNCH)
#undef GFX_LAUNCH
    finish_sums(ws, sums, R, chunks, s);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_stft_band_loss_bwd_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap,
                               const float* window, const float* fb, const int32_t* row_lo, const int32_t* row_hi,
                               const int32_t* col_lo, const int32_t* col_hi, int64_t n_bins, const float* coef, float* gpred,
                               gfx_rowmap_t gmap, int64_t R, int64_t L, int64_t n_fft, int64_t hop, float eps, int accumulate,
                               void* ws, size_t ws_bytes, void* stream) {
    using namespace gfx::stftloss;
    Geometry g;
    int logn;
    int64_t chunks, segs;
    const int rc = check_entry(pred && target && window && fb && row_lo && row_hi && col_lo && col_hi && coef && gpred &&
                                   gmap.inner > 0 && n_bins >= 1 && n_bins <= n_fft / 2 + 1,
                               pmap, tmap, R, L, n_fft, hop, eps, ws, ws_bytes, g, logn, chunks, &segs);
    if (rc != GFX_OK) return rc;
    const Bands bd = {fb, row_lo, row_hi, col_lo, col_hi, (int)n_bins};
#define GFX_LAUNCH(LOGN)                                                                                                 \
    hipLaunchKernelGGL(stft_band_loss_bwd_kernel<LOGN>, dim3((unsigned)(R * segs)), dim3(THREADS), lds_bytes(n_fft),       \
                       (hipStream_t)stream, pred, pmap, target, tmap, window, bd, coef, gpred, gmap, g, (int)segs, eps, \
                       accumulate)
    GFX_STFT_LOSS_BY_SIZE(logn, GFX_LAUNCH)
#undef GFX_LAUNCH
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
