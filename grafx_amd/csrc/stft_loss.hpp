// The frame transform of the STFT loss (stft_loss.hip, which describes it) and what its kernels share with the banded
// loss of stft_band_loss.hip: the LDS image, the sample ring, the radix-2 passes, the per-bin formulas, the geometry, and on
// the host the argument check of the four entries and the launch of the one finish kernel.
#pragma once
#include "common.hpp"

namespace gfx {
namespace stftloss {

constexpr int THREADS = 256;
constexpr int SLOTS = 2048;                 // complex points of the transform buffer
constexpr int RUN = 8;                      // batches of SLOTS / n_fft frames per forward workgroup
constexpr int SEG = 4096;                   // gradient samples one backward workgroup owns,
constexpr int CELLS = SEG / THREADS;        // this many per thread, in registers

__device__ __forceinline__ int64_t lo(int64_t a, int64_t b) { return a < b ? a : b; }
__device__ __forceinline__ int64_t hi(int64_t a, int64_t b) { return a > b ? a : b; }

// (gfx::row_off64 with c = 0 changed the code of every kernel here by an instruction or two)
__device__ __forceinline__ int64_t sig_row_off(const gfx_rowmap_t& m, int64_t r) {
    return (r / m.inner) * m.stride_outer + (r % m.inner) * m.stride_inner;
}

// Where point i of the transform buffer lives: one float2 of padding after every 32, so that the eight consecutive points a
// thread owns in the pass over the lowest bits (64 bytes apart from lane to lane) spread over all banks.
__device__ __forceinline__ constexpr int pad(int i) { return i + (i >> 5); }
constexpr int ZSIZE = SLOTS + SLOTS / 32;

constexpr int RING = 2048;                   // staged samples per signal: a batch spans (NB - 1) * hop + N <= RING positions

struct Geometry {                            // what is not fixed by n_fft
    int hop;
    int64_t L, frames;
};

template <int LOGN>
struct Size {
    static constexpr int N = 1 << LOGN, HALF = N / 2, NB = SLOTS / N;     // NB frames per batch
};

// Stages whose pairs are less than 2^FINE apart read their twiddles from per-stage tables (stage b: 2^b entries at offset
// 2^b - 1, 2^FINE - 1 in all): in the one table of n / 2 they are 2^(logn - 1 - b) entries apart and the lanes of a wave
// would meet on one bank, up to 32 of them.
constexpr int FINE = 8;

struct Image {                               // the carve of the dynamic LDS region
    float2* z;
    float2* tw;
    float2* fine;
    float* win;
    float* sp;
    float* st;
    float* red;
};

template <int LOGN>
__device__ __forceinline__ Image carve(char* base) {
    Image im;
    im.z = reinterpret_cast<float2*>(base);
    im.tw = im.z + ZSIZE;
    im.fine = im.tw + Size<LOGN>::HALF;
    im.win = reinterpret_cast<float*>(im.fine + (1 << FINE));
    im.sp = im.win + Size<LOGN>::N;
    im.st = im.sp + RING;
    im.red = im.st + RING;
    return im;
}

template <int LOGN>
__device__ __forceinline__ void build_tables(const Image& im, const float* __restrict__ window) {
    constexpr int N = Size<LOGN>::N;
    for (int j = threadIdx.x; j < N / 2; j += THREADS) {
        double s, c;
        sincospi(2.0 * (double)j / (double)N, &s, &c);
        im.tw[j] = make_float2((float)c, (float)-s);
    }
    for (int i = threadIdx.x; i < (1 << FINE) - 1; i += THREADS) {
        const int b = 31 - __clz(i + 1), j = i + 1 - (1 << b);            // e^{-2 pi i j / 2^(b + 1)}
        double s, c;
        sincospi((double)j / (double)(1 << b), &s, &c);
        im.fine[i] = make_float2((float)c, (float)-s);
    }
    for (int j = threadIdx.x; j < N; j += THREADS) im.win[j] = window[j];
}

// The staged samples are a ring over the padded positions (position q in slot q mod RING; sample u = q - n / 2, reflected
// at both ends): consecutive batches of a workgroup overlap, so only the positions a batch adds are read from memory --
// fetched into registers once the batch before has left the ring, and committed to it before that batch's successor is
// filled (the forward holds them through the transform, the backward commits them before it).
// (`tid` of fetch, commit and fill is the thread's index: the plain kernels pass nothing, the banded backward passes it as a
// value taken anew in every batch, per_batch() of stft_band_loss.hip, so that the positions below are not all held in
// registers from before its loop.)
struct Fetch {
    float p[RING / THREADS], t[RING / THREADS];
};

template <int LOGN>
__device__ __forceinline__ void fetch(Fetch& r, const float* __restrict__ p, const float* __restrict__ t, int64_t q, int count,
                                      int64_t L, int tid = threadIdx.x) {
    constexpr int HALF = Size<LOGN>::HALF;
#pragma unroll
    for (int i = 0; i < RING / THREADS; ++i) {
        const int o = tid + i * THREADS;
        int64_t u = q + o - HALF;
        float a = 0.0f, b = 0.0f;
        if (o < count && u < L + HALF) {                     // (beyond the padding: frames that do not exist)
            if (u < 0) u = -u;
            if (u >= L) u = 2 * (L - 1) - u;
            a = p[u];
            b = t[u];
        }
        r.p[i] = a;
        r.t[i] = b;
    }
}

__device__ __forceinline__ void commit(const Image& im, const Fetch& r, int64_t q, int count, int tid = threadIdx.x) {
    const int q0 = (int)(q & (RING - 1));
#pragma unroll
    for (int i = 0; i < RING / THREADS; ++i) {
        const int o = tid + i * THREADS;
        if (o < count) {
            im.sp[(q0 + o) & (RING - 1)] = r.p[i];
            im.st[(q0 + o) & (RING - 1)] = r.t[i];
        }
    }
}

// Fill the transform buffer with the windowed frames of the batch that starts at frame mb; frames past the last one are
// zero.  Returns whether any pred sample this thread read differs from its target sample.  No barrier.
template <int LOGN>
__device__ __forceinline__ int fill(const Image& im, int64_t mb, const Geometry& g, int tid = threadIdx.x) {
    constexpr int N = Size<LOGN>::N;
    const int q0 = (int)((mb * g.hop) & (RING - 1));
    const int valid = (int)lo(Size<LOGN>::NB, g.frames - mb);
    int differ = 0;
#pragma unroll
    for (int q = 0; q < SLOTS / THREADS; ++q) {
        const int idx = tid + q * THREADS;
        const int f = idx >> LOGN, j = idx & (N - 1);
        float2 v = make_float2(0.0f, 0.0f);
        if (f < valid) {
            const int slot = (q0 + f * g.hop + j) & (RING - 1);
            const float a = im.sp[slot], b = im.st[slot], w = im.win[j];
            differ |= !(a == b);
            v = make_float2(w * a, w * b);
        }
        im.z[pad(idx)] = v;
    }
    return differ;
}

// One pass over the buffer: thread t owns the 8 points whose index differs in bits [LO, LO + 3) and runs the radix-2
// butterflies of index bits LO + FIRST .. LO + LAST in registers (decimation in frequency takes the bits downwards and
// multiplies after the difference; the inverse, decimation in time, takes them upwards with conjugate twiddles before
// the sum).  The frames of the buffer lie above bit LOGN and are never paired.  No barrier.
template <bool INVERSE, int LOGN, int LO, int FIRST, int LAST>
__device__ __forceinline__ void pass8(float2* z, const float2* tw, const float2* fine) {
    const int tlow = threadIdx.x & ((1 << LO) - 1);
    const int base = ((threadIdx.x >> LO) << (LO + 3)) | tlow;
    float2 v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = z[pad(base | (e << LO))];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int bit = INVERSE ? s : 2 - s;
        if (bit < FIRST || bit > LAST) continue;
        const int b = LO + bit;                              // the index bit of this stage: pairs 2^b apart
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            if (e & (1 << bit)) continue;
            const int jl = e & ((1 << bit) - 1);             // (with LO = 0 the twiddle index is this constant)
            float2 w;
            if (b == 0) w = make_float2(1.0f, 0.0f);
            else if (b == 1 && LO == 0) w = jl ? make_float2(0.0f, -1.0f) : make_float2(1.0f, 0.0f);
            else if (b < FINE && b < LOGN - 1) w = fine[(1 << b) - 1 + ((jl << LO) | tlow)];
            else w = tw[((jl << LO) | tlow) << (LOGN - 1 - b)];
            const float2 a = v[e], c = v[e | (1 << bit)];
            if (INVERSE) {
                const float cx = c.x * w.x + c.y * w.y, cy = c.y * w.x - c.x * w.y;      // c * conj(w)
                v[e] = make_float2(a.x + cx, a.y + cy);
                v[e | (1 << bit)] = make_float2(a.x - cx, a.y - cy);
            } else {
                const float dx = a.x - c.x, dy = a.y - c.y;
                v[e] = make_float2(a.x + c.x, a.y + c.y);
                v[e | (1 << bit)] = make_float2(dx * w.x - dy * w.y, dx * w.y + dy * w.x);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) z[pad(base | (e << LO))] = v[e];
}

// natural order in, bit-reversed order out, every frame of the buffer at once; ends with a barrier
template <int LOGN, int TOP = LOGN - 1>
__device__ __forceinline__ void fft_dif(float2* z, const float2* tw, const float2* fine) {
    if constexpr (TOP >= 0) {
        constexpr int LO = TOP >= 2 ? TOP - 2 : 0;
        pass8<false, LOGN, LO, 0, TOP - LO>(z, tw, fine);
        __syncthreads();
        fft_dif<LOGN, LO - 1>(z, tw, fine);
    }
}

// the unnormalised inverse (e^{+...}): bit-reversed order in, natural order out; ends with a barrier
template <int LOGN, int DONE = 0>
__device__ __forceinline__ void ifft_dit(float2* z, const float2* tw, const float2* fine) {
    if constexpr (DONE < LOGN) {
        constexpr int LO = DONE <= LOGN - 3 ? DONE : LOGN - 3;
        pass8<true, LOGN, LO, DONE - LO, 2>(z, tw, fine);
        __syncthreads();
        ifft_dit<LOGN, LO + 3>(z, tw, fine);
    }
}

// The bins thread-slot b of the buffer owns: k = bitrev(2 c) < n / 2 of frame f at position pk = 2 c, and its mirror n - k
// at pm.  c = 0 is k = 0 and owns k = n / 2 (position 1) too; both mirror themselves.
struct Bins {
    int f, k, pk, pm;
};

template <int LOGN>
__device__ __forceinline__ Bins bins_of(int b) {
    constexpr int N = Size<LOGN>::N;
    Bins s;
    s.f = b >> (LOGN - 1);
    const int c = b & (N / 2 - 1);
    const int base = s.f << LOGN;
    s.k = (int)(__brev((unsigned)(2 * c)) >> (32 - LOGN));
    s.pk = base + 2 * c;
    s.pm = base + (int)(__brev((unsigned)((N - s.k) & (N - 1))) >> (32 - LOGN));
    return s;
}

__device__ __forceinline__ void split(const float2 zk, const float2 zm, float2& P, float2& T) {
    P = make_float2(0.5f * (zk.x + zm.x), 0.5f * (zk.y - zm.y));
    T = make_float2(0.5f * (zk.y + zm.y), 0.5f * (zm.x - zk.x));
}

struct Sums {
    float A, B, E, D;
};

// (the hardware's square root, reciprocal and logarithm, one unit in the last place each: the sums are held to 1e-5)
__device__ __forceinline__ void add_bin(Sums& s, float2 P, float2 T, float eps, bool same) {
    const float t2 = fmaxf(T.x * T.x + T.y * T.y, eps);
    s.B += t2;
    if (same) return;
    const float p2 = fmaxf(P.x * P.x + P.y * P.y, eps);
    const float d = __builtin_amdgcn_sqrtf(t2) - __builtin_amdgcn_sqrtf(p2);
    s.A += d * d;
    s.E += fabsf(d);
    s.D += 0.5f * fabsf(__logf(t2 * __builtin_amdgcn_rcpf(p2)));      // |log|T| - log|P||
}

// G = live * (2 cA (|P| - |T|) + cE sign(|P| - |T|) + cD sign(log|P| - log|T|) / |P|) * P / |P|
__device__ __forceinline__ float2 bin_grad(float2 P, float2 T, float eps, float cA, float cE, float cD) {
    const float p2 = P.x * P.x + P.y * P.y;
    if (!(p2 > eps)) return make_float2(0.0f, 0.0f);
    const float ip = __builtin_amdgcn_rsqf(p2);              // 1 / |P|
    const float d = p2 * ip - __builtin_amdgcn_sqrtf(fmaxf(T.x * T.x + T.y * T.y, eps));
    const float sg = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);
    const float s = (2.0f * cA * d + sg * (cE + cD * ip)) * ip;
    return make_float2(s * P.x, s * P.y);
}

static inline bool geometry(Geometry& g, int& logn, int64_t L, int64_t n_fft, int64_t hop) {
    if (n_fft < 128 || n_fft > 2048 || (n_fft & (n_fft - 1)) || hop < 1 || hop > n_fft || L <= n_fft / 2 ||
        L > 0x7fffffffLL - 4096)
        return false;
    logn = __builtin_ctz((unsigned)n_fft);
    g.hop = (int)hop;
    g.L = L;
    g.frames = 1 + L / hop;
    return true;
}

static inline int64_t chunks_of(const Geometry& g, int64_t n_fft) {
    const int64_t per = (int64_t)RUN * (SLOTS / n_fft);
    return (g.frames + per - 1) / per;
}

// What the four entries of the two losses check alike, and the codes they answer in their order.  `own`: the entry's own
// pointers, row map and band count are in order.  `segs`: the backward's count of segments per row (its grid is limited as
// well); nullptr for the sums, whose float4 partials need an aligned workspace.  Sets g, logn, chunks and *segs.
static inline int check_entry(bool own, const gfx_rowmap_t& pmap, const gfx_rowmap_t& tmap, int64_t R, int64_t L,
                              int64_t n_fft, int64_t hop, float eps, const void* ws, size_t ws_bytes, Geometry& g, int& logn,
                              int64_t& chunks, int64_t* segs = nullptr) {
    if (!own || !ws || R <= 0 || !(eps > 0.0f) || pmap.inner <= 0 || tmap.inner <= 0 || !geometry(g, logn, L, n_fft, hop))
        return GFX_EINVAL;
    chunks = chunks_of(g, n_fft);
    if (segs) *segs = (L + SEG - 1) / SEG;
    if (R > 0x7fffffffLL / chunks || (segs ? R > 0x7fffffffLL / *segs : ((uintptr_t)ws & 15) != 0)) return GFX_EINVAL;
    if (ws_bytes < (size_t)R * (size_t)chunks * 16) return GFX_ENOSPC;      // one buffer serves both calls of a step
    return GFX_OK;
}

// launches stft_loss_finish_kernel (stft_loss.hip): a row's partials summed in their order, in double
void finish_sums(const void* partials, float* sums, int64_t R, int64_t chunks, hipStream_t stream);

static inline size_t lds_bytes(int64_t n_fft) {
    return (size_t)ZSIZE * sizeof(float2) + (size_t)(n_fft / 2 + (1 << FINE)) * sizeof(float2) + (size_t)n_fft * sizeof(float) +
           2 * (size_t)RING * sizeof(float) + 64;
}

// the kernel compiled for n_fft = 2^logn
#define GFX_STFT_LOSS_BY_SIZE(logn, launch) \
    switch (logn) {                         \
        case 7: launch(7); break;           \
        case 8: launch(8); break;           \
        case 9: launch(9); break;           \
        case 10: launch(10); break;         \
        default: launch(11); break;         \
    }

}  // namespace stftloss
}  // namespace gfx
