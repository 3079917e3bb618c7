// Frequency-sampled IIR (biquad cascade) -> length-N FIR, plus the coefficient front-ends.
//
// Replaces IIRFilter._process_fsm / iir_fsm / delay — core/iir.py:147-150, 263-276:
//   D[d,k] = exp(-j*phase), phase = fl32(fl32(fl32(d*k / N) * 2) * pi)      (d = 0,1,2; k = 0..N/2)
//   H[k]   = prod_i (sum_d B[i,d] D[d,k]) / (sum_d A[i,d] D[d,k])           (complex64, in cascade order)
//   h      = irfft(H, n = N)
// The phase is rounded exactly like the reference's float32 tensor arithmetic so that
// high-Q sections (denominator near zero) see the same perturbed sample points.
//
// The inverse real DFT has arbitrary length N <= 4096 (e.g. 4000 = 2^5*5^3, 4001 prime), so it
// runs as a Bluestein chirp-z transform on the 8192-point LDS FFT tile: one workgroup per
// (row, filter-channel), 2 tile FFTs each.  Everything that depends on N alone is a per-N "plan": the chirp filter's
// spectrum, the chirp itself, and the sample points D[1,k], D[2,k] (evaluated by the same device sincosf the kernel
// used to call per workgroup, so the taps are bit-identical to the table-free version; the trigonometry and the
// integer k^2 mod 2N were ~90 % of the kernel's time and most of its 120 KB of code).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "common.hpp"
#include "fft_tile.hpp"

#define NAT(arr, i) arr[(i) >> 4][brev((i) & 15, 4)]

namespace gfx {

constexpr int FSM_MAX_N = 4096;  // 2N-1 <= 8192
// plan layout, in float2 units: [0, TILE_M) chirp-filter spectrum in thread layout; [PLAN_CHIRP, +N) e^{+i pi k^2/N};
// [PLAN_D, +2*(N/2+1)) the pairs (D[1,k], D[2,k]) as one float4 per bin
constexpr int PLAN_CHIRP = TILE_M, PLAN_D = TILE_M + FSM_MAX_N, PLAN_FLOAT2 = PLAN_D + 2 * (FSM_MAX_N / 2 + 4);
static inline bool fsm_pow2(int64_t N) { return N == 8192 || N == 16384; }

// exp(+i*pi*k^2/N) (sign = +1) or exp(-i*pi*k^2/N) (sign = -1); k^2 reduced mod 2N in integers
__device__ __forceinline__ float2 chirp(int k, int N, float sign) {
    const int r = (int)(((int64_t)k * k) % (2 * (int64_t)N));
    float s, c;
    sincospif((float)r / (float)N, &s, &c);
    return make_float2(c, sign * s);
}

__device__ __forceinline__ void sample_points(int k, int N, float2& d1, float2& d2);

__global__ __launch_bounds__(TILE_T, 2) void bluestein_plan_kernel(float2* __restrict__ plan, int N,
                                                                   const float2* __restrict__ twtab) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    TileTw tw;
    tile_twiddles(tw, twtab, t);
    cx v[32], w[2][16];
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int i = t + 256 * a;
        const int m = i < N ? i : (i > TILE_M - N ? TILE_M - i : -1);  // |m|; b[m] is even in m
        v[a] = m >= 0 ? to_cx(chirp(m, N, -1.0f)) : cx{0.0f, 0.0f};
    }
    tile_forward(v, w, tw, lds, t);
#pragma unroll
    for (int q = 0; q < 32; ++q) reinterpret_cast<cx*>(plan)[q * TILE_T + t] = w[q >> 4][q & 15];
    for (int k = t; k < N; k += TILE_T) plan[PLAN_CHIRP + k] = chirp(k, N, 1.0f);
    for (int k = t; k <= N / 2; k += TILE_T) {
        float2 d1, d2;
        sample_points(k, N, d1, d2);
        reinterpret_cast<float4*>(plan + PLAN_D)[k] = make_float4(d1.x, d1.y, d2.x, d2.y);
    }
}

// complex division, scaled like torch's vectorised complex64 kernel (divide through by max(|c|,|d|))
__device__ __forceinline__ float2 cdiv(float2 n, float2 d) {
    const float sc = 1.0f / fmaxf(fabsf(d.x), fabsf(d.y));
    const float a = n.x * sc, b = n.y * sc, c = d.x * sc, e = d.y * sc;
    const float den = 1.0f / (c * c + e * e);
    return make_float2((a * c + b * e) * den, (b * c - a * e) * den);
}

// D[1,k], D[2,k] at bin k, reference arithmetic (see header)
__device__ __forceinline__ void sample_points(int k, int N, float2& d1, float2& d2) {
    const float pi32 = 3.14159274101257324219f;
    const float ph1 = ((float)k / (float)N) * 2.0f * pi32;
    const float ph2 = ((float)(2 * k) / (float)N) * 2.0f * pi32;
    float s1, c1, s2, c2;
    sincosf(ph1, &s1, &c1);
    sincosf(ph2, &s2, &c2);
    d1 = make_float2(c1, -s1);
    d2 = make_float2(c2, -s2);
}

// Coefficients given in DOUBLE precision (gfx_iir_fsm_fir_f64c_f32; the third-octave GraphicEqualizer: 31 sections, the
// lowest with poles within 1e-3 of the unit circle): the response is evaluated in double precision at the exact sample
// points exp(-2 pi i d k / N) and rounded once.  What separates the reference from a float64 evaluation of its formulas
// there (1.3e-4 .. 3.6e-4 of the output) is the float32 REPRESENTATION of the coefficients -- 1 +- beta with beta = 6.5e-4
// keeps four digits of the bandwidth -- far more than the float32 phase of the sample points or the complex64 product
// (measured, round 5: double-precision sections and exact sample points on float32 coefficients both left the mid/side
// case at 3.40e-4 against the reference's 3.30e-4, the one row of the parity table where "ours <= reference" did not
// hold).  The parity rule for a reference that is itself > 1e-5 from float64 is "at least as close to float64 as the
// reference" (SURVEY H6): with the band design carried in double precision up to here the result is the float64
// evaluation, ~1e-6.  float32 coefficients keep the reference's float32 sample points and complex64 arithmetic at every
// cascade length, which meet it at 1e-5 directly.
__device__ __forceinline__ float2 cascade_response_f64(const double* __restrict__ B, const double* __restrict__ A, int K, int k,
                                                       int N) {
    double d1y, d1x, d2y, d2x;
    sincospi(-2.0 * (double)k / (double)N, &d1y, &d1x);
    sincospi(-4.0 * (double)k / (double)N, &d2y, &d2x);
    double hr = 1.0, hi = 0.0;
    for (int i = 0; i < K; ++i) {
        const double b0 = B[3 * i], b1 = B[3 * i + 1], b2 = B[3 * i + 2];
        const double a0 = A[3 * i], a1 = A[3 * i + 1], a2 = A[3 * i + 2];
        const double nr = b0 + b1 * d1x + b2 * d2x, ni = b1 * d1y + b2 * d2y;
        const double dr = a0 + a1 * d1x + a2 * d2x, di = a1 * d1y + a2 * d2y;
        const double inv = 1.0 / (dr * dr + di * di);
        const double qr = (nr * dr + ni * di) * inv, qi = (ni * dr - nr * di) * inv;
        const double tr = hr * qr - hi * qi;
        hi = hr * qi + hi * qr;
        hr = tr;
    }
    return make_float2((float)hr, (float)hi);
}

// cascade response from the sample points (0 <= k <= N/2)
__device__ __forceinline__ float2 cascade_response(const float* __restrict__ B, const float* __restrict__ A, int K,
                                                   float2 d1, float2 d2, int k, int N, const double* __restrict__ Bd = nullptr,
                                                   const double* __restrict__ Ad = nullptr) {
    if (Bd) return cascade_response_f64(Bd, Ad, K, k, N);   // uniform
    float2 H = make_float2(1.0f, 0.0f);
    for (int i = 0; i < K; ++i) {
        const float b0 = B[3 * i], b1 = B[3 * i + 1], b2 = B[3 * i + 2];
        const float a0 = A[3 * i], a1 = A[3 * i + 1], a2 = A[3 * i + 2];
        const float2 num = make_float2((b0 + b1 * d1.x) + b2 * d2.x, (b1 * d1.y) + b2 * d2.y);
        const float2 den = make_float2((a0 + a1 * d1.x) + a2 * d2.x, (a1 * d1.y) + a2 * d2.y);
        const float2 q = cdiv(num, den);
        H = (i == 0) ? q : make_float2(fmaf(H.x, q.x, -H.y * q.y), fmaf(H.x, q.y, H.y * q.x));
    }
    return H;
}

__global__ __launch_bounds__(TILE_T, 2) void iir_fsm_kernel(const float* __restrict__ Bs, const float* __restrict__ As,
                                                            const float2* __restrict__ plan, float* __restrict__ h,
                                                            int K, int N, const float2* __restrict__ twtab,
                                                            const double* __restrict__ Bs64, const double* __restrict__ As64) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const int64_t rc = blockIdx.x;
    const float* B = Bs ? Bs + rc * K * 3 : nullptr;
    const float* A = As ? As + rc * K * 3 : nullptr;
    const double* Bd = Bs64 ? Bs64 + rc * K * 3 : nullptr;
    const double* Ad = As64 ? As64 + rc * K * 3 : nullptr;
    const int half = N / 2;
    const bool even = (N & 1) == 0;

    TileTw tw;
    tile_twiddles(tw, twtab, t);
    cx v[32], w[2][16];
    // the cascade response is evaluated once per bin of the half spectrum (k <= N/2 <= 2048) and shared
    // through LDS; the Hermitian extension a c2r transform implies is read back from there
#pragma unroll
    for (int a = 0; a < 9; ++a) {
        const int k = t + 256 * a;
        if (k <= half) {
            const float4 d = reinterpret_cast<const float4*>(plan + PLAN_D)[k];
            lds[k] = to_cx(cascade_response(B, A, K, make_float2(d.x, d.y), make_float2(d.z, d.w), k, N, Bd, Ad));
        }
    }
    __syncthreads();
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int k = t + 256 * a;
        cx e = {0.0f, 0.0f};
        if (a < 17 && k < N) {
            const bool upper = k > half;
            cx Hk = lds[upper ? N - k : k];
            if (upper) Hk.y = -Hk.y;
            if (k == 0 || (even && k == half)) Hk.y = 0.0f;
            e = cmul(Hk, to_cx(plan[PLAN_CHIRP + k]));
        }
        v[a] = e;
    }
    __syncthreads();  // the response table is dead; the tile passes reuse this LDS
    tile_forward(v, w, tw, lds, t);
#pragma unroll
    for (int q = 0; q < 32; ++q) w[q >> 4][q & 15] = cmul(w[q >> 4][q & 15], reinterpret_cast<const cx*>(plan)[q * TILE_T + t]);
    __syncthreads();
    tile_inverse(w, v, tw, lds, t);
    const float sc = 1.0f / ((float)N * (float)TILE_M);
    float* out = h + rc * N;
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int n = t + 256 * a;
        if (n < N) {
            const float2 c = plan[PLAN_CHIRP + n];
            const cx e = v[brev(a, 5)];
            out[n] = (e.x * c.x - e.y * c.y) * sc;
        }
    }
}

// Power-of-two lengths above the Bluestein limit (N = 8192, 16384: the reference's own test parametrisation,
// tests/processors/test_filter.py:27): the length-N inverse real DFT IS the tile's inverse transform.  The sampled
// response Y[k] (k = 0..N/2) is placed on every (16384 / N)-th bin of a 16384-point Hermitian spectrum -- a spectrum
// that lives only on those bins belongs to a signal of period N, whose first N samples are h scaled by N / 16384 -- and
// folded into the packed form the tile inverts:  Ye[k] = (Y[k] + conj(Y[M-k])) / 2,  Yo[k] = e^{i pi k / M} (Y[k] -
// conj(Y[M-k])) / 2,  Z'[k] = Ye + i Yo,  Z'[M-k] = conj(Ye - i Yo)  (M = 8192; fft_tile.hpp, pair_merge).
__global__ __launch_bounds__(TILE_T, 2) void iir_fsm_pow2_kernel(const float* __restrict__ Bs, const float* __restrict__ As,
                                                                 float* __restrict__ h, int K, int N,
                                                                 const float2* __restrict__ twtab,
                                                                 const double* __restrict__ Bs64,
                                                                 const double* __restrict__ As64) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const int64_t rc = blockIdx.x;
    const float* B = Bs ? Bs + rc * K * 3 : nullptr;
    const float* A = As ? As + rc * K * 3 : nullptr;
    const double* Bd = Bs64 ? Bs64 + rc * K * 3 : nullptr;
    const double* Ad = As64 ? As64 + rc * K * 3 : nullptr;
    const int stride = TILE_F / N;
    TileTw tw;
    tile_twiddles(tw, twtab, t);
    cx v[32], w[2][16];
    auto Y = [&](int bin) -> cx {   // tile bin 0..M of the 16384-point spectrum
        if (bin % stride) return cx{0.0f, 0.0f};
        const int k = bin / stride;
        float2 d1, d2;
        sample_points(k, N, d1, d2);
        cx r = to_cx(cascade_response(B, A, K, d1, d2, k, N, Bd, Ad));
        if (k == 0 || k == N / 2) r.y = 0.0f;   // a c2r transform ignores the imaginary parts of DC and Nyquist
        return r;
    };
    for_each_pair(t, tw.base(), [&](int, int ia, int ib, cx, bool self) {
        const int j = (ia >> 4) ? bf_b(t) : bf_a(t);
        const int k = j + 512 * (ia & 15);
        const cx ya = Y(k), yb = (self && k != 0) ? ya : Y(TILE_M - k);
        float sn, cs;
        sincospif((float)k / (float)TILE_M, &sn, &cs);
        const cx ye = (ya + cconj(yb)) * 0.5f;
        const cx yo = cmul((ya - cconj(yb)) * 0.5f, cx{cs, sn});
        cx za, zb;
        pair_merge(ye, yo, za, zb);
        NAT(w, ia) = za;
        if (!self) NAT(w, ib) = zb;
    });
    tile_inverse(w, v, tw, lds, t);
    const float sc = (float)stride / (float)TILE_M;
    float* out = h + rc * N;
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        const int n = 2 * (t + 256 * a);
        const cx e = v[brev(a, 5)] * sc;
        if (n + 1 < N) *reinterpret_cast<float2*>(out + n) = make_float2(e.x, e.y);
    }
}

// ---- coefficient front-ends (elementwise over rows x K) ------------------------------------------
// ParametricEqualizer: eq.py:273-314 + filter.py:593-604 (activations), 645-656 (peaking),
// 687-705 (low shelf), 736-754 (high shelf).  One thread per (row-channel, band).
__global__ void peq_coeffs_kernel(const float* __restrict__ w0, const float* __restrict__ q_inv,
                                  const float* __restrict__ log_gain, float* __restrict__ Bs, float* __restrict__ As,
                                  int64_t n, int K, int shelving) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int band = (int)(i % K);
    const float pi32 = 3.14159274101257324219f;
    const float w = pi32 * (1.0f / (1.0f + expf(-w0[i])));
    const float qi = expf(q_inv[i]);
    const float A = expf(log_gain[i]);
    float sw, cw;
    sincosf(w, &sw, &cw);
    const float alpha = sw * qi * 0.5f;
    float b0, b1, b2, a0, a1, a2;
    const bool low = shelving && band == 0, high = shelving && band == K - 1;
    if (low || high) {
        const float sg = low ? 1.0f : -1.0f;
        const float ap1 = A + 1.0f, am1 = A - 1.0f;
        const float ap1c = ap1 * cw, am1c = am1 * cw;
        const float s = 2.0f * sqrtf(A) * alpha;
        b0 = A * ((ap1 - sg * am1c) + s);
        b1 = sg * 2.0f * A * (am1 - sg * ap1c);
        b2 = A * ((ap1 - sg * am1c) - s);
        a0 = (ap1 + sg * am1c) + s;
        a1 = -sg * 2.0f * (am1 + sg * ap1c);
        a2 = (ap1 + sg * am1c) - s;
    } else {
        const float aA = alpha * A, adA = alpha / A;
        b0 = 1.0f + aA;
        b1 = -2.0f * cw;
        b2 = 1.0f - aA;
        a0 = 1.0f + adA;
        a1 = b1;
        a2 = 1.0f - adA;
    }
    Bs[3 * i] = b0;
    Bs[3 * i + 1] = b1;
    Bs[3 * i + 2] = b2;
    As[3 * i] = a0;
    As[3 * i + 1] = a1;
    As[3 * i + 2] = a2;
}

// Backward of peq_coeffs_kernel: (gBs, gAs) -> (g w0, g q_inv, g log_gain), one thread per (row-channel, band).
// Partials with respect to the intermediates (A, cos w, alpha, s = 2 sqrt(A) alpha), then the activations' chain rule:
//   A = exp(log_gain), alpha = sin(w) exp(q_inv) / 2, w = pi sigmoid(w0).
__global__ void peq_coeffs_bwd_kernel(const float* __restrict__ w0, const float* __restrict__ q_inv,
                                      const float* __restrict__ log_gain, const float* __restrict__ gBs,
                                      const float* __restrict__ gAs, float* __restrict__ gw0, float* __restrict__ gq,
                                      float* __restrict__ glg, int64_t n, int K, int shelving) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n * K) return;
    const int band = (int)(i % K);
    const float pi32 = 3.14159274101257324219f;
    const float sig = 1.0f / (1.0f + expf(-w0[i]));
    const float w = pi32 * sig;
    const float qi = expf(q_inv[i]);
    const float A = expf(log_gain[i]);
    float sw, cw;
    sincosf(w, &sw, &cw);
    const float alpha = sw * qi * 0.5f;
    const float gb0 = gBs[3 * i], gb1 = gBs[3 * i + 1], gb2 = gBs[3 * i + 2];
    const float ga0 = gAs[3 * i], ga1 = gAs[3 * i + 1], ga2 = gAs[3 * i + 2];
    float dA, dcw, dal;  // dL/dA, dL/dcos(w), dL/dalpha
    const bool low = shelving && band == 0, high = shelving && band == K - 1;
    if (low || high) {
        const float sg = low ? 1.0f : -1.0f;
        const float ap1 = A + 1.0f, am1 = A - 1.0f, rA = sqrtf(A);
        const float s = 2.0f * rA * alpha;
        const float e = ap1 - sg * am1 * cw;   // shared term of b0, b2
        const float ds = A * (gb0 - gb2) + (ga0 - ga2);                    // dL/ds
        dA = gb0 * ((e + s) + A * (1.0f - sg * cw)) + gb1 * sg * 2.0f * ((am1 - sg * ap1 * cw) + A * (1.0f - sg * cw)) +
             gb2 * ((e - s) + A * (1.0f - sg * cw)) + (ga0 + ga2) * (1.0f + sg * cw) - ga1 * sg * 2.0f * (1.0f + sg * cw) +
             ds * alpha / rA;
        dcw = -(gb0 + gb2) * A * sg * am1 - gb1 * 2.0f * A * ap1 + (ga0 + ga2) * sg * am1 - ga1 * 2.0f * ap1;
        dal = ds * 2.0f * rA;
    } else {
        dA = alpha * (gb0 - gb2) - alpha / (A * A) * (ga0 - ga2);
        dcw = -2.0f * (gb1 + ga1);
        dal = A * (gb0 - gb2) + (ga0 - ga2) / A;
    }
    glg[i] = dA * A;
    gq[i] = dal * alpha;
    gw0[i] = (-dcw * sw + dal * cw * qi * 0.5f) * pi32 * sig * (1.0f - sig);
}

// BiquadFilter: filter.py:144-153.
__global__ void biquad_coeffs_kernel(const float* __restrict__ Bin, const float* __restrict__ A1_pre,
                                     const float* __restrict__ A2_pre, const float* __restrict__ A0,
                                     float* __restrict__ Bs, float* __restrict__ As, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float a1 = 2.0f * tanhf(A1_pre[i]);
    const float a1a = fabsf(a1);
    const float a2 = ((2.0f - a1a) * tanhf(A2_pre[i]) + a1a) / 2.0f;
    const float g = A0 ? A0[i] : 1.0f;
    As[3 * i] = g;
    As[3 * i + 1] = a1 * g;
    As[3 * i + 2] = a2 * g;
    Bs[3 * i] = Bin[3 * i] + 1.0f;
    Bs[3 * i + 1] = Bin[3 * i + 1];
    Bs[3 * i + 2] = Bin[3 * i + 2];
}

}  // namespace gfx

using namespace gfx;


namespace gfx {
// ---- gradient of the frequency-sampled taps with respect to the biquad coefficients (training path) -------------------
// h = irfft(resp, n = N), resp = prod_i num_i / den_i, num_i = sum_d B[i, d] D_d, D_d[k] = e^(-j phi[d, k]) (core/iir.py:
// 147-152, 263-276); autograd through it is
//     dL/dB[i, d] =  Re sum_k T_k D_d[k] / num_i[k],     dL/dA[i, d] = -Re sum_k T_k D_d[k] / den_i[k],
//     T_k = conj(G_k) w_k resp_k,   G = rfft(dL/dh),  w = (1, 2, ..., 2, [1 at N / 2]) / N
// (T / num_i formed as conj(G) w prod_{j != i}(num_j / den_j) / den_i: num_i may be zero at a bin)
// -- the sums over the bins cancel to a few 1e-5 of their terms, so everything here is double (as the torch form of rounds
// 4-5 was: ~40 complex128 kernels per equaliser stage and step; this is one).  One workgroup per (filter row, section i):
// every thread recomputes the response of its bins (K complex divisions) and keeps six sums.  `delays`: the (3, F)
// complex64 table of the forward pass, float32 phases as upstream forms them.
__global__ __launch_bounds__(256) void iir_fsm_bwd_kernel(const float* __restrict__ Bs, const float* __restrict__ As,
                                                          const float2* __restrict__ G, const float2* __restrict__ delays,
                                                          float* __restrict__ gB, float* __restrict__ gA, int K, int N,
                                                          int wantB, int wantA) {
    __shared__ double red[6][4];
    const int64_t rc = blockIdx.x;
    const int sec = blockIdx.y;
    const int F = N / 2 + 1;
    const float* B = Bs + rc * K * 3;
    const float* A = As + rc * K * 3;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < F; k += blockDim.x) {
        double2 D[3];
#pragma unroll
        for (int d = 0; d < 3; ++d) D[d] = make_double2((double)delays[d * F + k].x, (double)delays[d * F + k].y);
        double2 resp = make_double2(1.0, 0.0), mynum = resp, myden = resp, others = resp;   // others = prod_{j != sec} num_j / den_j
        for (int i = 0; i < K; ++i) {
            double2 num = make_double2(0.0, 0.0), den = num;
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                num.x += (double)B[i * 3 + d] * D[d].x; num.y += (double)B[i * 3 + d] * D[d].y;
                den.x += (double)A[i * 3 + d] * D[d].x; den.y += (double)A[i * 3 + d] * D[d].y;
            }
            const double dd = den.x * den.x + den.y * den.y;
            const double2 q = make_double2((num.x * den.x + num.y * den.y) / dd, (num.y * den.x - num.x * den.y) / dd);
            resp = make_double2(resp.x * q.x - resp.y * q.y, resp.x * q.y + resp.y * q.x);
            if (i == sec) { mynum = num; myden = den; }
            else others = make_double2(others.x * q.x - others.y * q.y, others.x * q.y + others.y * q.x);
        }
        const double w = ((k == 0 || (!(N & 1) && k == N / 2)) ? 1.0 : 2.0) / (double)N;
        const float2 g = G[rc * F + k];
        // T = conj(G) w resp
        const double2 T = make_double2(w * ((double)g.x * resp.x + (double)g.y * resp.y), w * ((double)g.x * resp.y - (double)g.y * resp.x));
        // T / num_sec = conj(G) w others / den_sec: never divided by the numerator, which is exactly zero at a sampled bin
        // for a section with a zero on the unit circle there (high-pass at k = 0, low-pass at N / 2, band-pass at both)
        const double2 U = make_double2(w * ((double)g.x * others.x + (double)g.y * others.y), w * ((double)g.x * others.y - (double)g.y * others.x));
        const double dn = myden.x * myden.x + myden.y * myden.y;
        const double2 tn = make_double2((U.x * myden.x + U.y * myden.y) / dn, (U.y * myden.x - U.x * myden.y) / dn);   // T / num
        const double2 td = make_double2((T.x * myden.x + T.y * myden.y) / dn, (T.y * myden.x - T.x * myden.y) / dn);   // T / den
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            acc[d] += tn.x * D[d].x - tn.y * D[d].y;          // Re((T / num) D_d)
            acc[3 + d] -= td.x * D[d].x - td.y * D[d].y;      // -Re((T / den) D_d)
        }
    }
#pragma unroll
    for (int v = 0; v < 6; ++v) {
        double x = acc[v];
        for (int o = 32; o > 0; o >>= 1) x += __shfl_down(x, o, 64);
        if ((threadIdx.x & 63) == 0) red[v][threadIdx.x >> 6] = x;
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        const double x = red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3];
        const int64_t o = (rc * K + sec) * 3;
        if (threadIdx.x < 3) { if (wantB) gB[o + threadIdx.x] = (float)x; }
        else if (wantA) gA[o + threadIdx.x - 3] = (float)x;
    }
}
}  // namespace gfx

extern "C" {

int gfx_iir_fsm_native(int64_t N) { return (N >= 1 && N <= FSM_MAX_N) || fsm_pow2(N); }
size_t gfx_iir_fsm_plan_bytes(int64_t N) { return (N < 1 || N > FSM_MAX_N) ? 0 : (size_t)PLAN_FLOAT2 * sizeof(float2); }

int gfx_iir_fsm_plan_f32(void* plan, int64_t N, void* stream) {
    if (!plan || N < 1 || N > FSM_MAX_N) return GFX_EINVAL;
    if (allow_lds(bluestein_plan_kernel, TILE_LDS_BYTES)) return GFX_ELAUNCH;
    const float2* tw = tile_twiddle_table((hipStream_t)stream);
    if (!tw) return GFX_ELAUNCH;
    hipLaunchKernelGGL(bluestein_plan_kernel, dim3(1), dim3(TILE_T), TILE_LDS_BYTES, (hipStream_t)stream,
                       (float2*)plan, (int)N, tw);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

static int iir_fsm_fir_launch(const float* Bs, const float* As, const double* Bs64, const double* As64, const void* plan,
                              float* h, int64_t RC, int64_t K, int64_t N, void* stream) {
    if (!h || RC <= 0 || K <= 0 || N < 1 || RC > 0x7fffffffLL) return GFX_EINVAL;
    if (fsm_pow2(N)) {  // no plan needed
        if (allow_lds(iir_fsm_pow2_kernel, TILE_LDS_BYTES)) return GFX_ELAUNCH;
        const float2* tw2 = tile_twiddle_table((hipStream_t)stream);
        if (!tw2) return GFX_ELAUNCH;
        hipLaunchKernelGGL(iir_fsm_pow2_kernel, dim3((unsigned)RC), dim3(TILE_T), TILE_LDS_BYTES, (hipStream_t)stream, Bs,
                           As, h, (int)K, (int)N, tw2, Bs64, As64);
        return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
    }
    if (!plan || N > FSM_MAX_N) return GFX_EINVAL;
    if (allow_lds(iir_fsm_kernel, TILE_LDS_BYTES)) return GFX_ELAUNCH;
    const float2* tw = tile_twiddle_table((hipStream_t)stream);
    if (!tw) return GFX_ELAUNCH;
    hipLaunchKernelGGL(iir_fsm_kernel, dim3((unsigned)RC), dim3(TILE_T), TILE_LDS_BYTES, (hipStream_t)stream, Bs, As,
                       (const float2*)plan, h, (int)K, (int)N, tw, Bs64, As64);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_iir_fsm_fir_f32(const float* Bs, const float* As, const void* plan, float* h, int64_t RC, int64_t K,
                        int64_t N, void* stream) {
    if (!Bs || !As) return GFX_EINVAL;
    return iir_fsm_fir_launch(Bs, As, nullptr, nullptr, plan, h, RC, K, N, stream);
}

int gfx_iir_fsm_fir_f64c_f32(const double* Bs, const double* As, const void* plan, float* h, int64_t RC, int64_t K,
                             int64_t N, void* stream) {
    if (!Bs || !As) return GFX_EINVAL;
    return iir_fsm_fir_launch(nullptr, nullptr, Bs, As, plan, h, RC, K, N, stream);
}

int gfx_peq_coeffs_f32(const float* w0, const float* q_inv, const float* log_gain, float* Bs, float* As, int64_t n,
                       int64_t K, int use_shelving, void* stream) {
    if (!w0 || !q_inv || !log_gain || !Bs || !As || n <= 0 || K <= 0) return GFX_EINVAL;
    const int64_t total = n * K;
    hipLaunchKernelGGL(peq_coeffs_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w0,
                       q_inv, log_gain, Bs, As, n, (int)K, use_shelving);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_peq_coeffs_bwd_f32(const float* w0, const float* q_inv, const float* log_gain, const float* gBs, const float* gAs,
                           float* gw0, float* gq_inv, float* glog_gain, int64_t n, int64_t K, int use_shelving,
                           void* stream) {
    if (!w0 || !q_inv || !log_gain || !gBs || !gAs || !gw0 || !gq_inv || !glog_gain || n <= 0 || K <= 0) return GFX_EINVAL;
    const int64_t total = n * K;
    hipLaunchKernelGGL(peq_coeffs_bwd_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, w0,
                       q_inv, log_gain, gBs, gAs, gw0, gq_inv, glog_gain, n, (int)K, use_shelving);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_biquad_coeffs_f32(const float* Bin, const float* A1_pre, const float* A2_pre, const float* A0, float* Bs,
                          float* As, int64_t n, void* stream) {
    if (!Bin || !A1_pre || !A2_pre || !Bs || !As || n <= 0) return GFX_EINVAL;
    hipLaunchKernelGGL(biquad_coeffs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, Bin,
                       A1_pre, A2_pre, A0, Bs, As, n);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

int gfx_iir_fsm_bwd_f32(const float* Bs, const float* As, const float* G, const float* delays, float* gB, float* gA,
                        int64_t RC, int64_t K, int64_t N, void* stream) {
    if (!Bs || !As || !G || !delays || (!gB && !gA) || RC <= 0 || RC > 0x7fffffffLL || K < 1 || K > 65535 || N < 1 ||
        N > 0x3fffffffLL)
        return GFX_EINVAL;
    hipLaunchKernelGGL(iir_fsm_bwd_kernel, dim3((unsigned)RC, (unsigned)K), dim3(256), 0, (hipStream_t)stream, Bs, As,
                       (const float2*)G, (const float2*)delays, gB, gA, (int)K, (int)N, gB ? 1 : 0, gA ? 1 : 0);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
