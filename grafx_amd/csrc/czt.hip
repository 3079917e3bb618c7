// The reference's odd-length aliasing, y = irfft_{P-1}(rfft_P(z)), as two chirp-z transforms on the LDS FFT tile.
//
// convolve() (core/convolution.py:119-134) pads to P = Lx + Lh - 1, multiplies rffts and calls irfft WITHOUT n, i.e.
// with length 2 (P // 2).  For odd P that inverts a P-point spectrum on a (P-1)-point grid -- a global resampling of the
// linear convolution z.  Every reference default (4000 / 16384 / 60000 taps with even
// audio lengths) takes that path, so reproducing it is part of parity.  P is arbitrary (131072 + 4000 - 1 = 135071 is
// not even composite-friendly), hence Bluestein:
//
//   Z[k] = cP[k]  sum_m (z[m] cP[m]) bP[k - m],   cP[k] = e^{-i pi k^2 / P},  bP[j] = e^{+i pi j^2 / P},  k < K = (P+1)/2
//   y[n] = Re( cQ[n] sum_k (w_k Z[k] cQ[k]) bQ[n - k] ) / Q,   cQ[k] = e^{+i pi k^2 / Q},  bQ[j] = e^{-i pi j^2 / Q},
//          Q = P - 1,  w_0 = w_{K-1} = 1, else 2   (taking the real part drops Im Z[0], Im Z[K-1] like a c2r transform)
//
// two circular convolutions of NFFT = C x 8192 >= (3P - 1) / 2 points (C = the smallest count of tiles with prime factors
// up to 7 that covers them: 25 for P = 135 071, where the next power of two is 32), each a "four-step" FFT around the tile:
//   cols_fwd : per column n2 (of 8192) a C-point DFT over n1 (registers) and the twiddle W_NFFT^(n2 k1)
//   rows     : per row k1 one tile: forward, multiply by the chirp's spectrum (thread layout, precomputed), inverse
//   cols_inv : conjugate twiddle, C-point inverse DFT, then the chirp / weights of the next step
// all in place on one NFFT-point complex buffer per signal row.  fp32 throughout; the chirps are evaluated once per P
// in double with the phase reduced exactly (k^2 mod 2P in integers).  C <= 32 covers P <= 174,763; beyond, up to three
// OUTER radix-4 levels split the transform into 4 / 16 / 64 sub-transforms of C x 8192 points (czt_outer_*: 4-point DFT
// over the quarters + twiddle W_N^(n' k3), in place, applied recursively): NFFT <= 2^24, P <= 11,184,811 (233 s of audio at
// 48 kHz plus the filter).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>

#include "czt_core.hpp"

namespace gfx {

template <typename T>
__global__ void czt_chirp_table_kernel(typename Prec<T>::T2* __restrict__ tab, int64_t n, int64_t den, float sign) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tab[i] = chirp_d<T>(i, den, sign);
}

// MODE 0: real rows, z[row, i - lo] tab[i] for lo <= i < lo + len (row stride ldz), zero elsewhere;  MODE 1: the complex
// buffer itself;  MODE 2: a chirp sequence (plan building)
template <typename T, int C, int MODE>
__global__ __launch_bounds__(256) void czt_cols_fwd_kernel(const float* __restrict__ z,
                                                          const typename Prec<T>::T2* __restrict__ tab,
                                                          typename Prec<T>::T2* __restrict__ buf, CztGeom g, int64_t ldz,
                                                          int64_t lo, int64_t len, ChirpSeq cs) {
    using cx = typename Prec<T>::cxt;
    const int n2 = blockIdx.x * 256 + threadIdx.x;          // column 0..8191
    const int64_t row = blockIdx.y;                        // signal row * S + sub-transform
    const int64_t NS = g.NFFT / g.S;                       // points of one sub-transform
    typename Prec<T>::T2* b = buf + row * NS;
    const ColBuf<T> cb(b, NS);
    cx v[C];
#pragma unroll
    for (int n1 = 0; n1 < C; ++n1) {
        const int64_t i = (int64_t)n1 * TILE_M + n2;
        cx e = {0, 0};
        if (MODE == 0) {
            if (i >= lo && i < lo + len) e = to_cx(tab[i]) * (T)z[row * ldz + (i - lo)];
        } else if (MODE == 1) {
            e = cb.ld(n1, n2);
        } else {
            if (i <= cs.hi) e = to_cx(chirp_d<T>(i, cs.den, cs.sign));
            else if (i >= g.NFFT - cs.lo) e = to_cx(chirp_d<T>(g.NFFT - i, cs.den, cs.sign));
        }
        v[n1] = e;
    }
    col_dft<C, false>(v);
    ColTw<T, C> tw(n2, (int)NS, false);
#pragma unroll
    for (int k1 = 0; k1 < C; ++k1) col_out<T, C>(cb, tw, k1, n2, v[spos(C, k1)]);
}

// One tile per (row, k1): forward, times the chirp spectrum, inverse -- in place.  PLAN: forward only, spectrum stored
// in thread layout.
// float: the twiddles live through the tile, the spectrum is loaded up front and the tile goes through a descriptor (10.1
// -> 9.3 ms per 4096 rows).  double: the split tile (fft_tile_f64.hpp: exchanges in two rounds, twiddles fetched per pass),
// the spectrum eight values at a time and global accesses to the tile (measured 1 % better than the descriptor form).
template <typename T, bool PLAN>
__global__ __launch_bounds__(TILE_T, 2) void czt_rows_kernel(
    typename Prec<T>::T2* __restrict__ buf, const typename Prec<T>::T2* __restrict__ spec,
    typename Prec<T>::T2* __restrict__ spec_out, int C, const typename Prec<T>::T2* __restrict__ twtab) {
    using cx = typename Prec<T>::cxt;
    constexpr bool F32 = sizeof(T) == 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    cx* lds = reinterpret_cast<cx*>(lds_raw);
    const int t = threadIdx.x;
    const int64_t tile = blockIdx.x;                    // row * C + k1
    const int k1 = (int)(tile % C);                       // C here = tiles per signal row = S * C
    constexpr uint32_t TILE_BYTES = TILE_M * sizeof(cx);
    const __amdgpu_buffer_rsrc_t rb = tile_rsrc(reinterpret_cast<cx*>(buf) + tile * TILE_M, TILE_BYTES);
    TileTw tw;
    if constexpr (F32) tile_twiddles(tw, twtab, t);
    cx v[32], w[2][16];
    cx* b = reinterpret_cast<cx*>(buf) + tile * TILE_M;
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        if constexpr (F32) v[a] = tile_ld<CZT_NT>(rb, t, a, (cx*)nullptr);
        else v[a] = __builtin_nontemporal_load(&b[t + 256 * a]);
    }
    // float: the spectrum's loads go out with the tile's, up front, as in fftconv1_kernel -- left to itself the compiler
    // issues each one right before its product and waits for it, 32 L2 round trips in the middle of the tile (in double the
    // 128 registers are not there)
    cx sreg[32];
    const __amdgpu_buffer_rsrc_t rs = tile_rsrc(reinterpret_cast<const cx*>(spec) + (PLAN ? 0 : (int64_t)k1 * TILE_M), TILE_BYTES);
    if constexpr (F32 && !PLAN) {
#pragma unroll
        for (int q = 0; q < 32; ++q) sreg[q] = tile_ld<0>(rs, t, q, (cx*)nullptr);
        __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (F32) tile_forward(v, w, tw, lds, t);
    else tile_forward(v, w, twtab, lds, t);
    if (PLAN) {
        cx* o = reinterpret_cast<cx*>(spec_out) + (int64_t)k1 * TILE_M;
#pragma unroll
        for (int q = 0; q < 32; ++q) o[q * TILE_T + t] = w[q >> 4][q & 15];
        return;
    }
    if constexpr (F32) {
#pragma unroll
        for (int q = 0; q < 32; ++q) w[q >> 4][q & 15] = cmul(w[q >> 4][q & 15], sreg[q]);
    } else {
        // eight spectrum values at a time, fenced: left to itself the scheduler requests all 32 (128 registers) on top of the
        // 128 of the tile, and at two workgroups per CU there are 256 in all
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            __builtin_amdgcn_sched_barrier(0);
            cx sp[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) sp[q] = tile_ld<0>(rs, t, 8 * g + q, (cx*)nullptr);
#pragma unroll
            for (int q = 0; q < 8; ++q) w[(8 * g + q) >> 4][(8 * g + q) & 15] = cmul(w[(8 * g + q) >> 4][(8 * g + q) & 15], sp[q]);
        }
        __builtin_amdgcn_sched_barrier(0);
    }
    __syncthreads();
    if constexpr (F32) tile_inverse(w, v, tw, lds, t);
    else tile_inverse(w, v, twtab, lds, t);
#pragma unroll
    for (int a = 0; a < 32; ++a) {
        if constexpr (F32) tile_st<CZT_NT>(rb, t, a, v[brev(a, 5)]);
        else __builtin_nontemporal_store(v[brev(a, 5)], &b[t + 256 * a]);
    }
}

// MODE 0 (after the first convolution): buf[k] <- conv[k] cP[k] w_k cQ[k] / NFFT for k < K, zero beyond
// MODE 1 (after the second):            y[row, n - lo] <- Re(conv[n] cQ[n]) / (NFFT Q)  for lo <= n < lo + len
// MODE 3: MODE 0 and the second convolution's column pass (cols_fwd MODE 1) in one -- the same thread owns the column in
//         both, so the buffer is read and written once instead of twice
// (the adjoint passes cP in cQ's place for MODE 1: its output lives on the P grid, still divided by Q)
template <typename T, int C, int MODE>
__global__ __launch_bounds__(256) void czt_cols_inv_kernel(typename Prec<T>::T2* __restrict__ buf,
                                                          const typename Prec<T>::T2* __restrict__ cP,
                                                          const typename Prec<T>::T2* __restrict__ cQ,
                                                          float* __restrict__ y, int64_t ldy, int64_t lo, int64_t len,
                                                          CztGeom g) {
    using cx = typename Prec<T>::cxt;
    const int n2 = blockIdx.x * 256 + threadIdx.x;
    const int64_t row = blockIdx.y;
    const int64_t NS = g.NFFT / g.S;
    typename Prec<T>::T2* b = buf + row * NS;
    const ColBuf<T> cb(b, NS);
    cx v[C];
    ColTw<T, C> twi(n2, (int)NS, true);
#pragma unroll
    for (int k1 = 0; k1 < C; ++k1) v[k1] = col_in<T, C>(cb, twi, k1, n2);
    col_dft<C, true>(v);
    const T sc = (T)1 / (T)NS;
    if (MODE == 3) {   // the step between the two convolutions (S = 1): MODE 0's values, then cols_fwd's MODE 1 on them
        cx u[C];
#pragma unroll
        for (int n1 = 0; n1 < C; ++n1) {      // (bin_factor written out: through it the double instances of 12 tiles and
            const int64_t i = (int64_t)n1 * TILE_M + n2;      // more come out scheduled differently)
            cx o = {0, 0};
            if (i < g.K) {
                const T wk = (i == 0 || i == g.K - 1) ? (T)1 : (T)2;
                o = cmul(cmul(v[spos(C, n1)] * sc, to_cx(cP[i])), to_cx(cQ[i])) * wk;
            }
            u[n1] = o;
        }
        col_dft<C, false>(u);
        ColTw<T, C> twf(n2, (int)NS, false);
#pragma unroll
        for (int k1 = 0; k1 < C; ++k1) col_out<T, C>(cb, twf, k1, n2, u[spos(C, k1)]);
        return;
    }
#pragma unroll
    for (int n1 = 0; n1 < C; ++n1) {
        const int64_t i = (int64_t)n1 * TILE_M + n2;
        const cx e = v[spos(C, n1)] * sc;
        if (MODE == 2) cb.st(n1, n2, e);                   // plain inverse of a sub-transform (outer level follows)
        else if (MODE == 0) cb.st(n1, n2, bin_factor<T>(e, i, g, cP, cQ));
        else real_out<T>(e, i, g, cQ, y, ldy, lo, len, row);
    }
}

// ---- outer radix-4 level (S = 4): NFFT = 4 NS, n = n3 NS + n', k = k3 + 4 k' ---------------------------------------
//   forward:  sub[k3][n'] = ( sum_n3 x[n3 NS + n'] W_4^(n3 k3) ) W_NFFT^(n' k3)      then four NS-point transforms
//   inverse:  x[n3 NS + n'] = (1/4) sum_k3 ( sub[k3][n'] conj W_NFFT^(n' k3) ) W_4^(-n3 k3)
// in place (a thread owns the four positions n' + n3 NS).  Input / output modes as in the column kernels.
template <typename T, int MODE>   // 0: real rows times a chirp table; 1: complex buffer; 2: a chirp sequence (plan)
__global__ __launch_bounds__(256) void czt_outer_fwd_kernel(const float* __restrict__ z,
                                                           const typename Prec<T>::T2* __restrict__ tab,
                                                           typename Prec<T>::T2* __restrict__ buf, CztGeom g, int64_t ldz,
                                                           int64_t lo, int64_t len, ChirpSeq cs) {
    using cx = typename Prec<T>::cxt;
    const int64_t NS = g.NFFT / 4;
    const int64_t np = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = blockIdx.y;
    typename Prec<T>::T2* b = buf + row * g.NFFT;
    cx v[4];
#pragma unroll
    for (int n3 = 0; n3 < 4; ++n3) {
        const int64_t i = n3 * NS + np;
        cx e = {0, 0};
        if (MODE == 0) {
            if (i >= lo && i < lo + len) e = to_cx(tab[i]) * (T)z[row * ldz + (i - lo)];
        } else if (MODE == 1) {
            e = buf_load<T>(&b[i]);
        } else {
            if (i <= cs.hi) e = to_cx(chirp_d<T>(i, cs.den, cs.sign));
            else if (i >= g.NFFT - cs.lo) e = to_cx(chirp_d<T>(g.NFFT - i, cs.den, cs.sign));
        }
        v[n3] = e;
    }
    dif<4, false>(v);
#pragma unroll
    for (int k3 = 0; k3 < 4; ++k3) r4_out<T>(b, NS, np, g.NFFT, k3, v[brev(k3, 2)]);
}

template <typename T, int MODE>   // 0: next step's input (times cP w_k cQ for k < K, zero beyond); 1: real output slice
__global__ __launch_bounds__(256) void czt_outer_inv_kernel(typename Prec<T>::T2* __restrict__ buf,
                                                           const typename Prec<T>::T2* __restrict__ cP,
                                                           const typename Prec<T>::T2* __restrict__ cQ,
                                                           float* __restrict__ y, int64_t ldy, int64_t lo, int64_t len,
                                                           CztGeom g) {
    using cx = typename Prec<T>::cxt;
    const int64_t NS = g.NFFT / 4;
    const int64_t np = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = blockIdx.y;
    typename Prec<T>::T2* b = buf + row * g.NFFT;
    cx v[4];
#pragma unroll
    for (int k3 = 0; k3 < 4; ++k3) v[k3] = r4_in<T>(b, NS, np, g.NFFT, k3);
    dif<4, true>(v);
    if (MODE == 2) {   // MODE 0's values, then czt_outer_fwd_kernel's MODE 1 on them: one pass over the buffer
        cx u[4];
#pragma unroll
        for (int n3 = 0; n3 < 4; ++n3) u[n3] = bin_factor<T>(v[brev(n3, 2)], n3 * NS + np, g, cP, cQ, (T)0.25);
        dif<4, false>(u);
#pragma unroll
        for (int k3 = 0; k3 < 4; ++k3) r4_out<T>(b, NS, np, g.NFFT, k3, u[brev(k3, 2)]);
        return;
    }
#pragma unroll
    for (int n3 = 0; n3 < 4; ++n3) {
        const int64_t i = n3 * NS + np;
        const cx e = v[brev(n3, 2)] * (T)0.25;
        if (MODE == 3) buf_store<T>(&b[i], e);             // plain inverse of an inner level
        else if (MODE == 0) buf_store<T>(&b[i], bin_factor<T>(e, i, g, cP, cQ));
        else real_out<T>(e, i, g, cQ, y, ldy, lo, len, row);
    }
}

template <typename T, int MODE>
static void launch_cols_fwd(const CztGeom& g, const float* z, const typename Prec<T>::T2* cP, typename Prec<T>::T2* buf,
                            int64_t rows, hipStream_t st, int64_t ldz = 0, int64_t lo = 0, int64_t len = 0,
                            ChirpSeq cs = ChirpSeq{0, 0, 1, 1.0}) {
    const dim3 grid(TILE_M / 256, (unsigned)(rows * g.S)), blk(256);   // one "row" per sub-transform
    // beyond 32 tiles, what the pair form asks for: every chirp spectrum, and the buffer where its middle step is not fused
#define GFX_CF(CC) case CC: if constexpr (CC <= CZT_MAXC || MODE == 2 || (MODE == 1 && !pair_mid_fused<T, CC>())) \
        hipLaunchKernelGGL((czt_cols_fwd_kernel<T, CC, MODE>), grid, blk, 0, st, z, cP, buf, g, ldz, lo, len, cs); break;
    switch (g.C) { GFX_CZT_PAIR_SIZES(GFX_CF) default: break; }
#undef GFX_CF
}

template <typename T, int MODE>
static void launch_cols_inv(const CztGeom& g, typename Prec<T>::T2* buf, const typename Prec<T>::T2* cP,
                            const typename Prec<T>::T2* cQ, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows,
                            hipStream_t st) {
    const dim3 grid(TILE_M / 256, (unsigned)(rows * g.S)), blk(256);
#define GFX_CI(CC) case CC: hipLaunchKernelGGL((czt_cols_inv_kernel<T, CC, MODE>), grid, blk, 0, st, buf, cP, cQ, y, ldy, lo, len, g); break;
    switch (g.C) { GFX_CZT_SIZES(GFX_CI) default: break; }
#undef GFX_CI
}

// the double tile's twiddles: TW_ROWS x 256 double2 (rows as in fft_tile.hpp), one table per device
__global__ void czt_twiddle_table_f64_kernel(double2* __restrict__ table) {
    const int t = threadIdx.x, row = blockIdx.x;
    int num;
    double den;
    if (row < 4) { num = t * row; den = 8192.0; }
    else if (row < 12) { num = t * 4 * (row - 4); den = 8192.0; }
    else if (row < 16) { num = (t & 15) * (row - 12); den = 256.0; }
    else { num = (t & 15) * 4 * (row - 16); den = 256.0; }
    double s, c;
    sincospi(2.0 * (double)num / den, &s, &c);
    table[row * TILE_T + t] = make_double2(c, -s);
}

static const double2* tile_twiddle_table_f64(hipStream_t stream) {
    static std::mutex mu;
    static double2* tables[64] = {nullptr};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    if (!tables[dev]) {
        double2* p = nullptr;
        if (hipMalloc(&p, sizeof(double2) * TW_ROWS * TILE_T) != hipSuccess) return nullptr;
        hipLaunchKernelGGL(czt_twiddle_table_f64_kernel, dim3(TW_ROWS), dim3(TILE_T), 0, stream, p);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
            hipFree(p);
            return nullptr;
        }
        tables[dev] = p;
    }
    return tables[dev];
}

// The levels below the outermost one and the column pass: every 4^lvl-th part of the buffer is its own transform
template <typename T>
static void czt_inner_fwd(const CztGeom& g, typename Prec<T>::T2* buf, int64_t rows, hipStream_t st) {
    using T2 = typename Prec<T>::T2;
    const ChirpSeq none{0, 0, 1, 1.0};
    for (int lvl = 1; lvl < g.levels; ++lvl) {
        CztGeom gl = g;
        gl.NFFT = g.NFFT >> (2 * lvl);
        const dim3 grid((unsigned)(gl.NFFT / 4 / 256), (unsigned)(rows << (2 * lvl)));
        hipLaunchKernelGGL((czt_outer_fwd_kernel<T, 1>), grid, dim3(256), 0, st, (const float*)nullptr, (const T2*)nullptr, buf,
                           gl, (int64_t)0, (int64_t)0, (int64_t)0, none);
    }
    launch_cols_fwd<T, 1>(g, nullptr, nullptr, buf, rows, st);
}

template <typename T>
static void czt_inner_inv(const CztGeom& g, typename Prec<T>::T2* buf, const typename Prec<T>::T2* cP,
                          const typename Prec<T>::T2* cQ, int64_t rows, hipStream_t st) {
    launch_cols_inv<T, 2>(g, buf, cP, cQ, nullptr, 0, 0, 0, rows, st);
    for (int lvl = g.levels - 1; lvl >= 1; --lvl) {
        CztGeom gl = g;
        gl.NFFT = g.NFFT >> (2 * lvl);
        const dim3 grid((unsigned)(gl.NFFT / 4 / 256), (unsigned)(rows << (2 * lvl)));
        hipLaunchKernelGGL((czt_outer_inv_kernel<T, 3>), grid, dim3(256), 0, st, buf, cP, cQ, (float*)nullptr, (int64_t)0,
                           (int64_t)0, (int64_t)0, gl);
    }
}

template <typename T> static const typename Prec<T>::T2* czt_twiddles(hipStream_t st) {
    if constexpr (sizeof(T) == 4) return tile_twiddle_table(st);
    else return tile_twiddle_table_f64(st);
}

template <typename T>
static const typename Prec<T>::T2* tile_setup(bool plan, hipStream_t st) {
    const typename Prec<T>::T2* tw = czt_twiddles<T>(st);
    const bool ok = tw && (plan ? allow_lds(czt_rows_kernel<T, true>, Prec<T>::lds_bytes) == GFX_OK
                                : allow_lds(czt_rows_kernel<T, false>, Prec<T>::lds_bytes) == GFX_OK);
    return ok ? tw : nullptr;
}

template <typename T>
static void tile_pass(typename Prec<T>::T2* buf, const typename Prec<T>::T2* spec, int64_t tiles, int ctot,
                      const typename Prec<T>::T2* tw, hipStream_t st) {
    hipLaunchKernelGGL((czt_rows_kernel<T, false>), dim3((unsigned)tiles), dim3(TILE_T), Prec<T>::lds_bytes, st, buf, spec,
                       (typename Prec<T>::T2*)nullptr, ctot, tw);
}

template <typename T>
static void chirp_tables(typename Prec<T>::T2* cP, typename Prec<T>::T2* cQ, int64_t P, hipStream_t st) {
    hipLaunchKernelGGL(czt_chirp_table_kernel<T>, dim3((unsigned)((P + 255) / 256)), dim3(256), 0, st, cP, P, P, -1.0f);
    hipLaunchKernelGGL(czt_chirp_table_kernel<T>, dim3((unsigned)((P - 1 + 255) / 256)), dim3(256), 0, st, cQ, P - 1, P - 1, 1.0f);
}

// the sequence through the forward passes of the transform, then the tile pass in PLAN mode
template <typename T>
static void chirp_spectrum(const CztGeom& g, ChirpSeq cs, typename Prec<T>::T2* buf, typename Prec<T>::T2* spec,
                           const typename Prec<T>::T2* tw, hipStream_t st) {
    using T2 = typename Prec<T>::T2;
    const int ctot = g.S * g.C;
    if (g.levels == 0) launch_cols_fwd<T, 2>(g, nullptr, nullptr, buf, 1, st, 0, 0, 0, cs);
    else {
        hipLaunchKernelGGL((czt_outer_fwd_kernel<T, 2>), dim3((unsigned)(g.NFFT / 4 / 256), 1), dim3(256), 0, st, (const float*)nullptr,
                           (const T2*)nullptr, buf, g, (int64_t)0, (int64_t)0, (int64_t)0, cs);
        czt_inner_fwd<T>(g, buf, 1, st);
    }
    hipLaunchKernelGGL((czt_rows_kernel<T, true>), dim3((unsigned)ctot), dim3(TILE_T), Prec<T>::lds_bytes, st, buf,
                       (const T2*)nullptr, spec, ctot, tw);
}

// what the pair form shares with this file (declared in czt_core.hpp)
#define GFX_CZT_SHARED(T, T2)                                                                                                  \
    void czt_levels_fwd(const CztGeom& g, T2* buf, int64_t rows, hipStream_t st) { czt_inner_fwd<T>(g, buf, rows, st); }          \
    void czt_levels_inv(const CztGeom& g, T2* buf, int64_t rows, hipStream_t st) {                                               \
        czt_inner_inv<T>(g, buf, nullptr, nullptr, rows, st);                                                                    \
    }                                                                                                                            \
    const T2* czt_tile_setup(bool plan, hipStream_t st, const T2*) { return tile_setup<T>(plan, st); }                           \
    void czt_tile_pass(T2* buf, const T2* spec, int64_t tiles, int ctot, const T2* tw, hipStream_t st) {                         \
        tile_pass<T>(buf, spec, tiles, ctot, tw, st);                                                                            \
    }                                                                                                                            \
    void czt_chirp_tables(T2* cP, T2* cQ, int64_t P, hipStream_t st) { chirp_tables<T>(cP, cQ, P, st); }                         \
    void czt_chirp_spectrum(const CztGeom& g, ChirpSeq cs, T2* buf, T2* spec, const T2* tw, hipStream_t st) {                    \
        chirp_spectrum<T>(g, cs, buf, spec, tw, st);                                                                             \
    }
GFX_CZT_SHARED(float, float2)
GFX_CZT_SHARED(double, double2)
#undef GFX_CZT_SHARED

template <typename T>
static int czt_plan(void* plan, int64_t P, void* ws, size_t ws_bytes, hipStream_t st) {
    using T2 = typename Prec<T>::T2;
    CztGeom g;
    if (!plan || !czt_geom(P, g)) return GFX_EINVAL;
    if (!ws || ws_bytes < (size_t)g.NFFT * sizeof(T2)) return GFX_ENOSPC;
    const T2* tw = tile_setup<T>(true, st);
    if (!tw) return GFX_ELAUNCH;
    T2* cP = (T2*)plan;
    T2* cQ = cP + g.P;
    T2* spec = cQ + g.Q;
    chirp_tables<T>(cP, cQ, g.P, st);
    // forward: bP over [-(P-1), K-1], bQ over [-(K-1), Q-1];  adjoint: bQ over [-(Q-1), K-1], bP over [-(K-1), P-1]
    const ChirpSeq seqs[4] = {{g.P - 1, g.K - 1, g.P, 1.0}, {g.K - 1, g.Q - 1, g.Q, -1.0},
                              {g.Q - 1, g.K - 1, g.Q, -1.0}, {g.K - 1, g.P - 1, g.P, 1.0}};
    for (int i = 0; i < 4; ++i) chirp_spectrum<T>(g, seqs[i], (T2*)ws, spec + (int64_t)i * g.NFFT, tw, st);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

// The two chirp-z transforms of one direction: rows of `in` (slice [ilo, ilo + ilen) of the first grid, times tab1) ->
// convolution with spec1 -> times cP cQ w_k on the K bins -> convolution with spec2 -> Re(. tab2) / Q into the slice
// [olo, olo + olen) of the second grid.
template <typename T>
static int czt_run(const CztGeom& g, const float* in, int64_t ldi, int64_t ilo, int64_t ilen,
                   const typename Prec<T>::T2* tab1, const typename Prec<T>::T2* spec1, const typename Prec<T>::T2* spec2,
                   const typename Prec<T>::T2* tab2, float* out, int64_t ldo, int64_t olo, int64_t olen, int64_t rows,
                   const typename Prec<T>::T2* cP, const typename Prec<T>::T2* cQ, typename Prec<T>::T2* buf, hipStream_t st) {
    using T2 = typename Prec<T>::T2;
    const T2* tw = tile_setup<T>(false, st);
    if (!tw) return GFX_ELAUNCH;
    const int ctot = g.S * g.C;
    const int64_t tiles = rows * ctot;
    if (g.levels == 0) {
        launch_cols_fwd<T, 0>(g, in, tab1, buf, rows, st, ldi, ilo, ilen);
        tile_pass<T>(buf, spec1, tiles, ctot, tw, st);
        launch_cols_inv<T, 3>(g, buf, cP, cQ, nullptr, 0, 0, 0, rows, st);
        tile_pass<T>(buf, spec2, tiles, ctot, tw, st);
        launch_cols_inv<T, 1>(g, buf, cP, tab2, out, ldo, olo, olen, rows, st);
        return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
    }
    // outer radix-4 levels around 4^levels sub-transforms of C x 8192 points per row
    const dim3 og((unsigned)(g.NFFT / 4 / 256), (unsigned)rows);
    hipLaunchKernelGGL((czt_outer_fwd_kernel<T, 0>), og, dim3(256), 0, st, in, tab1, buf, g, ldi, ilo, ilen, ChirpSeq{0, 0, 1, 1.0});
    czt_inner_fwd<T>(g, buf, rows, st);
    tile_pass<T>(buf, spec1, tiles, ctot, tw, st);
    czt_inner_inv<T>(g, buf, cP, cQ, rows, st);
    hipLaunchKernelGGL((czt_outer_inv_kernel<T, 2>), og, dim3(256), 0, st, buf, cP, cQ, (float*)nullptr, (int64_t)0,
                       (int64_t)0, (int64_t)0, g);
    czt_inner_fwd<T>(g, buf, rows, st);
    tile_pass<T>(buf, spec2, tiles, ctot, tw, st);
    czt_inner_inv<T>(g, buf, cP, cQ, rows, st);
    hipLaunchKernelGGL((czt_outer_inv_kernel<T, 1>), og, dim3(256), 0, st, buf, cP, tab2, out, ldo, olo, olen, g);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

template <typename T>
static int czt_alias(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                     const void* plan, void* ws, size_t ws_bytes, void* stream, bool adjoint,
                     const gfx_rowmap_t* ymap = nullptr, int yC = 0, int64_t row0 = 0) {
    using T2 = typename Prec<T>::T2;
    CztGeom g;
    if (!z || !y || !plan || rows <= 0 || rows > 16383 || !czt_geom(P, g) || (ymap && adjoint) ||
        !czt_output_args(g, ymap, yC, row0, rows, lo, len, ldy))
        return GFX_EINVAL;
    if (!ws || ws_bytes < (size_t)rows * g.NFFT * sizeof(T2)) return GFX_ENOSPC;
    const T2* cP = (const T2*)plan;
    const T2* cQ = cP + g.P;
    const T2* spec = cQ + g.Q;
    const int64_t step = 65535 / g.S;        // rows * S sub-transforms ride on a grid dimension
    for (int64_t r0 = 0; r0 < rows; r0 += step) {
        const int64_t n = rows - r0 < step ? rows - r0 : step;
        T2* buf = (T2*)ws + r0 * g.NFFT;
        int rc;
        g.row0 = row0 + r0;
        if (!adjoint)   // z (rows x P) -> y[:, lo : lo + len]
            rc = czt_run<T>(g, z + r0 * g.P, g.P, 0, g.P, cP, spec, spec + g.NFFT, cQ, ymap ? y : y + r0 * ldy, ldy, lo, len, n, cP,
                            cQ, buf, (hipStream_t)stream);
        else   // `z` is the gradient gy (row stride ldy) of y[:, lo : lo + len], `y` the gradient gz (rows x P)
            rc = czt_run<T>(g, z + r0 * ldy, ldy, lo, len, cQ, spec + 2 * g.NFFT, spec + 3 * g.NFFT, cP, y + r0 * g.P, g.P, 0,
                            g.P, n, cP, cQ, buf, (hipStream_t)stream);
        if (rc != GFX_OK) return rc;
    }
    return GFX_OK;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_odd_alias_plan_bytes(int64_t P) {
    CztGeom g;
    return czt_geom(P, g) ? czt_plan_f2(g) * sizeof(float2) : 0;
}

size_t gfx_odd_alias_workspace_bytes(int64_t rows, int64_t P) {
    CztGeom g;
    if (rows <= 0 || !czt_geom(P, g)) return 0;
    return (size_t)rows * g.NFFT * sizeof(float2);
}

int gfx_odd_alias_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream) {
    return czt_plan<float>(plan, P, ws, ws_bytes, (hipStream_t)stream);
}

int gfx_odd_alias_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                      const void* plan, void* ws, size_t ws_bytes, const gfx_rowmap_t* ymap, int64_t C, int64_t row0,
                      void* stream) {
    if (!ymap) return czt_alias<float>(z, y, ldy, lo, len, rows, P, plan, ws, ws_bytes, stream, false);
    if (C < 1 || C > 0x7fffffffLL) return GFX_EINVAL;
    return czt_alias<float>(z, y, len, lo, len, rows, P, plan, ws, ws_bytes, stream, false, ymap, (int)C, row0);
}

// Transpose of gfx_odd_alias_f32 (the gradient of the aliasing step): with G'[k] = sum_n gy[n] e^{+2 pi i k n / Q},
//   gz[m] = Re( sum_{k < K} w_k G'[k] e^{-2 pi i k m / P} ) / Q
// i.e. the same two chirp-z transforms in the other order -- cQ / bQ first (Q inputs, K bins), cP / bP second (P
// outputs) -- with the chirps' supports mirrored (the plan's third and fourth spectrum).
int gfx_odd_alias_adjoint_f32(const float* gy, int64_t ldg, int64_t lo, int64_t len, float* gz, int64_t rows, int64_t P,
                              const void* plan, void* ws, size_t ws_bytes, void* stream) {
    return czt_alias<float>(gy, gz, ldg, lo, len, rows, P, plan, ws, ws_bytes, stream, true);
}

// ---- the same with double-precision transforms (fp32 in and out): plan and workspace are twice the size ------------
size_t gfx_odd_alias_precise_plan_bytes(int64_t P) { return 2 * gfx_odd_alias_plan_bytes(P); }

size_t gfx_odd_alias_precise_workspace_bytes(int64_t rows, int64_t P) { return 2 * gfx_odd_alias_workspace_bytes(rows, P); }

int gfx_odd_alias_precise_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream) {
    return czt_plan<double>(plan, P, ws, ws_bytes, (hipStream_t)stream);
}

int gfx_odd_alias_precise_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                              const void* plan, void* ws, size_t ws_bytes, void* stream) {
    return czt_alias<double>(z, y, ldy, lo, len, rows, P, plan, ws, ws_bytes, stream, false);
}

int gfx_odd_alias_precise_adjoint_f32(const float* gy, int64_t ldg, int64_t lo, int64_t len, float* gz, int64_t rows,
                                      int64_t P, const void* plan, void* ws, size_t ws_bytes, void* stream) {
    return czt_alias<double>(gy, gz, ldg, lo, len, rows, P, plan, ws, ws_bytes, stream, true);
}

}  // extern "C"
