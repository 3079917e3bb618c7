// Backward of the exact biquad cascade (csrc/biquad.hip) in two passes over the signal, nothing of the signal's size kept
// between forward and backward (gfx950).
//
// Per row-channel and section i = 1 .. K, a0-normalised (b = B / a0, a = A / a0), u_0 = x, y = u_K:
//     w_i[n] = u_{i-1}[n] - a1 w_i[n-1] - a2 w_i[n-2],   u_i[n] = b0 w_i[n] + b1 w_i[n-1] + b2 w_i[n-2]
// with (w_i[-1], w_i[-2]) = zi and zf = (w_i[L-1], w_i[L-2]).  Given g_K = dL/dy and (q1, q2) = dL/dzf, from K down to 1:
//     r_i[m]   = sum_d b_d g_i[m+d]  (+ q1 at m = L-1, + q2 at m = L-2)
//     lam_i[m] = r_i[m] - a1 lam_i[m+1] - a2 lam_i[m+2]                      g_{i-1} = lam_i,  dL/dx = lam_1
//     db_d = sum_n g_i[n] w_i[n-d] (d = 0, 1, 2),   da_d = -sum_n lam_i[n] w_i[n-d] (d = 1, 2)
//     dzi  = (r_i[-1] - a1 lam_i[0] - a2 lam_i[1],  r_i[-2] - a2 lam_i[0])
//     dB_d = db_d / a0,  dA_d = da_d / a0 (d = 1, 2),  dA_0 = -(sum b_d db_d + sum a_d da_d) / a0.
//
// One wave owns a pair of row-channels from start to end, as in the forward's whole-wave form (64 lanes x 8 samples = one
// 512-sample tile, packed fp32 over the pair):
//   a. biquad_bwd_checkpoint_kernel walks x forward (from zi) without storing y and writes, per tile, every section's
//      entering state (w[n0-1], w[n0-2]) into the workspace: 16 B per pair, section and tile.
//   b. biquad_bwd_adjoint_kernel walks the tiles from the last to the first.  In a tile it
//      - rebuilds u_0 .. u_{K-1} section by section with the forward's lane scan, the carry read from the workspace (no
//        chain from tile to tile), and leaves in LDS every section's per-lane entering state and the input of every G-th
//        section;
//      - then takes the sections in groups of G from the last group to the first: the group's w_i are rerun from those
//        (no scan) into LDS, and read back with the LANES AND SAMPLES REVERSED -- lane l holds the samples of lane 63 - l,
//        latest first.  In that order the adjoint recursion is the forward recursion: the same matrix M, the same powers,
//        the same DPP scan (scan64), its carry (lam[n0+512], lam[n0+513]) kept per section from the later tile.  g, lam and
//        the store of gx live in the reversed order throughout; only w crosses lanes, through LDS.
//      The five sums of a section and tile are added over the wave with DPP in fp32 (a fixed tree) and lane 63 adds the
//      tile's total to a double in LDS; the channel and a0 algebra at the end is in double.  No atomics: two calls give the
//      same bits, and a pair's results do not depend on the other pairs of the call.
// With Cout = 2 a pair is the two channels of one row: the Cf = 1 sum of dB / dA and the Cin = 1 sum of gx are taken inside
// the pair; with more channels a pair is not a row, and the entry refuses a broadcast whose gradient is asked (the caller
// passes that side expanded and adds the channels).  LDS per wave: K * 1.9 KB + (G + ceil(K / G)) * 4 KB with G = ceil(sqrt(K)): 11 KB at K = 1, 32 KB at K = 6,
// 108 KB at K = 32.
#include "biquad_common.hpp"

namespace gfx {

constexpr int BB_TILE = BQ_T * BQ_E;   // 512 samples

using f4 = float __attribute__((ext_vector_type(4)));

struct BbArgs {
    gfx_rowmap_t xmap, gmap, gxmap;
    int64_t L, total, ntiles, pair0;
    int Cin, Cf, Cout, K, G, NG, xvec, gvec, gxvec;
};

// LDS of the adjoint kernel, in this order; the checkpoint kernel uses the first two only
struct BbLds {
    SecConst* sec;   // [K]         carry1 / carry2: checkpoint pass: the running w state; adjoint pass: the lam carry
    f2* rowpow;      // [K][16][4]  M^(E (j + 1))
    f2* st;          // [K][2][64]  per-lane entering state of every section in this tile
    f2* uin;         // [NG][8][64] input of the first section of every group
    f2* wst;         // [G][8][64]  w of the running group's sections
    f2* gc;          // [K][2]      (g_i[n0+512], g_i[n0+513]) from the later tile
    double* acc;     // [K][5][2]   db0, db1, db2, da1, da2 per channel of the pair
};
__device__ __forceinline__ BbLds bb_lds(unsigned char* smem, int K, int G, int NG) {
    BbLds l;
    l.sec = reinterpret_cast<SecConst*>(smem);
    l.rowpow = reinterpret_cast<f2*>(l.sec + K);
    l.st = l.rowpow + (size_t)K * 64;
    l.uin = l.st + (size_t)K * 128;
    l.wst = l.uin + (size_t)NG * 512;
    l.gc = l.wst + (size_t)G * 512;
    l.acc = reinterpret_cast<double*>(l.gc + (size_t)K * 2);
    return l;
}
static inline size_t bb_checkpoint_lds_bytes(int64_t K) { return (size_t)K * (sizeof(SecConst) + 64 * sizeof(f2)); }
static inline size_t bb_adjoint_lds_bytes(int64_t K, int64_t G, int64_t NG) {
    return (size_t)K * (sizeof(SecConst) + (64 + 128 + 2) * sizeof(f2) + 10 * sizeof(double)) +
           (size_t)(G + NG) * 512 * sizeof(f2);
}

// where a pair's two row-channels live
struct BbPair {
    int64_t rc0;
    bool live[2];
    int64_t r[2];
    int c[2];
    const float *B[2], *A[2];
};
__device__ __forceinline__ BbPair bb_pair(const BbArgs& a, const float* Bs, const float* As) {
    BbPair p;
    p.rc0 = 2 * (a.pair0 + (int64_t)blockIdx.x);
    p.live[0] = p.rc0 < a.total;
    p.live[1] = p.rc0 + 1 < a.total;
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        const int64_t rc = p.live[ch] ? p.rc0 + ch : (p.live[0] ? p.rc0 : 0);   // a missing partner re-reads its neighbour
        p.r[ch] = rc / a.Cout;
        p.c[ch] = (int)(rc - p.r[ch] * a.Cout);
        const int64_t f = (p.r[ch] * a.Cf + (a.Cf == 1 ? 0 : p.c[ch])) * a.K * 3;
        p.B[ch] = Bs + f;
        p.A[ch] = As + f;
    }
    return p;
}

// the forward's tables for the whole-wave form: lane (k, ch) takes section k + 32 j of row-channel ch; carries zeroed
__device__ __forceinline__ void bb_tables(const BbLds& l, const BbPair& p, int K, int t) {
    for (int k = t >> 1; k < K; k += BQ_T / 2) {
        const int ch = t & 1;
        const float a0 = p.A[ch][3 * k];
        const float a1 = p.A[ch][3 * k + 1] / a0, a2 = p.A[ch][3 * k + 2] / a0;
        M2d s = {-(double)a1, -(double)a2, 1.0, 0.0};
#pragma unroll
        for (int e = 1; e < BQ_E; e *= 2) s = mul(s, s);   // M^E
        M2d pw_j = s;
        for (int j = 0; j < 16; ++j) {   // M^(E (j + 1))
            float* dst = reinterpret_cast<float*>(l.rowpow + (size_t)(k * 16 + j) * 4);
            dst[0 + ch] = (float)pw_j.a;
            dst[2 + ch] = (float)pw_j.b;
            dst[4 + ch] = (float)pw_j.c;
            dst[6 + ch] = (float)pw_j.d;
            pw_j = mul(pw_j, s);
        }
#pragma unroll
        for (int d = 0; d < 5; ++d) {
            reinterpret_cast<float*>(&l.sec[k].step[d][0])[ch] = (float)s.a;
            reinterpret_cast<float*>(&l.sec[k].step[d][1])[ch] = (float)s.b;
            reinterpret_cast<float*>(&l.sec[k].step[d][2])[ch] = (float)s.c;
            reinterpret_cast<float*>(&l.sec[k].step[d][3])[ch] = (float)s.d;
            s = mul(s, s);
        }
        reinterpret_cast<float*>(&l.sec[k].b0)[ch] = p.B[ch][3 * k] / a0;
        reinterpret_cast<float*>(&l.sec[k].b1)[ch] = p.B[ch][3 * k + 1] / a0;
        reinterpret_cast<float*>(&l.sec[k].b2)[ch] = p.B[ch][3 * k + 2] / a0;
        reinterpret_cast<float*>(&l.sec[k].a1)[ch] = a1;
        reinterpret_cast<float*>(&l.sec[k].a2)[ch] = a2;
        reinterpret_cast<float*>(&l.sec[k].carry1)[ch] = 0.0f;
        reinterpret_cast<float*>(&l.sec[k].carry2)[ch] = 0.0f;
    }
}

// bb_tables above and scan64 below are COPIES of the forward's table set-up and of its step 2 for RL = 64
// (biquad_kernel.hpp, whose text is included twice and cannot be called): the backward rebuilds the forward's states with
// them, so a change to either side must be made on both.
// The forward's step 2 over the 64 lanes: (s1, s2) in: the end state of this lane's chunk run
// from silence; out: the lane's TRUE entering state, given the state (c1, c2) entering the tile.  (nx1, nx2): the state at
// the end of the tile, wave-uniform.
__device__ __forceinline__ void scan64(const SecConst& q, const f2* rp, int rl, f2 c1, f2 c2, f2& s1, f2& s2, f2& nx1,
                                       f2& nx2) {
    f2 i1 = s1, i2 = s2, m1, m2;
    if (rl == 0) {
        apply2(q.step[0], c1, c2, m1, m2);
        i1 += m1;
        i2 += m2;
    }
    apply2(q.step[0], dpp2<0x111>(i1), dpp2<0x111>(i2), m1, m2);
    i1 += m1;
    i2 += m2;
    apply2(q.step[1], dpp2<0x112>(i1), dpp2<0x112>(i2), m1, m2);
    i1 += m1;
    i2 += m2;
    apply2(q.step[2], dpp2<0x114>(i1), dpp2<0x114>(i2), m1, m2);
    i1 += m1;
    i2 += m2;
    apply2(q.step[3], dpp2<0x118>(i1), dpp2<0x118>(i2), m1, m2);
    i1 += m1;
    i2 += m2;
    const f2 w[4] = {rp[0], rp[1], rp[2], rp[3]};
    apply2(w, dpp2<0x142, 0xa>(i1), dpp2<0x142, 0xa>(i2), m1, m2);
    i1 += m1;
    i2 += m2;
    f2 u1 = dpp2<0x143, 0xc>(i1), u2 = dpp2<0x143, 0xc>(i2);
    apply2(q.step[4], u1, u2, m1, m2);   // M^128
    if (rl >= 48) {
        u1 = m1;
        u2 = m2;
    }
    apply2(w, u1, u2, m1, m2);
    i1 += m1;
    i2 += m2;
    s1 = dpp2<0x138>(i1);
    s2 = dpp2<0x138>(i2);
    nx1 = last_lane(i1);
    nx2 = last_lane(i2);
    if (rl == 0) {
        s1 = c1;
        s2 = c2;
    }
}

// the wave's sum in lane 63 (other lanes: partial sums), a fixed tree
__device__ __forceinline__ f2 wave_sum63(f2 v) {
    v += dpp2<0x111>(v);
    v += dpp2<0x112>(v);
    v += dpp2<0x114>(v);
    v += dpp2<0x118>(v);
    v += dpp2<0x142, 0xa>(v);
    v += dpp2<0x143, 0xc>(v);
    return v;
}

// eight consecutive samples from n of a row, zeros from L on
__device__ __forceinline__ void bb_load8(const float* row, int64_t n, int64_t L, bool vec, float (&e)[BQ_E]) {
    if (vec && n + BQ_E <= L) {
#pragma unroll
        for (int j = 0; j < BQ_E / 4; ++j) {
            const f4 q = *reinterpret_cast<const f4*>(row + n + 4 * j);
            e[4 * j] = q.x; e[4 * j + 1] = q.y; e[4 * j + 2] = q.z; e[4 * j + 3] = q.w;
        }
    } else {
#pragma unroll
        for (int i = 0; i < BQ_E; ++i) e[i] = n + i < L ? row[n + i] : 0.0f;
    }
}
__device__ __forceinline__ void bb_store8(float* row, int64_t n, int64_t L, bool vec, const float (&e)[BQ_E]) {
    if (vec && n + BQ_E <= L) {
#pragma unroll
        for (int j = 0; j < BQ_E / 4; ++j)
            __builtin_nontemporal_store(f4{e[4 * j], e[4 * j + 1], e[4 * j + 2], e[4 * j + 3]},
                                        reinterpret_cast<f4*>(row + n + 4 * j));
    } else {
#pragma unroll
        for (int i = 0; i < BQ_E; ++i)
            if (n + i < L) row[n + i] = e[i];
    }
}

// one section over this lane's chunk from its entering state: w into wv (when asked), the section's output into v
template <bool KEEP_W, bool OUT>
__device__ __forceinline__ void bb_section(const SecConst& q, f2 s1, f2 s2, f2 (&v)[BQ_E], f2 (&wv)[BQ_E]) {
    const f2 a1 = q.a1, a2 = q.a2, b0 = q.b0, b1 = q.b1, b2 = q.b2;
#pragma unroll
    for (int i = 0; i < BQ_E; ++i) {
        const f2 w = fma2(-a2, s2, fma2(-a1, s1, v[i]));
        if (KEEP_W) wv[i] = w;
        if (OUT) v[i] = fma2(b0, w, fma2(b1, s1, b2 * s2));
        s2 = s1;
        s1 = w;
    }
}
__device__ __forceinline__ void bb_zero_run(const SecConst& q, const f2 (&v)[BQ_E], f2& s1, f2& s2) {
    const f2 a1 = q.a1, a2 = q.a2;
    s1 = f2{0.0f, 0.0f};
    s2 = f2{0.0f, 0.0f};
#pragma unroll
    for (int i = 0; i < BQ_E; ++i) {
        const f2 w = fma2(-a2, s2, fma2(-a1, s1, v[i]));
        s2 = s1;
        s1 = w;
    }
}

// ------------------------------------------------------------------------------------------------ a. checkpoint pass
__global__ __launch_bounds__(BQ_T) void biquad_bwd_checkpoint_kernel(const float* __restrict__ x,
                                                                     const float* __restrict__ Bs,
                                                                     const float* __restrict__ As,
                                                                     const float* __restrict__ zi, f4* __restrict__ ws,
                                                                     BbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int rl = threadIdx.x;
    const BbLds l = bb_lds(smem, a.K, 0, 0);
    const BbPair p = bb_pair(a, Bs, As);
    bb_tables(l, p, a.K, rl);
    if (zi != nullptr) {
        for (int k = rl >> 1; k < a.K; k += BQ_T / 2) {
            const int ch = rl & 1;
            if (!p.live[ch]) continue;
            const float* z = zi + ((p.rc0 + ch) * a.K + k) * 2;
            reinterpret_cast<float*>(&l.sec[k].carry1)[ch] = z[0];
            reinterpret_cast<float*>(&l.sec[k].carry2)[ch] = z[1];
        }
    }
    __syncthreads();
    if (!p.live[0]) return;   // (the whole workgroup: one wave, one pair)
    const float* xr[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) xr[ch] = x + row_off(a.xmap, p.r[ch], a.Cin == 1 ? 0 : p.c[ch]);
    f4* wsp = ws + (size_t)((a.pair0 + (int64_t)blockIdx.x) * a.ntiles) * a.K;
    for (int64_t t = 0; t < a.ntiles; ++t) {
        const bool last = t + 1 == a.ntiles;   // its entering states are all that is wanted of the last tile
        f2 v[BQ_E], none[BQ_E];
        if (!last) {
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                float e[BQ_E];
                bb_load8(xr[ch], t * BB_TILE + BQ_E * rl, a.L, a.xvec, e);
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) reinterpret_cast<float*>(&v[i])[ch] = e[i];
            }
        }
        for (int k = 0; k < a.K; ++k) {
            SecConst& q = l.sec[k];
            const f2 c1 = q.carry1, c2 = q.carry2;
            if (rl == 0) wsp[t * a.K + k] = f4{c1.x, c1.y, c2.x, c2.y};
            if (last) continue;
            f2 s1, s2, nx1, nx2;
            bb_zero_run(q, v, s1, s2);
            scan64(q, l.rowpow + (size_t)(k * 16 + (rl & 15)) * 4, rl, c1, c2, s1, s2, nx1, nx2);
            if (rl == 0) {
                q.carry1 = nx1;   // same-wave LDS accesses are ordered: read above, write here
                q.carry2 = nx2;
            }
            if (k + 1 < a.K) bb_section<false, true>(q, s1, s2, v, none);
        }
    }
}

// ------------------------------------------------------------------------------------------------ b. adjoint pass
__global__ __launch_bounds__(BQ_T) void biquad_bwd_adjoint_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                                  float* __restrict__ gx, const float* __restrict__ Bs,
                                                                  const float* __restrict__ As,
                                                                  const float* __restrict__ gzf, float* __restrict__ gB,
                                                                  float* __restrict__ gA, float* __restrict__ gzi,
                                                                  const f4* __restrict__ ws, BbArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int rl = threadIdx.x, ml = BQ_T - 1 - rl;
    const BbLds l = bb_lds(smem, a.K, a.G, a.NG);
    const BbPair p = bb_pair(a, Bs, As);
    bb_tables(l, p, a.K, rl);   // (the carries start at zero: lam past the end of the signal)
    for (int i = rl; i < a.K * 2; i += BQ_T) l.gc[i] = f2{0.0f, 0.0f};
    for (int i = rl; i < a.K * 10; i += BQ_T) l.acc[i] = 0.0;
    __syncthreads();
    if (!p.live[0]) return;   // (the whole workgroup: one wave, one pair)
    const float *xr[2], *gr[2];
    float* gxr[2];
#pragma unroll
    for (int ch = 0; ch < 2; ++ch) {
        xr[ch] = x + row_off(a.xmap, p.r[ch], a.Cin == 1 ? 0 : p.c[ch]);
        gr[ch] = g + row_off(a.gmap, p.r[ch], p.c[ch]);
        gxr[ch] = gx == nullptr ? nullptr : gx + row_off(a.gxmap, p.r[ch], a.Cin == 1 ? 0 : p.c[ch]);
    }
    const bool fold_x = a.Cin == 1 && a.Cout == 2;   // the pair is the two channels of one row, which read one x
    const f4* wsp = ws + (size_t)((a.pair0 + (int64_t)blockIdx.x) * a.ntiles) * a.K;
    const f2 zero2 = {0.0f, 0.0f};

    for (int64_t t = a.ntiles - 1; t >= 0; --t) {
        const int64_t n0 = t * BB_TILE;
        const int64_t nm = n0 + BQ_E * ml;   // the chunk this lane holds in the reversed order: gm[j] <-> sample nm + 7 - j
        f2 v[BQ_E], gm[BQ_E], none[BQ_E];
        __syncthreads();   // the later tile's reversed reads of st are done
#pragma unroll
        for (int ch = 0; ch < 2; ++ch) {
            float e[BQ_E];
            bb_load8(xr[ch], n0 + BQ_E * rl, a.L, a.xvec, e);
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) reinterpret_cast<float*>(&v[i])[ch] = e[i];
            bb_load8(gr[ch], nm, a.L, a.gvec, e);
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) reinterpret_cast<float*>(&gm[i])[ch] = p.live[ch] ? e[BQ_E - 1 - i] : 0.0f;
        }
        // the sections' inputs and per-lane entering states, in the forward's lane order
        for (int k = 0; k < a.K; ++k) {
            const SecConst& q = l.sec[k];
            if (k % a.G == 0) {
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) l.uin[((k / a.G) * BQ_E + i) * BQ_T + rl] = v[i];
            }
            const f4 ck = wsp[t * a.K + k];
            f2 s1, s2, nx1, nx2;
            bb_zero_run(q, v, s1, s2);
            scan64(q, l.rowpow + (size_t)(k * 16 + (rl & 15)) * 4, rl, f2{ck.x, ck.y}, f2{ck.z, ck.w}, s1, s2, nx1, nx2);
            l.st[(k * 2) * BQ_T + rl] = s1;
            l.st[(k * 2 + 1) * BQ_T + rl] = s2;
            if (k + 1 < a.K) bb_section<false, true>(q, s1, s2, v, none);
        }
        const bool tail = n0 + BB_TILE + 1 >= a.L;   // the tile holds sample L - 1 or L - 2
        for (int grp = a.NG - 1; grp >= 0; --grp) {
            const int k0 = grp * a.G, k1 = k0 + a.G < a.K ? k0 + a.G : a.K;
            __syncthreads();   // the group before has been read; st and uin are written
#pragma unroll
            for (int i = 0; i < BQ_E; ++i) v[i] = l.uin[(grp * BQ_E + i) * BQ_T + rl];
            for (int k = k0; k < k1; ++k) {
                f2 wv[BQ_E];
                const f2 s1 = l.st[(k * 2) * BQ_T + rl], s2 = l.st[(k * 2 + 1) * BQ_T + rl];
                if (k + 1 < k1)
                    bb_section<true, true>(l.sec[k], s1, s2, v, wv);
                else
                    bb_section<true, false>(l.sec[k], s1, s2, v, wv);
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) l.wst[((k - k0) * BQ_E + i) * BQ_T + rl] = wv[i];
            }
            __syncthreads();   // w crosses lanes
            for (int k = k1 - 1; k >= k0; --k) {
                SecConst& q = l.sec[k];
                const f2 a1 = q.a1, a2 = q.a2, b0 = q.b0, b1 = q.b1, b2 = q.b2;
                // wx[j] = w[nm + 7 - j], j = 0 .. 9: the chunk latest first, then its entering state
                f2 wx[BQ_E + 2];
#pragma unroll
                for (int j = 0; j < BQ_E; ++j) wx[j] = l.wst[((k - k0) * BQ_E + (BQ_E - 1 - j)) * BQ_T + ml];
                wx[BQ_E] = l.st[(k * 2) * BQ_T + ml];
                wx[BQ_E + 1] = l.st[(k * 2 + 1) * BQ_T + ml];
                // r: the two samples after the chunk are the last two of the lane below (lane 0: of the later tile)
                f2 h1 = dpp2<0x138>(gm[BQ_E - 1]), h2 = dpp2<0x138>(gm[BQ_E - 2]);
                if (rl == 0) {
                    h1 = l.gc[2 * k];
                    h2 = l.gc[2 * k + 1];
                }
                const f2 g0 = last_lane(gm[BQ_E - 1]), g1 = last_lane(gm[BQ_E - 2]);   // g[n0], g[n0 + 1]
                f2 r[BQ_E];
                r[0] = fma2(b0, gm[0], fma2(b1, h1, b2 * h2));
                r[1] = fma2(b0, gm[1], fma2(b1, gm[0], b2 * h1));
#pragma unroll
                for (int j = 2; j < BQ_E; ++j) r[j] = fma2(b0, gm[j], fma2(b1, gm[j - 1], b2 * gm[j - 2]));
                f2 q1 = zero2, q2 = zero2;
                if (gzf != nullptr && tail) {
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        if (!p.live[ch]) continue;
                        const float* z = gzf + ((p.rc0 + ch) * a.K + k) * 2;
                        reinterpret_cast<float*>(&q1)[ch] = z[0];
                        reinterpret_cast<float*>(&q2)[ch] = z[1];
                    }
#pragma unroll
                    for (int j = 0; j < BQ_E; ++j) {
                        const int64_t n = nm + BQ_E - 1 - j;
                        if (n == a.L - 1) r[j] += q1;
                        if (n == a.L - 2) r[j] += q2;
                    }
                }
                f2 sum[5] = {zero2, zero2, zero2, zero2, zero2};
#pragma unroll
                for (int j = 0; j < BQ_E; ++j) {
                    sum[0] = fma2(gm[j], wx[j], sum[0]);
                    sum[1] = fma2(gm[j], wx[j + 1], sum[1]);
                    sum[2] = fma2(gm[j], wx[j + 2], sum[2]);
                }
                if (rl == 0) {
                    l.gc[2 * k] = g0;
                    l.gc[2 * k + 1] = g1;
                }
                // lam: the forward recursion in the reversed order
                const f2 c1 = q.carry1, c2 = q.carry2;
                f2 s1, s2, nx1, nx2;
                bb_zero_run(q, r, s1, s2);
                scan64(q, l.rowpow + (size_t)(k * 16 + (rl & 15)) * 4, rl, c1, c2, s1, s2, nx1, nx2);
                if (rl == 0) {
                    q.carry1 = nx1;   // (lam[n0], lam[n0 + 1])
                    q.carry2 = nx2;
                }
#pragma unroll
                for (int j = 0; j < BQ_E; ++j) {
                    const f2 lam = fma2(-a2, s2, fma2(-a1, s1, r[j]));
                    sum[3] = fma2(-lam, wx[j + 1], sum[3]);
                    sum[4] = fma2(-lam, wx[j + 2], sum[4]);
                    gm[j] = lam;
                    s2 = s1;
                    s1 = lam;
                }
#pragma unroll
                for (int d = 0; d < 5; ++d) {
                    const f2 tot = wave_sum63(sum[d]);
                    if (rl == BQ_T - 1) {
                        l.acc[(k * 5 + d) * 2] += (double)tot.x;
                        l.acc[(k * 5 + d) * 2 + 1] += (double)tot.y;
                    }
                }
                if (t == 0 && gzi != nullptr && rl == 0) {
                    // r[-1] = b1 g[0] + b2 g[1] (+ q2 when L = 1), r[-2] = b2 g[0]
                    f2 rm1 = fma2(b1, g0, b2 * g1);
                    if (a.L == 1) rm1 += q2;
                    const f2 z1 = fma2(-a2, nx2, fma2(-a1, nx1, rm1));
                    const f2 z2 = fma2(-a2, nx1, b2 * g0);
#pragma unroll
                    for (int ch = 0; ch < 2; ++ch) {
                        if (!p.live[ch]) continue;
                        float* z = gzi + ((p.rc0 + ch) * a.K + k) * 2;
                        z[0] = ch ? z1.y : z1.x;
                        z[1] = ch ? z2.y : z2.x;
                    }
                }
            }
        }
        if (gx != nullptr) {
#pragma unroll
            for (int ch = 0; ch < 2; ++ch) {
                if (!p.live[ch] || (fold_x && ch == 1)) continue;
                float e[BQ_E];
#pragma unroll
                for (int i = 0; i < BQ_E; ++i) {
                    const f2 s = gm[BQ_E - 1 - i];
                    e[i] = fold_x ? s.x + s.y : (ch ? s.y : s.x);
                }
                bb_store8(gxr[ch], nm, a.L, a.gxvec, e);
            }
        }
    }
    __syncthreads();   // lane 63's sums
    if (gB == nullptr && gA == nullptr) return;
    const bool fold_f = a.Cf == 1 && a.Cout == 2;    // the pair's two channels share one filter
    for (int k = rl >> 1; k < a.K; k += BQ_T / 2) {
        const int ch = rl & 1;
        if (!p.live[ch] || (fold_f && ch == 1)) continue;
        double s[5];
#pragma unroll
        for (int d = 0; d < 5; ++d) s[d] = l.acc[(k * 5 + d) * 2 + ch] + (fold_f ? l.acc[(k * 5 + d) * 2 + 1] : 0.0);
        const double a0 = p.A[ch][3 * k];
        const SecConst& q = l.sec[k];
        const double b0 = reinterpret_cast<const float*>(&q.b0)[ch], b1 = reinterpret_cast<const float*>(&q.b1)[ch],
                     b2 = reinterpret_cast<const float*>(&q.b2)[ch], a1 = reinterpret_cast<const float*>(&q.a1)[ch],
                     a2 = reinterpret_cast<const float*>(&q.a2)[ch];
        const int64_t f = ((p.r[ch] * a.Cf + (a.Cf == 1 ? 0 : p.c[ch])) * a.K + k) * 3;
        if (gB != nullptr) {
            gB[f] = (float)(s[0] / a0);
            gB[f + 1] = (float)(s[1] / a0);
            gB[f + 2] = (float)(s[2] / a0);
        }
        if (gA != nullptr) {
            gA[f] = (float)(-(b0 * s[0] + b1 * s[1] + b2 * s[2] + a1 * s[3] + a2 * s[4]) / a0);
            gA[f + 1] = (float)(s[3] / a0);
            gA[f + 2] = (float)(s[4] / a0);
        }
    }
}

static inline int64_t bb_pairs(int64_t R, int64_t C_out) { return (R * C_out + 1) / 2; }
static inline int64_t bb_tiles(int64_t L) { return (L + BB_TILE - 1) / BB_TILE; }
constexpr int64_t BB_MAX_BLOCKS = 1 << 22;   // pairs per launch

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_biquad_cascade_bwd_ws_bytes(int64_t R, int64_t C_out, int64_t K, int64_t L) {
    if (R <= 0 || C_out <= 0 || K <= 0 || L <= 0) return 0;
    return (size_t)bb_pairs(R, C_out) * (size_t)bb_tiles(L) * (size_t)K * sizeof(f4);
}

int gfx_biquad_cascade_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* g, gfx_rowmap_t gmap, float* gx,
                               gfx_rowmap_t gxmap, const float* Bs, const float* As, const float* zi, const float* gzf,
                               float* gB, float* gA, float* gzi, void* ws, size_t ws_bytes, int64_t R, int64_t C_in,
                               int64_t C_f, int64_t K, int64_t L, void* stream) {
    if (!x || !g || !Bs || !As || R <= 0 || L <= 0 || K < 1 || K > BQ_MAX_K) return GFX_EINVAL;
    if (C_in < 1 || C_f < 1 || (C_in != C_f && C_in != 1 && C_f != 1)) return GFX_EINVAL;
    if (xmap.inner <= 0 || gmap.inner <= 0 || (gx && gxmap.inner <= 0) || R > 0x7fffffffLL) return GFX_EINVAL;
    if (!gx && !gB && !gA && !gzi) return GFX_EINVAL;
    const int64_t C_out = C_in > C_f ? C_in : C_f;
    // a broadcast channel's sum is taken inside the pair, which holds a row's channels only when there are two of them
    if (C_out > 2 && ((C_f == 1 && (gB || gA)) || (C_in == 1 && gx))) return GFX_EINVAL;
    if (!ws ||!aligned16(ws) || ws_bytes < gfx_biquad_cascade_bwd_ws_bytes(R, C_out, K, L)) return GFX_EINVAL;
    BbArgs a;
    a.xmap = xmap; a.gmap = gmap; a.gxmap = gx ? gxmap : xmap;
    a.L = L; a.total = R * C_out; a.ntiles = bb_tiles(L);
    a.Cin = (int)C_in; a.Cf = (int)C_f; a.Cout = (int)C_out; a.K = (int)K;
    a.G = 1;
    while (a.G * a.G < a.K) ++a.G;   // ceil(sqrt(K)) sections a group
    a.NG = (a.K + a.G - 1) / a.G;
    a.xvec = aligned16(x) && map_vec(xmap);
    a.gvec = aligned16(g) && map_vec(gmap);
    a.gxvec = gx && aligned16(gx) && map_vec(gxmap);
    const size_t lds_a = bb_checkpoint_lds_bytes(K), lds_b = bb_adjoint_lds_bytes(K, a.G, a.NG);
    if (allow_lds(biquad_bwd_checkpoint_kernel, lds_a) != GFX_OK || allow_lds(biquad_bwd_adjoint_kernel, lds_b) != GFX_OK)
        return GFX_ELAUNCH;
    const int64_t pairs = bb_pairs(R, C_out);
    for (int64_t p0 = 0; p0 < pairs; p0 += BB_MAX_BLOCKS) {
        const int64_t n = pairs - p0 < BB_MAX_BLOCKS ? pairs - p0 : BB_MAX_BLOCKS;
        a.pair0 = p0;
        hipLaunchKernelGGL(biquad_bwd_checkpoint_kernel, dim3((unsigned)n), dim3(BQ_T), lds_a, (hipStream_t)stream, x, Bs,
                           As, zi, reinterpret_cast<f4*>(ws), a);
        hipLaunchKernelGGL(biquad_bwd_adjoint_kernel, dim3((unsigned)n), dim3(BQ_T), lds_b, (hipStream_t)stream, x, g, gx,
                           Bs, As, gzf, gB, gA, gzi, reinterpret_cast<const f4*>(ws), a);
        if (hipGetLastError() != hipSuccess) return GFX_ELAUNCH;
    }
    return GFX_OK;
}

}  // extern "C"
