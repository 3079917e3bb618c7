// Backward of the dynamics path (dynamics.hip): the gain computer's derivatives, the fused backward of the compressor /
// gate with the one-pole energy smoother (row kernel and one-shot tiles), and the standalone backward pieces.
// Kernels and entry points: included by dynamics.hip alone and compiled as part of it (the end of that file says why).
#pragma once
#include "dyn_common.hpp"

namespace gfx {

// ---- backward of the gain computer (training path of Compressor / NoiseGate) --------------------------------
// Partial derivatives of g = log_gain(G) (dynamics.py:444-489 compressor, 676-721 gate) w.r.t. G, the threshold T,
// log_ratio and log_knee.  The region masks are piecewise constant, as in torch's autograd of the same expressions.
struct KneeGrad {
    float dG, dT, dlr, dlk;
};
__device__ __forceinline__ KneeGrad log_gain_grad(const Knee& q, float G) {
    KneeGrad o = {0.0f, 0.0f, 0.0f, 0.0f};
    const float d = G - q.T;
    if (!q.gate) {
        const float c = q.invR - 1.0f;  // (1/R - 1)
        if (q.kind == 0 || (q.kind == 1 && G > q.T + q.W)) {
            if (q.kind == 1 || d > 0.0f) {  // above the threshold: g = (1/R - 1)(G - T)
                o.dG = c;
                o.dT = -c;
                o.dlr = -d * q.invR * q.invR * q.er;
            }
        } else if (q.kind == 1) {
            if (!(G < q.T - q.W)) {  // knee region: g = c s^2 / (4W), s = G - T + W
                const float s = d + q.W, h = s / (2.0f * q.W);
                o.dG = c * h;
                o.dT = -c * h;
                o.dlr = -q.invR * q.invR * s * s / (4.0f * q.W) * q.er;
                o.dlk = c * (h - h * h) * q.W;  // dg/dW * dW/dlk,  W = exp(lk)/2
            }
        } else {  // exponential: g = c softplus(k d) / k
            const float v = q.k * d;
            const float sp = softplusf(v), sg = v > 20.0f ? 1.0f : sigmoidf(v);
            o.dG = c * sg;
            o.dT = -c * sg;
            o.dlr = -q.invR * q.invR * sp / q.k * q.er;
            o.dlk = c * (sg * v - sp) / q.k;  // dg/dk * k
        }
    } else {
        const float c = 1.0f - q.R;  // (1 - R) = -exp(lr)
        if (q.kind == 0 || (q.kind == 1 && G < q.T - q.W)) {
            if (q.kind == 1 || d < 0.0f) {  // below the threshold: g = (R - 1)(G - T)
                o.dG = -c;
                o.dT = c;
                o.dlr = d * q.er;
            }
        } else if (q.kind == 1) {
            if (!(G > q.T + q.W)) {  // knee region: g = c s^2 / (4W), s = G - T - W
                const float s = d - q.W, h = s / (2.0f * q.W);
                o.dG = c * h;
                o.dT = -c * h;
                o.dlr = -s * s / (4.0f * q.W) * q.er;
                o.dlk = c * (-h - h * h) * q.W;
            }
        } else {  // exponential: g = -er softplus(k (T - G)) / k
            const float v = -q.k * d;
            const float sp = softplusf(v), sg = v > 20.0f ? 1.0f : sigmoidf(v);
            o.dG = q.er * sg;
            o.dT = -q.er * sg;
            o.dlr = -q.er * sp / q.k;
            o.dlk = -q.er * (sg * v - sp) / q.k;
        }
    }
    return o;
}

// ---- fused backward of the compressor / gate with the one-pole energy smoother ------------------------------
// Two passes, one workgroup per row.  The first (dyn_bwd_u1_kernel, forward in time) scans the energy of x into
//   u1[n] = (1-a) * (untruncated scan of the energy)   (R, L)
// -- or the training forward has stored it already (gfx_dynamics_fused_f32's u1) and the pass is not run.  The second
// (dyn_bwd_c_kernel) walks BACKWARD in time: it recomputes the gain and denv = dL/d(smoothed energy), relu-masked, from
// (x, gy, u1) with env = relu(u1[m] - a^N u1[m-N]), runs the smoother's adjoint de[m] = sum_{k<N} h[k] denv[m+k] (the same
// scan on the reversed sequence), writes gx = gain * gy + (2/C) * de * x and sums the parameter gradients of the row.
//   the scan pass reads 8 B and writes 4 B per stereo sample; the backward walk reads 20 B (x, gy, u1) and writes 8 B.
// Position j of the reversed walk is sample L-1-j.
__device__ __forceinline__ void rload4(const float* __restrict__ row, int64_t j, int64_t L, bool vec, float (&v)[DE]) {
    // v[i] = row[L-1-(j+i)], zero outside [0, L)
    const int64_t hi = L - 1 - j;  // sample of v[0]
    if (vec && hi - 3 >= 0 && hi < L) {
        const float4 q = *reinterpret_cast<const float4*>(row + hi - 3);
        v[0] = q.w; v[1] = q.z; v[2] = q.y; v[3] = q.x;
    } else {
#pragma unroll
        for (int i = 0; i < DE; ++i) v[i] = (hi - i >= 0 && hi - i < L) ? row[hi - i] : 0.0f;
    }
}
__device__ __forceinline__ void rstore4(float* __restrict__ row, int64_t j, int64_t L, bool vec, const float (&v)[DE]) {
    const int64_t hi = L - 1 - j;
    if (vec && hi - 3 >= 0 && hi < L) {
        *reinterpret_cast<float4*>(row + hi - 3) = make_float4(v[3], v[2], v[1], v[0]);
    } else {
#pragma unroll
        for (int i = 0; i < DE; ++i)
            if (hi - i >= 0 && hi - i < L) row[hi - i] = v[i];
    }
}

__device__ __forceinline__ void dyn_bwd_u1_stream(const DynArgs& a, const OnePole& p, const float* x0, const float* x1,
                                                  float* u1, float* slots, int t) {
    const int lane = t & 63, wave = t >> 6;
    const bool vx = vec_ok(x0) && vec_ok(x1), vo = (a.L % 4) == 0;
    const float invC = 1.0f / (float)a.C;
    float carry = 0.0f;
    const int64_t ntiles = (a.L + DTILE - 1) / DTILE;
    float nxa[DE], nxb[DE] = {0.0f, 0.0f, 0.0f, 0.0f};
    load4(x0, (int64_t)DE * t, a.L, vx, nxa);
    if (a.C == 2) load4(x1, (int64_t)DE * t, a.L, vx, nxb);
    for (int64_t tile = 0; tile < ntiles; ++tile) {
        const int64_t n = tile * DTILE + DE * t;
        float xa[DE], xb[DE], e[DE], u[DE], raw[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            xa[i] = nxa[i];
            xb[i] = nxb[i];
        }
        if (tile + 1 < ntiles) {
            load4(x0, n + DTILE, a.L, vx, nxa);
            if (a.C == 2) load4(x1, n + DTILE, a.L, vx, nxb);
        }
#pragma unroll
        for (int i = 0; i < DE; ++i) e[i] = (a.C == 2 ? (xa[i] * xa[i] + xb[i] * xb[i]) : xa[i] * xa[i]) * invC;
        scan_tile(p, e, u, carry, slots + 8 * (tile & 1), lane, wave);
#pragma unroll
        for (int i = 0; i < DE; ++i) raw[i] = p.one_m_a * u[i];
        store4(u1, n, a.L, vo, raw);
    }
}

__global__ __launch_bounds__(DT) void dyn_bwd_u1_kernel(const float* __restrict__ x, const float* __restrict__ z_alpha,
                                                        float* __restrict__ u1, DynArgs a,
                                                        const float* __restrict__ tab = nullptr) {
    __shared__ float slots[16];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (tab && tab[(size_t)r * DP_TAB + DP_ONESHOT] != 0.0f) return;   // a one-shot row rebuilds its scan in its own tiles
    OnePole p;
    onepole_setup(p, z_alpha[r], a.N, t & 63);
    dyn_bwd_u1_stream(a, p, x + row_off(a.xmap, r, 0), x + row_off(a.xmap, r, a.C == 2 ? 1 : 0), u1 + r * a.L, slots, t);
}

// dL/d(smoothed energy) at four (reversed-walk) positions from the samples, output gradients and scan values there;
// also returns the gain and, when `acc` is given, adds the parameter-gradient terms.
// (A: float in the tiles -- eight terms per thread and launch, the sums continue in double --, double in the row kernel, where
// a thread adds hundreds of terms of both signs; FAST: hardware log / exp / reciprocal in the tiles, the library functions in
// the row kernel)
template <bool FAST = false, typename A = float>
__device__ __forceinline__ void dyn_denv4(const DynArgs& a, const Knee& q, const float (&xa)[DE], const float (&xb)[DE],
                                          const float (&ga)[DE], const float (&gb)[DE], const float (&lin)[DE],
                                          float (&dv)[DE], float (&gn)[DE], A* acc) {
#pragma unroll
    for (int i = 0; i < DE; ++i) {
        const float env = fmaxf(lin[i], 0.0f);
        const float G = FAST ? FastMath::log(env + 1e-5f) : logf(env + 1e-5f);
        gn[i] = FAST ? FastMath::exp(log_gain_m<FastMath>(q, G)) : expf(log_gain(q, G));
        const float dgain = a.C == 2 ? (ga[i] * xa[i] + gb[i] * xb[i]) : ga[i] * xa[i];
        const float dg = dgain * gn[i];
        const KneeGrad k = log_gain_grad(q, G);
        dv[i] = lin[i] > 0.0f ? (FAST ? dg * k.dG * __builtin_amdgcn_rcpf(env + 1e-5f) : dg * k.dG / (env + 1e-5f)) : 0.0f;
        if (acc) {   // samples outside the row have x = gy = 0, hence dg = 0
            acc[0] += dg * k.dT;
            acc[1] += dg * k.dlr;
            acc[2] += dg * k.dlk;
        }
    }
}

// For rows whose truncation term is live (TRUNC) the second scan needs denv N samples later and recomputes it from a second
// set of loads there.
// POLE: also accumulate the pole gradient of the truncated smoother.  With U = u1 / (1-a) (the un-truncated scan),
// g = denv and de = this pass's adjoint scan,
//   dL/da = sum_m  -g[m] U[m] + (a^N - (1-a) N a^(N-1)) g[m] U[m-N] + de[m] U[m-1]
// (the last term is sum_n g[n] (1-a) (D[n] - a^N D[n-N]), D = dU/da, moved onto the adjoint scan: D is a scan of U,
// so pairing it with g equals pairing U with the backward scan of g, which is de one sample later).
template <bool TRUNC, bool POLE>
__device__ __forceinline__ void dyn_bwd_c_stream(const DynArgs& a, const OnePole& p, const Knee& q, const float* x0,
                                                 const float* x1, const float* g0, const float* g1, const float* u1,
                                                 float* o0, float* o1, float* slots, int t, double& pole,
                                                 double (&acc)[3]) {
    const int lane = t & 63, wave = t >> 6;
    const bool al = (a.L % 4) == 0;  // reversed float4 groups stay 16-byte aligned only then
    const bool vx = al && vec_ok(x0) && vec_ok(x1) && vec_ok(g0) && vec_ok(g1), vo = al;
    const bool vgx = al && vec_ok(o0) && vec_ok(o1);
    const float k2 = 2.0f / (float)a.C;
    const float pole_c2 = p.a_N - p.one_m_a * (float)a.N * (p.a_N / p.a);
    float carry = 0.0f, carry2 = 0.0f;
    const int64_t ntiles = (a.L + DTILE - 1) / DTILE;
    // software prefetch of the next tile's operands (the scan's barrier would otherwise fence the loads)
    float nu[DE], nxa[DE], nga[DE], nxb[DE] = {0.0f, 0.0f, 0.0f, 0.0f}, ngb[DE] = {0.0f, 0.0f, 0.0f, 0.0f};
    rload4(u1, (int64_t)DE * t, a.L, vo, nu);
    rload4(x0, (int64_t)DE * t, a.L, vx, nxa);
    rload4(g0, (int64_t)DE * t, a.L, vx, nga);
    if (a.C == 2) {
        rload4(x1, (int64_t)DE * t, a.L, vx, nxb);
        rload4(g1, (int64_t)DE * t, a.L, vx, ngb);
    }
    for (int64_t tile = 0; tile < ntiles; ++tile) {
        const int64_t j = tile * DTILE + DE * t;
        float uu[DE], xa[DE], ga[DE], xb[DE], gb[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            uu[i] = nu[i];
            xa[i] = nxa[i];
            ga[i] = nga[i];
            xb[i] = nxb[i];
            gb[i] = ngb[i];
        }
        if (tile + 1 < ntiles) {
            rload4(u1, j + DTILE, a.L, vo, nu);
            rload4(x0, j + DTILE, a.L, vx, nxa);
            rload4(g0, j + DTILE, a.L, vx, nga);
            if (a.C == 2) {
                rload4(x1, j + DTILE, a.L, vx, nxb);
                rload4(g1, j + DTILE, a.L, vx, ngb);
            }
        }
        float un[DE] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (TRUNC) rload4(u1, j + a.N, a.L, false, un);
        float lin[DE], d[DE], gn[DE], u[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) lin[i] = TRUNC ? fmaf(-p.a_N, un[i], uu[i]) : uu[i];
        dyn_denv4(a, q, xa, xb, ga, gb, lin, d, gn, acc);
        scan_tile(p, d, u, carry, slots + 8 * (tile & 1), lane, wave);
        if (TRUNC) {
            // denv at the walk position j - N (N samples later in time), recomputed from its own operands; its lagged scan
            // value is u1 at (j - N) + N = j, i.e. uu
            float u_l[DE], xa2[DE], ga2[DE], xb2[DE] = {0.0f, 0.0f, 0.0f, 0.0f}, gb2[DE] = {0.0f, 0.0f, 0.0f, 0.0f};
            rload4(u1, j - a.N, a.L, false, u_l);
            rload4(x0, j - a.N, a.L, false, xa2);
            rload4(g0, j - a.N, a.L, false, ga2);
            if (a.C == 2) {
                rload4(x1, j - a.N, a.L, false, xb2);
                rload4(g1, j - a.N, a.L, false, gb2);
            }
            float lin2[DE], d2[DE], gn2[DE], u2[DE];
#pragma unroll
            for (int i = 0; i < DE; ++i) lin2[i] = fmaf(-p.a_N, uu[i], u_l[i]);
            dyn_denv4(a, q, xa2, xb2, ga2, gb2, lin2, d2, gn2, (float*)nullptr);
            scan_tile(p, d2, u2, carry2, slots + 8 * (tile & 1) + 4, lane, wave);
#pragma unroll
            for (int i = 0; i < DE; ++i) u[i] = fmaf(-p.a_N, u2[i], u[i]);
        }
        if (POLE) {
            const int64_t below = a.L - 1 - j - DE;  // sample under this thread's four
            const float um = (below >= 0 && below < a.L) ? u1[below] : 0.0f;
#pragma unroll
            for (int i = 0; i < DE; ++i) {
                const float prev = i + 1 < DE ? uu[i + 1] : um;
                pole += (double)(p.one_m_a * u[i] * prev - d[i] * uu[i]);
                if (TRUNC) pole += (double)(pole_c2 * d[i] * un[i]);
            }
        }
        float oa[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) oa[i] = fmaf(gn[i], ga[i], k2 * p.one_m_a * u[i] * xa[i]);
        rstore4(o0, j, a.L, vgx, oa);
        if (a.C == 2) {
            float ob[DE];
#pragma unroll
            for (int i = 0; i < DE; ++i) ob[i] = fmaf(gn[i], gb[i], k2 * p.one_m_a * u[i] * xb[i]);
            rstore4(o1, j, a.L, vgx, ob);
        }
    }
}

__global__ __launch_bounds__(DT) void dyn_bwd_c_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                       gfx_rowmap_t gmap, const float* __restrict__ log_threshold,
                                                       const float* __restrict__ log_ratio,
                                                       const float* __restrict__ log_knee,
                                                       const float* __restrict__ z_alpha, const float* __restrict__ u1,
                                                       float* __restrict__ dalpha, float* __restrict__ gparams,
                                                       float* __restrict__ gx, DynArgs a,
                                                       const float* __restrict__ oneshot_tab) {
    __shared__ float slots[16];
    __shared__ double red[4][4];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x;
    if (oneshot_tab && oneshot_tab[(size_t)r * DP_TAB + DP_ONESHOT] != 0.0f) return;   // dyn_bwd_oneshot_kernel's row
    OnePole p;
    onepole_setup(p, z_alpha[r], a.N, t & 63);
    const float* x0 = x + row_off(a.xmap, r, 0);
    const float* x1 = x + row_off(a.xmap, r, a.C == 2 ? 1 : 0);
    const float* g0 = gy + row_off(gmap, r, 0);
    const float* g1 = gy + row_off(gmap, r, a.C == 2 ? 1 : 0);
    float* o0 = gx + row_off(a.ymap, r, 0);
    float* o1 = gx + row_off(a.ymap, r, a.C == 2 ? 1 : 0);
    Knee q;
    knee_setup(q, log_threshold[r], log_ratio[r], log_knee ? log_knee[r] : 0.0f, a.knee, a.gate);
    double pole = 0.0, acc[3] = {0.0, 0.0, 0.0};    // per-thread sums over the whole row: double (hundreds of terms of both signs)
    const float* ur = u1 + r * a.L;
    if (dalpha) {
        if (p.trunc)
            dyn_bwd_c_stream<true, true>(a, p, q, x0, x1, g0, g1, ur, o0, o1, slots, t, pole, acc);
        else
            dyn_bwd_c_stream<false, true>(a, p, q, x0, x1, g0, g1, ur, o0, o1, slots, t, pole, acc);
    } else if (p.trunc) {
        dyn_bwd_c_stream<true, false>(a, p, q, x0, x1, g0, g1, ur, o0, o1, slots, t, pole, acc);
    } else {
        dyn_bwd_c_stream<false, false>(a, p, q, x0, x1, g0, g1, ur, o0, o1, slots, t, pole, acc);
    }
    double v4[4] = {acc[0], acc[1], acc[2], pole};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = v4[k];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
        if ((t & 63) == 0) red[k][t >> 6] = v;
    }
    __syncthreads();
    if (t < 3) gparams[3 * r + t] = (float)(red[t][0] + red[t][1] + red[t][2] + red[t][3]);
    if (t == 3 && dalpha) dalpha[r] = (float)((red[3][0] + red[3][1] + red[3][2] + red[3][3]) / (double)p.one_m_a);  // u1 = (1-a) U
}

// The backward-in-time pass as dependency-free one-shot tiles (the backward twin of dyn_oneshot_kernel): in the reversed
// "walk" coordinates of dyn_bwd_c_stream the adjoint of the smoother is the same one-pole scan, so a wave takes 512 walk
// positions, rebuilds the scan state entering them from the H positions before (= the H samples LATER in time: lanes
// 4 l < H recompute denv there from their own predicated loads) and needs nothing from any other tile.  Rows are chosen
// on the device from the same pole table; per-row sums (knee parameters, pole) are reduced per workgroup, written to
// `partial` [row][group][4] and added up in group order by dyn_bwd_sums_kernel.  gx means what it means in dyn_bwd_c_kernel.
// Knee kind and compressor / gate are template parameters (one gain-curve path per instantiation: the generic code is
// 15 k instructions, more than the instruction cache holds), every access is a whole aligned float4 (the launcher only
// takes this path for 16-byte aligned rows of a length divisible by four), and log / exp / the reciprocal are the hardware
// forms as in the forward tiles (6.0 vs 6.4 ms with the library functions, 6.9-7.1 for the row kernel, at 8192 rows).
// samples L-4-j .. L-1-j in walk order (v[0] = the latest), zero when the group is outside [0, L)
__device__ __forceinline__ void rl4(const float* __restrict__ row, int64_t j, int64_t L, float (&v)[DE]) {
    const int64_t n = L - 4 - j;
    float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (n >= 0 && n + 4 <= L) q = *reinterpret_cast<const float4*>(row + n);
    v[0] = q.w; v[1] = q.z; v[2] = q.y; v[3] = q.x;
}

// RESCAN (round 6): the smoother's scan u1 is not read but REBUILT from x -- in walk coordinates the forward-in-time scan is
// a SUFFIX scan (u1[j] depends on the positions after j = the samples before it in time): the two sub-tiles' local and
// in-wave scans run with the shuffles mirrored, the state entering the tile from its far end is the dot product of the H
// samples beyond it (x only: one more predicated 16-byte load per channel), and the H positions in front of the tile (whose
// denv the adjoint scan needs) continue the scan from the tile's first value.  4 of the 28 bytes per stereo sample go away
// here, and the forward pass of a training step does not have to store the scan at all (4 of its 20).
// (three waves per SIMD = 168 VGPRs: the rescan's 169-172 would otherwise cost a whole wave of occupancy)
template <int KIND, bool GATE, bool RESCAN>
__global__ __launch_bounds__(DT, 3) void dyn_bwd_oneshot_kernel(const float* __restrict__ x, const float* __restrict__ gy,
                                                             gfx_rowmap_t gmap, const float* __restrict__ log_threshold,
                                                             const float* __restrict__ log_ratio,
                                                             const float* __restrict__ log_knee,
                                                             const float* __restrict__ tab, const float* __restrict__ u1,
                                                             const float* __restrict__ dalpha /* only: wanted? */,
                                                             double* __restrict__ partial,
                                                             float* __restrict__ gx, DynArgs a, unsigned ngroups,
                                                             unsigned nblocks) {
    __shared__ double red[4][4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned per_xcd = gridDim.x >> 3;
    const unsigned b = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (b >= nblocks) return;
    const unsigned r = b / ngroups;
    const unsigned grp = b - r * ngroups;
    const float* tb = tab + (size_t)r * DP_TAB;
    if (tb[DP_ONESHOT] == 0.0f) return;                 // dyn_bwd_c_kernel's row (uniform)
    const int64_t s = (int64_t)grp * OS_GTILE + (int64_t)wave * OS_WTILE;     // first WALK position of this wave's tile
    const int64_t L = s < a.L ? a.L : 0;                // a wave past the row end reads zeros and stores nothing
    const float* x0 = x + row_off(a.xmap, r, 0);
    const float* x1 = x + row_off(a.xmap, r, a.C == 2 ? 1 : 0);
    const float* g0 = gy + row_off(gmap, r, 0);
    const float* g1 = gy + row_off(gmap, r, a.C == 2 ? 1 : 0);
    float* o0 = gx + row_off(a.ymap, r, 0);
    float* o1 = gx + row_off(a.ymap, r, a.C == 2 ? 1 : 0);
    const float* ur = RESCAN ? nullptr : u1 + (int64_t)r * a.L;
    const bool stereo = a.C == 2;
    const int64_t j0 = s + DE * lane;

    float uu[OS_SUB][DE], xa[OS_SUB][DE], xb[OS_SUB][DE], ga[OS_SUB][DE], gb[OS_SUB][DE];
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        if constexpr (!RESCAN) rl4(ur, j0 + 256 * k, L, uu[k]);
        rl4(x0, j0 + 256 * k, L, xa[k]);
        rl4(g0, j0 + 256 * k, L, ga[k]);
        rl4(x1, j0 + 256 * k, stereo ? L : 0, xb[k]);
        rl4(g1, j0 + 256 * k, stereo ? L : 0, gb[k]);
    }
    // walk positions s - 4 (l + 1) .. s - 4 l - 1 = taps 4 l + 3 .. 4 l of the state entering the tile
    const int H = (int)tb[DP_HIST];
    const bool hist = s != 0 && DE * lane < H;
    const int64_t Lh = hist ? L : 0, jh = s - DE * (lane + 1);
    float hu[DE], hxa[DE], hxb[DE], hga[DE], hgb[DE];
    if constexpr (!RESCAN) rl4(ur, jh, Lh, hu);
    rl4(x0, jh, Lh, hxa);
    rl4(g0, jh, Lh, hga);
    rl4(x1, jh, stereo ? Lh : 0, hxb);
    rl4(g1, jh, stereo ? Lh : 0, hgb);
    // u1 one walk position past the tile (the pole term pairs every position with the next one)
    const int64_t edge = a.L - 1 - (s + OS_WTILE);
    float u_edge = 0.0f;
    if constexpr (!RESCAN) u_edge = (dalpha && L != 0 && edge >= 0) ? ur[edge] : 0.0f;
    const float a1 = tb[77], one_m_a = tb[78], a_sub = tb[70];
    const float apk[DE] = {tb[73], tb[74], tb[75], tb[76]};
    const float a_lane = tb[lane];
    float a_step[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) a_step[d] = tb[64 + d];
    if constexpr (RESCAN) {
        const float invC = 1.0f / (float)a.C;
        // the H samples beyond the far end of the tile (walk positions s + 512 + 4 lane + i: EARLIER in time; zeros past
        // the row start), taps a^(4 lane + i)
        float fxa[DE], fxb[DE];
        const int64_t Lf = DE * lane < H ? L : 0;
        rl4(x0, s + OS_WTILE + DE * lane, Lf, fxa);
        rl4(x1, s + OS_WTILE + DE * lane, stereo ? Lf : 0, fxb);
        // local and in-wave SUFFIX scans of the two sub-tiles (independent of each other)
        float fl[OS_SUB][DE], fexcl[OS_SUB], ftot[OS_SUB];
#pragma unroll
        for (int k = 0; k < OS_SUB; ++k) {
            float acc = 0.0f;
#pragma unroll
            for (int i = DE - 1; i >= 0; --i) {
                const float e = (stereo ? (xa[k][i] * xa[k][i] + xb[k][i] * xb[k][i]) : xa[k][i] * xa[k][i]) * invC;
                acc = fmaf(a1, acc, e);
                fl[k][i] = acc;
            }
            float inc = acc;
#pragma unroll
            for (int st = 0; st < 6; ++st) {
                const float dn = __shfl_down(inc, 1 << st, 64);
                if (lane + (1 << st) < 64) inc = fmaf(a_step[st], dn, inc);
            }
            const float ex = __shfl_down(inc, 1, 64);
            fexcl[k] = lane == 63 ? 0.0f : ex;
            ftot[k] = __shfl(inc, 0, 64);
        }
        float w = 0.0f;
#pragma unroll
        for (int i = DE - 1; i >= 0; --i) {
            const float e = (stereo ? (fxa[i] * fxa[i] + fxb[i] * fxb[i]) : fxa[i] * fxa[i]) * invC;
            w = fmaf(a1, w, e);
        }
        float fc = w * a_lane;                    // (lanes without a live tap loaded zeros)
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) fc += __shfl_xor(fc, o, 64);
        u_edge = one_m_a * fc;                    // the scan one walk position past the tile (0 past the row start)
        const float a_far = tb[63 - lane];        // a^(4 (63 - lane)): from the sub-tile's far end to this lane's
#pragma unroll
        for (int k = OS_SUB - 1; k >= 0; --k) {
            const float pre = fmaf(a_far, fc, fexcl[k]);
            fc = fmaf(a_sub, fc, ftot[k]);
#pragma unroll
            for (int i = 0; i < DE; ++i) uu[k][i] = one_m_a * fmaf(apk[DE - 1 - i], pre, fl[k][i]);
        }
        // the scan continued over the H positions in front of the tile (lane l: s - 4 (l + 1) + i), from its value at s
        float hl[DE], acc = 0.0f;
#pragma unroll
        for (int i = DE - 1; i >= 0; --i) {
            const float e = (stereo ? (hxa[i] * hxa[i] + hxb[i] * hxb[i]) : hxa[i] * hxa[i]) * invC;
            acc = fmaf(a1, acc, e);
            hl[i] = acc;
        }
        float inc = acc;
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            const float up = __shfl_up(inc, 1 << st, 64);
            if (lane >= (1 << st)) inc = fmaf(a_step[st], up, inc);
        }
        const float ex = __shfl_up(inc, 1, 64);
        const float pre = fmaf(a_lane, fc, lane == 0 ? 0.0f : ex);
#pragma unroll
        for (int i = 0; i < DE; ++i) hu[i] = one_m_a * fmaf(apk[DE - 1 - i], pre, hl[i]);
    }
    Knee q;
    knee_setup(q, log_threshold[r], log_ratio[r], log_knee ? log_knee[r] : 0.0f, KIND, GATE ? 1 : 0);
    q.kind = KIND;
    q.gate = GATE ? 1 : 0;
    const float k2 = 2.0f / (float)a.C;

    float acc[3] = {0.0f, 0.0f, 0.0f}, pole = 0.0f;
    float d[OS_SUB][DE], gn[OS_SUB][DE], loc[OS_SUB][DE], excl[OS_SUB], total[OS_SUB];
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        dyn_denv4<true>(a, q, xa[k], xb[k], ga[k], gb[k], uu[k], d[k], gn[k], acc);
        float run = 0.0f;
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            run = fmaf(a1, run, d[k][i]);
            loc[k][i] = run;
        }
        float inc = run;
#pragma unroll
        for (int st = 0; st < 6; ++st) {
            const float up = __shfl_up(inc, 1 << st, 64);
            if (lane >= (1 << st)) inc = fmaf(a_step[st], up, inc);
        }
        const float ex = __shfl_up(inc, 1, 64);
        excl[k] = lane == 0 ? 0.0f : ex;
        total[k] = __shfl(inc, 63, 64);
    }
    float carry = 0.0f;
    if (s != 0 && H > 0) {                       // uniform
        float hd[DE], hgn[DE];
        dyn_denv4<true>(a, q, hxa, hxb, hga, hgb, hu, hd, hgn, (float*)nullptr);   // (lanes without a live tap hold zeros: denv = 0)
        float w = 0.0f;                          // Horner, farthest walk position first
#pragma unroll
        for (int i = 0; i < DE; ++i) w = fmaf(a1, w, hd[i]);
        float hs = hist ? w * a_lane : 0.0f;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) hs += __shfl_xor(hs, o, 64);
        carry = hs;
    }
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        const float pre = fmaf(a_lane, carry, excl[k]);
        carry = fmaf(a_sub, carry, total[k]);
        float u[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) u[i] = fmaf(apk[i], pre, loc[k][i]);        // the adjoint scan ("de")
        if (dalpha) {
            // u1 at the next walk position: the neighbouring lane's first value, the next sub-tile's, or the one past the tile
            float nxt = __shfl_down(uu[k][0], 1, 64);
            const float first_next = k + 1 < OS_SUB ? __shfl(uu[k + 1 < OS_SUB ? k + 1 : k][0], 0, 64) : u_edge;
            if (lane == 63) nxt = first_next;
#pragma unroll
            for (int i = 0; i < DE; ++i) {
                const float prev = i + 1 < DE ? uu[k][i + 1] : nxt;
                pole += one_m_a * u[i] * prev - d[k][i] * uu[k][i];
            }
        }
        const int64_t n = L - 4 - (j0 + 256 * k);
        if (n >= 0 && n + 4 <= L) {
            using f4 = float __attribute__((ext_vector_type(4)));
            f4 oa, ob;
#pragma unroll
            for (int i = 0; i < DE; ++i) {
                oa[3 - i] = fmaf(gn[k][i], ga[k][i], k2 * one_m_a * u[i] * xa[k][i]);
                ob[3 - i] = fmaf(gn[k][i], gb[k][i], k2 * one_m_a * u[i] * xb[k][i]);
            }
            *reinterpret_cast<f4*>(o0 + n) = oa;
            if (stereo) *reinterpret_cast<f4*>(o1 + n) = ob;
        }
    }
    double v4[4] = {acc[0], acc[1], acc[2], pole};      // eight terms per thread in float, everything above them in double
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        double v = v4[k];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
        if (lane == 0) red[k][wave] = v;
    }
    __syncthreads();
    // this workgroup's share of the row's four sums; dyn_bwd_sums_kernel adds the shares in group order (no atomics: the
    // parameter gradients are the same bits from run to run)
    if (t < 4) partial[((size_t)r * ngroups + grp) * 4 + t] = red[t][0] + red[t][1] + red[t][2] + red[t][3];
}

// gparams[r] (3 sums) and dalpha[r] of the rows dyn_bwd_oneshot_kernel took: its workgroups' partials in group order, one
// wave per row (lane l adds groups l, l + 64, ... in order, then a shuffle tree).
__global__ __launch_bounds__(64) void dyn_bwd_sums_kernel(const double* __restrict__ partial, const float* __restrict__ tab,
                                                          float* __restrict__ gparams, float* __restrict__ dalpha,
                                                          unsigned ngroups) {
    const unsigned r = blockIdx.x;
    const float* tb = tab + (size_t)r * DP_TAB;
    if (tb[DP_ONESHOT] == 0.0f) return;                 // dyn_bwd_c_kernel wrote this row's sums itself
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    for (unsigned g = threadIdx.x; g < ngroups; g += 64) {
        const double* p = partial + ((size_t)r * ngroups + g) * 4;
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        for (int o = 32; o > 0; o >>= 1) v[k] += __shfl_down(v[k], o, 64);
    if (threadIdx.x == 0) {
        gparams[3 * (size_t)r + 0] = (float)v[0];
        gparams[3 * (size_t)r + 1] = (float)v[1];
        gparams[3 * (size_t)r + 2] = (float)v[2];
        if (dalpha) dalpha[r] = (float)(v[3] / (double)tb[78]);   // u1 = (1 - a) U
    }
}

// One pass over (x, gy, env): gain = exp(g(log(env + 1e-5))),  dgain = sum_c gy x,  dg = dgain * gain,
//   denv = dg * dg/dG / (env + 1e-5),   gparams[r] += sum_n dg * (dg/dT, dg/dlog_ratio, dg/dlog_knee).
__global__ __launch_bounds__(256) void dyn_gain_bwd_kernel(const float* __restrict__ x, gfx_rowmap_t xmap,
                                                           const float* __restrict__ gy, gfx_rowmap_t gmap,
                                                           const float* __restrict__ env,
                                                           const float* __restrict__ log_threshold,
                                                           const float* __restrict__ log_ratio,
                                                           const float* __restrict__ log_knee, int64_t R, int64_t L,
                                                           int C, int knee, int gate, float* __restrict__ gain,
                                                           float* __restrict__ denv, float* __restrict__ gparams) {
    __shared__ float red[3][4];
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y) {
        Knee q;
        knee_setup(q, log_threshold[r], log_ratio[r], log_knee ? log_knee[r] : 0.0f, knee, gate);
        const float* x0 = x + row_off(xmap, r, 0);
        const float* x1 = x + row_off(xmap, r, C == 2 ? 1 : 0);
        const float* g0 = gy + row_off(gmap, r, 0);
        const float* g1 = gy + row_off(gmap, r, C == 2 ? 1 : 0);
        float sT = 0.0f, sR = 0.0f, sK = 0.0f;
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < L; n += (int64_t)gridDim.x * blockDim.x) {
            const float e = env[r * L + n];
            const float G = logf(e + 1e-5f);
            const float gn = expf(log_gain(q, G));
            const float dgain = C == 2 ? (g0[n] * x0[n] + g1[n] * x1[n]) : g0[n] * x0[n];
            const float dg = dgain * gn;
            const KneeGrad k = log_gain_grad(q, G);
            gain[r * L + n] = gn;
            denv[r * L + n] = dg * k.dG / (e + 1e-5f);
            sT += dg * k.dT;
            sR += dg * k.dlr;
            sK += dg * k.dlk;
        }
        for (int o = 32; o > 0; o >>= 1) {
            sT += __shfl_down(sT, o, 64);
            sR += __shfl_down(sR, o, 64);
            sK += __shfl_down(sK, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            red[0][threadIdx.x >> 6] = sT;
            red[1][threadIdx.x >> 6] = sR;
            red[2][threadIdx.x >> 6] = sK;
        }
        __syncthreads();
        if (threadIdx.x < 3)
            atomicAdd(&gparams[3 * r + threadIdx.x],
                      red[threadIdx.x][0] + red[threadIdx.x][1] + red[threadIdx.x][2] + red[threadIdx.x][3]);
        __syncthreads();
    }
}

// da[r] = sum_n g[n] (c0 U[n] + c2 U[n-N]) + g[n+1] (c1 S[n] + c3 S[n-N]),  U/S zero before the row start, g[L] = 0:
// the pole gradient of the truncated one-pole smoother from its two scans (see autograd.pole_gradient; the
// one-sample shift pairs g[n+1] with S[n] = D[n+1]).
__global__ __launch_bounds__(256) void onepole_dz_kernel(const float* __restrict__ g, const float* __restrict__ U,
                                                         const float* __restrict__ S, const float* __restrict__ coef,
                                                         float* __restrict__ da, int64_t L, int64_t N) {
    __shared__ float part[4];
    const int64_t r = blockIdx.x;
    const float c0 = coef[4 * r], c1 = coef[4 * r + 1], c2 = coef[4 * r + 2], c3 = coef[4 * r + 3];
    const float* gr = g + r * L;
    const float* Ur = U + r * L;
    const float* Sr = S + r * L;
    float s = 0.0f;
    for (int64_t n = threadIdx.x; n < L; n += 256) {
        float u = c0 * Ur[n], d = c1 * Sr[n];
        if (n >= N) {
            u += c2 * Ur[n - N];
            d += c3 * Sr[n - N];
        }
        s = fmaf(gr[n], u, s);
        if (n + 1 < L) s = fmaf(gr[n + 1], d, s);
    }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o, 64);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) da[r] = part[0] + part[1] + part[2] + part[3];
}

// gx[r,c,n] = gain[r,n] * gy[r,c,n] + (2/C) * de[r,n] * x[r,c,n]   (de = dL/d energy, energy = mean_c x^2)
__global__ void dyn_dx_kernel(const float* __restrict__ x, gfx_rowmap_t xmap, const float* __restrict__ gy,
                              gfx_rowmap_t gmap, const float* __restrict__ gain, const float* __restrict__ de,
                              float* __restrict__ gx, int64_t R, int64_t L, int C) {
    const float k = 2.0f / (float)C;
    for (int64_t r = blockIdx.y; r < R; r += gridDim.y)
    for (int c = 0; c < C; ++c) {
        const float* xr = x + row_off(xmap, r, c);
        const float* gr = gy + row_off(gmap, r, c);
        float* o = gx + (r * C + c) * L;
        for (int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; n < L; n += (int64_t)gridDim.x * blockDim.x)
            o[n] = fmaf(gain[r * L + n], gr[n], k * de[r * L + n] * xr[n]);
    }
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int gfx_dyn_gain_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, const float* env,
                         const float* log_threshold, const float* log_ratio, const float* log_knee, int64_t R, int64_t C,
                         int64_t L, int knee, int gate, float* gain, float* denv, float* gparams, void* stream) {
    if (!x || !gy || !env || !log_threshold || !log_ratio || !gain || !denv || !gparams) return GFX_EINVAL;
    if (R <= 0 || L <= 0 || (C != 1 && C != 2) || knee < 0 || knee > 2 || (knee != 0 && !log_knee)) return GFX_EINVAL;
    hipLaunchKernelGGL(dyn_gain_bwd_kernel, row_grid(R, L), dim3(256), 0, (hipStream_t)stream, x, xmap, gy, gmap, env,
                       log_threshold, log_ratio, log_knee, R, L, (int)C, knee, gate, gain, denv, gparams);
    return GFX_LAUNCH_OK();
}

size_t gfx_dynamics_bwd_ws_bytes(int64_t R, int64_t L) {   // the pole table + four partial sums per one-shot workgroup
    if (R <= 0 || L <= 0) return 0;
    // (the table padded to 8 bytes: the partial sums behind it are doubles)
    return (((size_t)R * DP_TAB + 1) & ~(size_t)1) * sizeof(float) + (size_t)R * (size_t)((L + OS_GTILE - 1) / OS_GTILE) * 4 * sizeof(double);
}

// u1_is_scratch = 0: u1 is the scan the forward pass kept.  u1_is_scratch != 0: u1 is SCRATCH (R x L floats) -- one-shot rows
// rebuild the scan inside their tiles and never touch it, the rows of the row kernel get theirs from dyn_bwd_u1_kernel first
int gfx_dynamics_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap,
                         const float* log_threshold, const float* log_ratio, const float* log_knee,
                         const float* z_alpha, int64_t R, int64_t C, int64_t L, int64_t iir_len, int knee, int gate,
                         float* gx, gfx_rowmap_t gxmap, float* gparams, float* u1, int u1_is_scratch, float* dalpha, void* ws,
                         size_t ws_bytes, void* stream) {
    const bool rescan = u1_is_scratch != 0;
    if (!x || !gy || !log_threshold || !log_ratio || !z_alpha || !gx || !gparams || !u1) return GFX_EINVAL;
    if (R <= 0 || L <= 0 || (C != 1 && C != 2) || iir_len < 1 || knee < 0 || knee > 2 || (knee != 0 && !log_knee))
        return GFX_EINVAL;
    if (R > 0x7fffffffLL || xmap.inner <= 0 || gmap.inner <= 0 || gxmap.inner <= 0) return GFX_EINVAL;
    if (ws && ws_bytes < gfx_dynamics_bwd_ws_bytes(R, L)) return GFX_ENOSPC;
    DynArgs a;
    a.xmap = xmap; a.ymap = gxmap; a.R = R; a.L = L; a.N = iir_len; a.C = (int)C;
    a.smoother = 1; a.knee = knee; a.gate = gate; a.prows = (unsigned)R; a.nchunks = 1; a.chunk_tiles = 0;
    hipStream_t st = (hipStream_t)stream;
    const float* tab = nullptr;
    const int64_t ngroups = (L + OS_GTILE - 1) / OS_GTILE;
    const bool vec = L % 4 == 0 && al16(x, xmap) && al16(gy, gmap) && al16(gx, gxmap) && ((uintptr_t)u1 & 15) == 0;
    if (ws && vec && L > OS_WTILE && R * ngroups <= 0x7ffffff0LL && ws_bytes >= gfx_dynamics_bwd_ws_bytes(R, L)) {
        // rows with a short smoother memory (chosen on the device, as in gfx_dynamics_fused_f32) run as one-shot tiles
        // whose workgroups leave partial sums behind the pole table; the row kernel writes the other rows
        float* t = (float*)ws;
        double* partial = reinterpret_cast<double*>(t + (((size_t)R * DP_TAB + 1) & ~(size_t)1));
        hipLaunchKernelGGL(dyn_pole_table_kernel, dim3((unsigned)R), dim3(64), 0, st, z_alpha, t, R, iir_len, (unsigned*)nullptr);
        const unsigned nblocks = (unsigned)(R * ngroups);
        const dim3 grid((nblocks + 7u) & ~7u);
        with_bool(rescan, [&](auto rs) {
            with_knee(knee, gate != 0, [&](auto kn, auto gt) {
                hipLaunchKernelGGL((dyn_bwd_oneshot_kernel<kn(), gt(), rs()>), grid, dim3(DT), 0, st, x, gy, gmap, log_threshold,
                                   log_ratio, log_knee, (const float*)t, (const float*)u1, (const float*)dalpha, partial, gx,
                                   a, (unsigned)ngroups, nblocks);
            });
        });
        hipLaunchKernelGGL(dyn_bwd_sums_kernel, dim3((unsigned)R), dim3(64), 0, st, (const double*)partial, (const float*)t,
                           gparams, dalpha, (unsigned)ngroups);
        tab = t;
    }
    if (rescan) hipLaunchKernelGGL(dyn_bwd_u1_kernel, dim3((unsigned)R), dim3(DT), 0, st, x, z_alpha, u1, a, tab);
    hipLaunchKernelGGL(dyn_bwd_c_kernel, dim3((unsigned)R), dim3(DT), 0, st, x, gy, gmap, log_threshold,
                       log_ratio, log_knee, z_alpha, u1, dalpha, gparams, gx, a, tab);
    return GFX_LAUNCH_OK();
}

int gfx_onepole_dz_f32(const float* g, const float* U, const float* D, const float* coef, float* da, int64_t R,
                       int64_t L, int64_t N, void* stream) {
    if (!g || !U || !D || !coef || !da || R <= 0 || L <= 0 || N < 1 || R > 0x7fffffffLL) return GFX_EINVAL;
    hipLaunchKernelGGL(onepole_dz_kernel, dim3((unsigned)R), dim3(256), 0, (hipStream_t)stream, g, U, D, coef, da, L, N);
    return GFX_LAUNCH_OK();
}

int gfx_dyn_dx_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, const float* gain,
                   const float* de, float* gx, int64_t R, int64_t C, int64_t L, void* stream) {
    if (!x || !gy || !gain || !de || !gx || R <= 0 || L <= 0 || (C != 1 && C != 2)) return GFX_EINVAL;
    hipLaunchKernelGGL(dyn_dx_kernel, row_grid(R, L), dim3(256), 0, (hipStream_t)stream, x, xmap, gy, gmap, gain, de, gx,
                       R, L, (int)C);
    return GFX_LAUNCH_OK();
}

}  // extern "C"
