// Dynamics path, forward: energy envelope, one-pole smoothing, gain computer and gain stage in one kernel.  The backward
// is dynamics_bwd.hpp, the stages as standalone passes dyn_elementwise.hpp, the ballistics adjoint ballistics_bwd.hpp (all
// three compiled as part of this file, see its end), the ballistics smoother itself ballistics.hip; what they share is
// dyn_common.hpp.
//
// Replaces (reference src/grafx/processors):
//   Compressor.forward / NoiseGate.forward + gain_{hard,quad,exp}_knee   dynamics.py:361-489, 598-721
//   with the TruncatedOnePoleIIRFilter smoother (h = (1-a) a^n, n < N; relu(convolve))   core/envelope.py:34-60
//
// The truncated one-pole FIR is applied as its exact recursive form
//     y[n] = (1-a) * (u[n] - a^N * u[n-N]),   u[n] = a*u[n-1] + e[n]
// with a workgroup-wide prefix scan (wave shuffles + one LDS hop) over 1024-sample tiles, one
// workgroup streaming each row: x is read once and y written once (8 B per channel-sample).
// The a^N correction only runs for rows where it is not negligible (a^N > 1e-9).
#include "dyn_common.hpp"

#ifndef GFX_DYN_PF
#define GFX_DYN_PF 1               // tiles requested ahead of the one being scanned (dyn_fused)
#endif

namespace gfx {

// ---- fused compressor / gate: energy -> one-pole -> log -> knee -> exp -> multiply -----------------
// Tiles [t_lo, t_hi) of the row are produced.  The smoother is a truncated FIR (N taps), so a chunk that does not
// start at the row start is exact if its scans start N samples early from a zero state: tiles [t_warm, t_lo) are
// scanned without producing output, and samples before `s0 = t_warm * DTILE` count as zero for both scans.
// u1row (training forward, whole rows only): also store (1-a) x the UN-truncated scan of the energy, which is what the
// backward pass needs (gfx_dynamics_bwd_f32, u1_is_scratch = 0) -- one extra 4-byte store per sample here instead of a pass over x there.
template <bool TRUNC>
__device__ __forceinline__ void dyn_stream(const DynArgs& a, const OnePole& p, const Knee& q, const float* x0,
                                           const float* x1, float* y0, float* y1, float* slots, int t,
                                           int64_t t_warm, int64_t t_lo, int64_t t_hi, float* u1row = nullptr) {
    const int lane = t & 63, wave = t >> 6;
    const bool vx = vec_ok(x0) && vec_ok(x1) && vec_ok(y0) && vec_ok(y1);
    const bool vu = (a.L % 4) == 0;
    float carry_u = 0.0f;
    const float invC = 1.0f / (float)a.C;
    float carry = 0.0f, carry2 = 0.0f;
    const int64_t s0 = t_warm * DTILE;
    // software prefetch: the next tile's samples are requested before the current tile is scanned, so the
    // HBM round trip overlaps the scan / log / exp work (the barrier inside scan_tile would otherwise fence it)
    // (GFX_DYN_PF tiles ahead: one workgroup streams one row, so its memory parallelism is what it keeps in flight itself)
    float na[GFX_DYN_PF][DE], nb[GFX_DYN_PF][DE];
#pragma unroll
    for (int k = 0; k < GFX_DYN_PF; ++k) {
#pragma unroll
        for (int i = 0; i < DE; ++i) na[k][i] = nb[k][i] = 0.0f;
        if (t_warm + k < t_hi) {
            load4(x0, (t_warm + k) * DTILE + (int64_t)DE * t, a.L, vx, na[k]);
            if (a.C == 2) load4(x1, (t_warm + k) * DTILE + (int64_t)DE * t, a.L, vx, nb[k]);
        }
    }
    for (int64_t tile = t_warm; tile < t_hi; ++tile) {
        const int64_t n = tile * DTILE + DE * t;
        float xa[DE], xb[DE], e[DE], env[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            xa[i] = na[0][i];
            xb[i] = nb[0][i];
        }
#pragma unroll
        for (int k = 0; k + 1 < GFX_DYN_PF; ++k)
#pragma unroll
            for (int i = 0; i < DE; ++i) {
                na[k][i] = na[k + 1][i];
                nb[k][i] = nb[k + 1][i];
            }
        if (tile + GFX_DYN_PF < t_hi) {
            load4(x0, n + (int64_t)GFX_DYN_PF * DTILE, a.L, vx, na[GFX_DYN_PF - 1]);
            if (a.C == 2) load4(x1, n + (int64_t)GFX_DYN_PF * DTILE, a.L, vx, nb[GFX_DYN_PF - 1]);
        }
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            const float sq = a.C == 2 ? (xa[i] * xa[i] + xb[i] * xb[i]) : xa[i] * xa[i];
            e[i] = sq * invC;  // dynamics.py:390 energy = x.square().mean(-2)
        }
        if (a.smoother == 1) {
            float u[DE];
            if (TRUNC && u1row) {   // the un-truncated scan, for the backward pass only (uniform branch)
                float uf[DE], raw[DE];
                scan_tile(p, e, uf, carry_u, slots + 8 * (tile & 1) + 4, lane, wave);
#pragma unroll
                for (int i = 0; i < DE; ++i) raw[i] = p.one_m_a * uf[i];
                store4(u1row, n, a.L, vu, raw);
            }
            if (TRUNC) {
                // ONE scan of e[n] - a^N e[n-N]: the scan is linear, and subtracting before accumulating keeps the
                // truncation exact where U[n] - a^N U[n-N] would cancel (short filters, poles near one)
                float da[DE], db[DE];
                load4(x0, n - a.N, a.L, false, da, s0);
                if (a.C == 2) load4(x1, n - a.N, a.L, false, db, s0);
#pragma unroll
                for (int i = 0; i < DE; ++i)
                    e[i] = fmaf(-p.a_N, (a.C == 2 ? (da[i] * da[i] + db[i] * db[i]) : da[i] * da[i]) * invC, e[i]);
            }
            scan_tile(p, e, u, carry, slots + 8 * (tile & 1), lane, wave);
            if (tile < t_lo) continue;  // warm-up tile: only the scan state matters (uniform branch)
            if (!TRUNC && u1row) {
                float raw[DE];
#pragma unroll
                for (int i = 0; i < DE; ++i) raw[i] = p.one_m_a * u[i];
                store4(u1row, n, a.L, vu, raw);
            }
#pragma unroll
            for (int i = 0; i < DE; ++i) env[i] = fmaxf(p.one_m_a * u[i], 0.0f);  // relu, envelope.py:48
        } else {
#pragma unroll
            for (int i = 0; i < DE; ++i) env[i] = e[i];
        }
        float ga[DE], gb[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            const float G = FastMath::log(env[i] + 1e-5f);                  // dynamics.py:394
            const float g = FastMath::exp(log_gain_m<FastMath>(q, G));      // 402-403
            ga[i] = g * xa[i];
            gb[i] = g * xb[i];
        }
        store4(y0, n, a.L, vx, ga);
        if (a.C == 2) store4(y1, n, a.L, vx, gb);
    }
}

__global__ __launch_bounds__(DT, 1) void dyn_fused_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                       const float* __restrict__ log_threshold,
                                                       const float* __restrict__ log_ratio,
                                                       const float* __restrict__ log_knee,
                                                       const float* __restrict__ z_alpha, DynArgs a,
                                                       float* __restrict__ u1, const float* __restrict__ oneshot_tab) {
    __shared__ float slots[16];
    const int t = threadIdx.x;
    const int64_t r = blockIdx.x / a.nchunks;
    const int chunk = (int)(blockIdx.x - r * a.nchunks);
    OnePole p;
    p.trunc = false;
    const unsigned pr = (unsigned)r % a.prows;
    // rows the one-shot grid takes (dyn_oneshot_kernel, same pole table, complementary test) are not produced here
    if (oneshot_tab && (oneshot_tab[(size_t)pr * DP_TAB + DP_ONESHOT] != 0.0f ||
                        oneshot_tab[(size_t)pr * DP_TAB + DP_LOOKBACK] != 0.0f)) return;
    if (a.smoother == 1) onepole_setup(p, z_alpha[pr], a.N, t & 63);
    Knee q;
    knee_setup(q, log_threshold[pr], log_ratio[pr], log_knee ? log_knee[pr] : 0.0f, a.knee, a.gate);
    const float* x0 = x + row_off(a.xmap, r, 0);
    const float* x1 = x + row_off(a.xmap, r, a.C == 2 ? 1 : 0);
    float* y0 = y + row_off(a.ymap, r, 0);
    float* y1 = y + row_off(a.ymap, r, a.C == 2 ? 1 : 0);
    const int64_t ntiles = (a.L + DTILE - 1) / DTILE;
    const int64_t t_lo = chunk * a.chunk_tiles, t_hi = min(t_lo + a.chunk_tiles, ntiles);
    if (t_lo >= t_hi) return;
    // warm-up: N taps of history (none without a smoother), whole tiles, not before the row start
    const int64_t warm_tiles = a.smoother == 1 ? (a.N + DTILE - 1) / DTILE : 0;
    const int64_t t_warm = t_lo > warm_tiles ? t_lo - warm_tiles : 0;
    float* u1row = u1 ? u1 + r * a.L : nullptr;   // (launched with nchunks = 1 then)
    if (p.trunc)
        dyn_stream<true>(a, p, q, x0, x1, y0, y1, slots, t, t_warm, t_lo, t_hi, u1row);
    else
        dyn_stream<false>(a, p, q, x0, x1, y0, y1, slots, t, t_warm, t_lo, t_hi, u1row);
}

// ---- the same fused compressor / gate as dependency-free ONE-SHOT tiles ---------------------------------------------
// dyn_fused_kernel streams a row per workgroup: a few thousand long-lived streams at scattered addresses, the access
// shape that tops out at 4.8-5.5 TB/s on this chip where a one-shot copy reaches 6.2-6.6 (profiles/r2/
// stream2_copy_ceiling.txt).  Here every 512-sample tile of every row belongs to one WAVE of a short-lived workgroup
// (four consecutive tiles per workgroup, workgroups of a row on consecutive logical block indices of one XCD, so the
// chip sweeps memory front to back) and NO state crosses tiles: the smoother is a FIR, h[k] = (1-a) a^k, so the scan
// state entering a tile is the weighted sum of the H most recent energies before it, u[s-1] = sum_{k<H} a^k e[s-1-k],
// with H the number of taps above 1e-12.  A tile re-reads those H samples (lane l takes taps 4l .. 4l+3 as one
// predicated 16-byte load per channel) and reduces them with six shuffles: no LDS, no barrier.
// Which rows qualify is decided ON THE DEVICE from the pole table (no host synchronisation): a row is taken here when its
// truncation term is dead (a^N <= 1e-12) and H <= OS_HMAX; every other row leaves this grid at once and is produced
// by dyn_fused_kernel, launched over the same rows with the complementary test.
// `any_lb` (nullable): set to 1 when some row takes the look-back tiles -- only then do the tile grids draw tickets
// (see LbArgs); without it no row is given to the look-back (the backward pass, callers without the larger workspace).
__global__ void dyn_pole_table_kernel(const float* __restrict__ z_alpha, float* __restrict__ tab, int64_t rows, int64_t N,
                                      unsigned* __restrict__ any_lb) {
    const int64_t r = blockIdx.x;
    const int lane = threadIdx.x;   // 64 threads
    if (r >= rows) return;
    OnePole p;
    onepole_setup(p, z_alpha[r], N, lane);
    float* t = tab + r * DP_TAB;
    t[lane] = p.a_lane;
    const double la = log((double)p.a);
    t[DP_LB_W + lane] = powk(la, 512.0 * lane);   // weight of the tile `lane + 1` tiles back in the state entering a tile
    if (lane == 0) {
#pragma unroll
        for (int d = 0; d < 6; ++d) t[64 + d] = p.a_step[d];
        t[70] = p.a_wave;
        t[71] = p.a_N;
#pragma unroll
        for (int i = 0; i <= DE; ++i) t[72 + i] = p.ap[i];
        t[77] = p.a;
        t[78] = p.one_m_a;
        t[79] = p.trunc ? 1.0f : 0.0f;
        // taps above 1e-12: H = ceil(log 1e-12 / log a); the row is one-shot material when the N-tap truncation is
        // beyond that (so H <= N and the truncation term is dead) and the history fits the re-read budget; with a longer
        // history (up to 64 tiles of 512 samples) the tiles get their entry state from their predecessors' aggregates
        const double h = ceil(-27.631021115928547 / la);
        const bool dead = h <= (double)N;
        const bool os = dead && h <= (double)OS_HMAX;
        const double m = ceil(h / 512.0);
        const bool lb = any_lb != nullptr && dead && !os && m <= 64.0;
        t[DP_ONESHOT] = os ? 1.0f : 0.0f;
        t[DP_HIST] = os ? (float)h : 0.0f;
        t[DP_LOOKBACK] = lb ? 1.0f : 0.0f;
        t[DP_LB_TILES] = lb ? (float)m : 0.0f;
        if (lb) *any_lb = 1u;
    }
}

// One WAVE per 512-sample tile, four tiles per workgroup, no LDS and no barrier: the wave scans two 256-sample
// sub-tiles (each lane 4 consecutive samples, 6 shuffle steps per sub-tile), chains them through one scalar carry, and
// gets the state entering its tile from the history dot product (lanes 4 l < H, one predicated 16-byte load per channel).
// One wave tile of one row, in two steps so that a caller walking several rows can have the next row's loads in flight
// while it works on this one.  os_load: x and the H samples of history before the tile (lanes 4 l < H; none before the row
// start; s is a multiple of 512).  os_finish: the scans, the gain, the stores of y (and of the scan); returns what it stored.
struct OsIn {
    float xa[OS_SUB][DE], xb[OS_SUB][DE], ha[DE], hb[DE];
};

// LOOK-BACK tiles (round 5): a smoother memory longer than the history a tile may re-read (H > OS_HMAX samples,
// up to 64 tiles) does not send the row to the row kernel any more.  The scan is linear, so the state entering tile j is
//     u[s - 1] = sum_{i >= 1} a^(512 (i - 1)) A[j - i],      A[t] = the state tile t leaves from a ZERO entry state,
// and A[t] depends on tile t's own samples only: every tile publishes its aggregate as soon as its local scans are done
// -- before it needs anything from anybody -- and then reads the M = ceil(H / 512) aggregates before it (lane i polls tile
// j - 1 - i; a 64-lane weighted sum).  One hop of latency, no chain along the row, 8 bytes of traffic per tile and row.
//   * hand-off: one naturally aligned 8-byte {aggregate, 1} granule per (row, tile), written by ONE agent-scope relaxed
//     store and polled with agent-scope relaxed loads (both bypass the CU's L1; an 8-byte granule needs no fence);
//     the granules are zeroed by a memset node in front of the launch.
//   * progress: a tile only ever waits for tiles of the same row with smaller indices, which live in workgroups with
//     smaller logical indices.  Logical indices are handed out by TICKETS (one counter per blockIdx & 7, so that a
//     workgroup's tiles stay on the XCD the block index maps to): whoever holds ticket t knows tickets < t were drawn by
//     workgroups that are running or done -- no assumption about the order in which the hardware starts workgroups.
//     Tickets are drawn only when the pole table found a look-back row (ctrl[8]).
struct LbArgs {
    unsigned long long* gran;   // [row][tile]; nullptr: no look-back in this launch
    unsigned* ctrl;             // [0..7] tickets, [8] "some row looks back"
    unsigned ntiles;            // 512-sample tiles per row
    int split;                  // the routing-sum kernel is launched in both forms (plain / deferred walk), see there
};

__device__ __forceinline__ unsigned lb_block_index(const LbArgs& lb, unsigned per_xcd) {
    __shared__ unsigned ticket;
    unsigned bi = blockIdx.x >> 3;
    if (lb.gran && lb.ctrl[8] != 0u) {     // uniform over the grid
        if (threadIdx.x == 0) ticket = atomicAdd(&lb.ctrl[blockIdx.x & 7u], 1u);
        __syncthreads();
        bi = ticket;
    }
    return (blockIdx.x & 7u) * per_xcd + bi;
}

template <bool AL>
__device__ __forceinline__ void os_load(const DynArgs& a, const float* __restrict__ x0, const float* __restrict__ x1,
                                        bool vx, const float* __restrict__ tb, int64_t s, int lane, OsIn& in) {
    const bool stereo = a.C == 2;
    const int64_t n0 = s + DE * lane;
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        ld4<AL>(x0, n0 + 256 * k, a.L, vx, in.xa[k]);
        if (stereo) ld4<AL>(x1, n0 + 256 * k, a.L, vx, in.xb[k]);
        else {
#pragma unroll
            for (int i = 0; i < DE; ++i) in.xb[k][i] = 0.0f;
        }
    }
    // history taps 4 l .. 4 l + 3 = samples s - 4 (l + 1) .. s - 4 l - 1
    const int H = (int)tb[DP_HIST];
    if (s != 0 && DE * lane < H) {
        ld4<AL>(x0, s - DE * (lane + 1), a.L, vx, in.ha);
        if (stereo) ld4<AL>(x1, s - DE * (lane + 1), a.L, vx, in.hb);
    }
}

// A tile in three steps, so that a caller walking several rows can put other rows' work between them:
//   os_scan    energies, the sub-tiles' local and in-wave scans; the state entering the tile from the re-read history
//              (one-shot rows) -- or, for a look-back row, the tile's aggregate PUBLISHED (see LbArgs)
//   os_lookback  the entry state of a look-back row from the aggregates of the tiles before it (polls them)
//   os_emit    envelope -> gain -> outputs, stores
struct OsMid {
    float loc[OS_SUB][DE], excl[OS_SUB], total[OS_SUB], carry;
};

template <bool AL>
__device__ __forceinline__ void os_scan(const DynArgs& a, const OsIn& in, const float* __restrict__ tb, int64_t s, int lane,
                                        OsMid& mid, unsigned long long* __restrict__ grow) {
    const bool stereo = a.C == 2;
    const float (&xa)[OS_SUB][DE] = in.xa;
    const float (&xb)[OS_SUB][DE] = in.xb;
    const int H = (int)tb[DP_HIST];
    const bool hist = s != 0 && DE * lane < H;
    const float a1 = tb[77], a_sub = tb[70];                             // a, a^256
    const float a_lane = tb[lane];                                       // a^(4 lane)
    float a_step[6];
#pragma unroll
    for (int d = 0; d < 6; ++d) a_step[d] = tb[64 + d];
    const float invC = 1.0f / (float)a.C;
    // the sub-tiles' local and in-wave scans do not depend on each other
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        float acc = 0.0f;
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            const float e = (stereo ? (xa[k][i] * xa[k][i] + xb[k][i] * xb[k][i]) : xa[k][i] * xa[k][i]) * invC;
            acc = fmaf(a1, acc, e);
            mid.loc[k][i] = acc;
        }
        float inc = acc;
#pragma unroll
        for (int d = 0; d < 6; ++d) {
            const float up = __shfl_up(inc, 1 << d, 64);
            if (lane >= (1 << d)) inc = fmaf(a_step[d], up, inc);
        }
        const float ex = __shfl_up(inc, 1, 64);
        mid.excl[k] = lane == 0 ? 0.0f : ex;
        mid.total[k] = __shfl(inc, 63, 64);      // the sub-tile's aggregate, uniform
    }
    // state entering the tile: sum over the live taps of a^k e[s-1-k], k = 4 lane + (3 - i)
    float carry = 0.0f;
    if (grow) {                                   // look-back row (uniform): publish the tile's aggregate
        float agg = mid.total[0];
#pragma unroll
        for (int k = 1; k < OS_SUB; ++k) agg = fmaf(a_sub, agg, mid.total[k]);
        if (lane == 0)
            __hip_atomic_store(grow + (int)(s / OS_WTILE), (1ull << 32) | (unsigned long long)__float_as_uint(agg),
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (s != 0 && H > 0) {                 // uniform
        float hs = 0.0f;
        if (hist) {
            float w = 0.0f;                       // Horner, oldest first: ((e0 a + e1) a + e2) a + e3
#pragma unroll
            for (int i = 0; i < DE; ++i) {
                const float eh = (stereo ? (in.ha[i] * in.ha[i] + in.hb[i] * in.hb[i]) : in.ha[i] * in.ha[i]) * invC;
                w = fmaf(a1, w, eh);
            }
            hs = w * a_lane;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) hs += __shfl_xor(hs, d, 64);
        carry = hs;
    }
    mid.carry = carry;
}

__device__ __forceinline__ float os_lookback(const float* __restrict__ tb, int64_t s, int lane,
                                              const unsigned long long* __restrict__ grow) {
    const int j = (int)(s / OS_WTILE);
    const int M = (int)tb[DP_LB_TILES];
    float hs = 0.0f;
    if (lane < M && lane < j) {
        const unsigned long long* g = grow + (j - 1 - lane);
        unsigned long long v = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while ((v >> 32) == 0ull) {
            __builtin_amdgcn_s_sleep(2);
            v = __hip_atomic_load(g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        hs = __uint_as_float((unsigned)v) * tb[DP_LB_W + lane];
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) hs += __shfl_xor(hs, d, 64);
    return hs;
}

template <bool AL>
__device__ __forceinline__ void os_emit(const DynArgs& a, const float (&xa)[OS_SUB][DE], const float (&xb)[OS_SUB][DE],
                                        const OsMid& mid, float carry, float* __restrict__ y0, float* __restrict__ y1,
                                        bool vx, float* __restrict__ u1row, const float* __restrict__ tb, const Knee& q,
                                        int64_t s, int lane, float (&ga)[OS_SUB][DE], float (&gb)[OS_SUB][DE]) {
    const bool stereo = a.C == 2;
    const int64_t n0 = s + DE * lane;
    const float one_m_a = tb[78], a_sub = tb[70];
    const float apk[DE] = {tb[73], tb[74], tb[75], tb[76]};              // a^1 .. a^4
    const float a_lane = tb[lane];
    const bool vu = (a.L % 4) == 0;
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        const float pre = fmaf(a_lane, carry, mid.excl[k]);   // u just before this lane's first sample of sub-tile k
        carry = fmaf(a_sub, carry, mid.total[k]);
        float raw[DE];
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            const float u = fmaf(apk[i], pre, mid.loc[k][i]);
            raw[i] = one_m_a * u;
            const float env = fmaxf(raw[i], 0.0f);                       // relu, envelope.py:48
            const float G = FastMath::log(env + 1e-5f);                  // dynamics.py:394
            const float g = FastMath::exp(log_gain_m<FastMath>(q, G));   // 402-403
            ga[k][i] = g * xa[k][i];
            gb[k][i] = g * xb[k][i];
        }
        const int64_t n = n0 + 256 * k;
        if (u1row) st4<AL>(u1row, n, a.L, vu, raw);
        if (y0) {                                     // (null: an output-only render that only sums this row)
            st4<AL>(y0, n, a.L, vx, ga[k]);
            if (stereo) st4<AL>(y1, n, a.L, vx, gb[k]);
        }
    }
}

// os_emit for a row whose local scans were NOT kept (the deferred walk of the routing-sum kernel keeps the samples, the
// exclusive in-wave scans and the sub-tile totals of its pending row, 18 registers + 2 scalars, and rebuilds the
// four-sample local scans here -- the same fused multiply-adds in the same order, so the same bits)
template <bool AL>
__device__ __forceinline__ void os_emit_lean(const DynArgs& a, const float (&xa)[OS_SUB][DE], const float (&xb)[OS_SUB][DE],
                                             const float (&excl)[OS_SUB], const float (&total)[OS_SUB], float carry,
                                             float* __restrict__ y0, float* __restrict__ y1, float* __restrict__ u1row,
                                             const float* __restrict__ tb, const Knee& q, int64_t s, int lane,
                                             float (&ga)[OS_SUB][DE], float (&gb)[OS_SUB][DE]) {
    const bool stereo = a.C == 2;
    const int64_t n0 = s + DE * lane;
    const float a1 = tb[77], one_m_a = tb[78], a_sub = tb[70];
    const float apk[DE] = {tb[73], tb[74], tb[75], tb[76]};              // a^1 .. a^4
    const float a_lane = tb[lane];
    const float invC = 1.0f / (float)a.C;
#pragma unroll
    for (int k = 0; k < OS_SUB; ++k) {
        const float pre = fmaf(a_lane, carry, excl[k]);
        carry = fmaf(a_sub, carry, total[k]);
        float raw[DE], acc = 0.0f;
#pragma unroll
        for (int i = 0; i < DE; ++i) {
            const float e = (stereo ? (xa[k][i] * xa[k][i] + xb[k][i] * xb[k][i]) : xa[k][i] * xa[k][i]) * invC;
            acc = fmaf(a1, acc, e);
            const float u = fmaf(apk[i], pre, acc);
            raw[i] = one_m_a * u;
            const float env = fmaxf(raw[i], 0.0f);
            const float G = FastMath::log(env + 1e-5f);
            const float g = FastMath::exp(log_gain_m<FastMath>(q, G));
            ga[k][i] = g * xa[k][i];
            gb[k][i] = g * xb[k][i];
        }
        const int64_t n = n0 + 256 * k;
        if (u1row) st4<AL>(u1row, n, a.L, true, raw);
        if (y0) {
            st4<AL>(y0, n, a.L, true, ga[k]);
            if (stereo) st4<AL>(y1, n, a.L, true, gb[k]);
        }
    }
}

template <bool AL>
__device__ __forceinline__ void os_finish(const DynArgs& a, const OsIn& in, float* __restrict__ y0, float* __restrict__ y1,
                                          bool vx, float* __restrict__ u1row, const float* __restrict__ tb, const Knee& q,
                                          int64_t s, int lane, float (&ga)[OS_SUB][DE], float (&gb)[OS_SUB][DE],
                                          unsigned long long* __restrict__ grow = nullptr) {
    OsMid mid;
    os_scan<AL>(a, in, tb, s, lane, mid, grow);
    const float carry = grow ? os_lookback(tb, s, lane, grow) : mid.carry;
    os_emit<AL>(a, in.xa, in.xb, mid, carry, y0, y1, vx, u1row, tb, q, s, lane, ga, gb);
}

__device__ __forceinline__ void os_tile(const DynArgs& a, const float* __restrict__ x0, const float* __restrict__ x1,
                                        float* __restrict__ y0, float* __restrict__ y1, float* __restrict__ u1row,
                                        const float* __restrict__ tb, const Knee& q, int64_t s, int lane,
                                        float (&ga)[OS_SUB][DE], float (&gb)[OS_SUB][DE],
                                        unsigned long long* __restrict__ grow) {
    const bool vx = vec_ok(x0) && vec_ok(x1) && vec_ok(y0) && vec_ok(y1);
    OsIn in;
    os_load<false>(a, x0, x1, vx, tb, s, lane, in);
    os_finish<false>(a, in, y0, y1, vx, u1row, tb, q, s, lane, ga, gb, grow);
}

__global__ __launch_bounds__(DT) void dyn_oneshot_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                         const float* __restrict__ log_threshold,
                                                         const float* __restrict__ log_ratio,
                                                         const float* __restrict__ log_knee,
                                                         const float* __restrict__ tab, DynArgs a, unsigned ngroups,
                                                         unsigned nblocks, float* __restrict__ u1, LbArgs lb) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // workgroup b runs on XCD b % 8: give each XCD a contiguous run of tiles (a tile's history is its neighbour's data);
    // the runs are whole rows (the launcher pads the grid), so a row's tiles never straddle two runs
    const unsigned per_xcd = gridDim.x >> 3;
    const unsigned b = lb_block_index(lb, per_xcd);
    if (b >= nblocks) return;
    const unsigned r = b / ngroups;
    const unsigned grp = b - r * ngroups;
    const unsigned pr = r % a.prows;
    const float* tb = tab + (size_t)pr * DP_TAB;
    const bool looks_back = lb.gran && tb[DP_LOOKBACK] != 0.0f;   // (the launchers hand look-back rows to the row-group walk)
    if (tb[DP_ONESHOT] == 0.0f && !looks_back) return;          // produced by dyn_fused_kernel / the row-group walk (uniform)
    const int64_t s = (int64_t)grp * OS_GTILE + (int64_t)wave * OS_WTILE;     // first sample of this wave's tile
    if (s >= a.L) return;
    Knee q;
    knee_setup(q, log_threshold[pr], log_ratio[pr], log_knee ? log_knee[pr] : 0.0f, a.knee, a.gate);
    float ga[OS_SUB][DE], gb[OS_SUB][DE];
    os_tile(a, x + row_off(a.xmap, r, 0), x + row_off(a.xmap, r, a.C == 2 ? 1 : 0), y + row_off(a.ymap, r, 0),
            y + row_off(a.ymap, r, a.C == 2 ? 1 : 0), u1 ? u1 + (int64_t)r * a.L : nullptr, tb, q, s, lane, ga, gb,
            looks_back ? lb.gran + (size_t)r * lb.ntiles : nullptr);
}

// The one-shot tiles with the ROUTING SUM that follows fused in (render/core.py:36-112: the "mix" stage whose sources are
// exactly this stage's rows).  The rows of one graph (`inner` consecutive rows, r = g * inner + j) feed the mix
// destinations; a wave owns one 512-sample tile of ALL rows of its graph, walks them in increasing j -- the summation order
// of the gather-sum kernels, from 0.0f, so the sums are bit-identical to the separate pass -- producing each row's output
// as os_tile does and adding it to the accumulators of the destinations it feeds: the mix stage's re-read of every row
// (its whole traffic but the output rows) disappears.  A destination occupies one of NA accumulators only between its
// first and its last source (the host colours the live ranges: the console's four buses take turns in one accumulator,
// the send bus holds the other), and is stored right after its last source -- 32 accumulator registers instead of 16 per
// destination: 115 VGPRs, four waves per SIMD.  sched[j], per row of a graph: bits 0..3 = accumulators
// the row is added to; byte 1 + a = (destination + 1) to store accumulator a to, and clear it, after this row (0: none).
// Rows the pole table sends to dyn_fused_kernel have been written by it BEFORE this grid (the launcher orders it so) and
// are read back here.
struct MixArgs {
    const int64_t* sched;                 // [inner]
    float* out;                           // mix destinations: out + g * sb + j * sv + c * sc
    int64_t sb, sv, sc;
    int inner;
    // sources of the routing sum that are NOT rows of this stage (finished rows of the same buffer, e.g. the reverb return
    // next to the bus compressors in a master sum): pairs (row offset from the first destination row, code as in sched),
    // n_pre of them added before the stage's rows and n_post after -- the sum stays in increasing row order
    const int64_t* extras;
    int n_pre, n_post;
    // the stage's own rows are consumed by the routing sums alone (an output-only render: nobody reads them afterwards), so
    // the tiles do not store them -- rows the ROW kernel produces are still written (the tiles read them back from y)
    int skip_rows;
};

// Knee kind and compressor / gate are template parameters: a wave runs the row body `inner` times, and with every gain curve
// (and the element-wise tail paths of load4 / store4) inlined it is 6 k instructions, more than the instruction cache holds
// -- 5.0 ms for 8192 rows where this form takes 3.3-3.5.  Requesting rows ahead of the one being scanned was measured too
// (register rings of 2-4 rows): slower at every depth, the registers cost more waves than the loads in flight gain
// (EXPERIMENTS.md).  The waves per SIMD are left to the compiler: the deferred walk takes 155 VGPRs, three waves, 4.19 ms for
// the 8192-row stage at a = 0.9975; forced to four waves it is 128 VGPRs and 84 bytes of scratch, 4.31 ms.
template <int NA, bool STEREO, int KIND, bool GATE, bool DEFER>
__global__ __launch_bounds__(DT, 1) void dyn_oneshot_mix_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                             const float* __restrict__ log_threshold,
                                                             const float* __restrict__ log_ratio,
                                                             const float* __restrict__ log_knee,
                                                             const float* __restrict__ tab, DynArgs a, unsigned ngroups,
                                                             unsigned nblocks, float* __restrict__ u1, MixArgs m, LbArgs lb) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // the launcher starts both forms of this kernel: the deferred walk takes the call when some row looks back, the plain
    // walk when none does (uniform over the grid; the other grid leaves at once)
    if (lb.split && (lb.gran && lb.ctrl[8] != 0u) != DEFER) return;
    const unsigned per_xcd = gridDim.x >> 3;
    const unsigned b = lb_block_index(lb, per_xcd);
    if (b >= nblocks) return;
    const unsigned g = b / ngroups;               // graph (batch index)
    const unsigned grp = b - g * ngroups;
    const int64_t s = (int64_t)grp * OS_GTILE + (int64_t)wave * OS_WTILE;
    if (s >= a.L) return;
    const int64_t n0 = s + DE * lane;
    // NA == 0: no routing sum at all -- the walk over groups of `inner` rows that produces the LOOK-BACK rows of a call
    // without a fused sum (every other row belongs to dyn_oneshot_kernel / dyn_fused_kernel and is skipped here)
    // The routing sums' accumulators: registers in the plain walk; in the deferred walk -- whose pending row costs it a wave
    // per SIMD otherwise (155 VGPRs) -- in LDS, which these kernels do not use for anything else: one 16-byte entry per
    // lane, accumulator, sub-tile and channel, lane-contiguous (conflict-free), 32 KB per workgroup for two stereo
    // accumulators.  A row touches the accumulators it feeds with one read-add-write each: ~16 LDS instructions per row
    // and lane against ~200 vector instructions.
    constexpr bool ACC_LDS = DEFER && NA > 0;
    constexpr int NCH = STEREO ? 2 : 1;
    using f4 = float __attribute__((ext_vector_type(4)));
    __shared__ f4 acc_lds[ACC_LDS ? NA * OS_SUB * NCH : 1][DT];
    float acc0[(!ACC_LDS && NA) ? NA : 1][OS_SUB][DE], acc1[(!ACC_LDS && STEREO && NA) ? NA : 1][OS_SUB][DE];
    if (ACC_LDS) {
#pragma unroll
        for (int i = 0; i < NA * OS_SUB * NCH; ++i) acc_lds[i][t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    } else {
#pragma unroll
        for (int c = 0; c < NA; ++c)
#pragma unroll
            for (int k = 0; k < OS_SUB; ++k)
#pragma unroll
                for (int i = 0; i < DE; ++i) {
                    acc0[c][k][i] = 0.0f;
                    if (STEREO) acc1[c][k][i] = 0.0f;
                }
    }
    float* const obase = NA ? m.out + (int64_t)g * m.sb : nullptr;
    // add one row's tile to the accumulators `code` names, then store and clear the destinations it completes
    auto settle = [&](uint64_t code, const float (&ga)[OS_SUB][DE], const float (&gb)[OS_SUB][DE]) {
        const unsigned add = (unsigned)code & 15u;
#pragma unroll
        for (int c = 0; c < NA; ++c) {
            const unsigned fl = (unsigned)(code >> (8 + 8 * c)) & 255u;
            if (ACC_LDS) {
                if ((((add >> c) & 1u) | fl) == 0u) continue;      // uniform: the row neither feeds nor completes it
                float* o0 = obase + (int64_t)(fl ? fl - 1u : 0u) * m.sv;
                float* o1 = o0 + m.sc;
#pragma unroll
                for (int k = 0; k < OS_SUB; ++k) {
                    f4 v0 = acc_lds[(c * OS_SUB + k) * NCH][t], v1 = {0.0f, 0.0f, 0.0f, 0.0f};
                    if (STEREO) v1 = acc_lds[(c * OS_SUB + k) * NCH + 1][t];
                    if ((add >> c) & 1u) {
#pragma unroll
                        for (int i = 0; i < DE; ++i) {
                            v0[i] += ga[k][i];
                            if (STEREO) v1[i] += gb[k][i];
                        }
                    }
                    if (fl != 0u) {                   // this destination is complete: store, clear
                        const float s0[DE] = {v0[0], v0[1], v0[2], v0[3]}, s1[DE] = {v1[0], v1[1], v1[2], v1[3]};
                        st4<true>(o0, n0 + 256 * k, a.L, true, s0);
                        if (STEREO) st4<true>(o1, n0 + 256 * k, a.L, true, s1);
                        v0 = f4{0.0f, 0.0f, 0.0f, 0.0f};
                        v1 = v0;
                    }
                    acc_lds[(c * OS_SUB + k) * NCH][t] = v0;
                    if (STEREO) acc_lds[(c * OS_SUB + k) * NCH + 1][t] = v1;
                }
                continue;
            }
            if ((add >> c) & 1u) {                // uniform
#pragma unroll
                for (int k = 0; k < OS_SUB; ++k)
#pragma unroll
                    for (int i = 0; i < DE; ++i) {
                        acc0[c][k][i] += ga[k][i];
                        if (STEREO) acc1[c][k][i] += gb[k][i];
                    }
            }
            if (fl != 0u) {                       // uniform: this destination is complete
                float* o0 = obase + (int64_t)(fl - 1u) * m.sv;
                float* o1 = o0 + m.sc;
#pragma unroll
                for (int k = 0; k < OS_SUB; ++k) {
                    st4<true>(o0, n0 + 256 * k, a.L, true, acc0[c][k]);
                    if (STEREO) st4<true>(o1, n0 + 256 * k, a.L, true, acc1[c][k]);
#pragma unroll
                    for (int i = 0; i < DE; ++i) {
                        acc0[c][k][i] = 0.0f;
                        if (STEREO) acc1[c][k][i] = 0.0f;
                    }
                }
            }
        }
    };
    auto extra = [&](int e) {                     // a finished row of the buffer that joins the sum
        const float* p0 = obase + m.extras[2 * e] * m.sv;
        const float* p1 = p0 + m.sc;
        float ga[OS_SUB][DE], gb[OS_SUB][DE];
#pragma unroll
        for (int k = 0; k < OS_SUB; ++k) {
            ld4<true>(p0, n0 + 256 * k, a.L, true, ga[k]);
            if (STEREO) ld4<true>(p1, n0 + 256 * k, a.L, true, gb[k]);
        }
        settle((uint64_t)m.extras[2 * e + 1], ga, gb);
    };
    for (int e = 0; e < m.n_pre; ++e) extra(e);
    if (!DEFER) {
        for (int jr = 0; jr < m.inner; ++jr) {
            const unsigned r = g * (unsigned)m.inner + (unsigned)jr;
            const unsigned pr = r % a.prows;
            const float* tb = tab + (size_t)pr * DP_TAB;
            const uint64_t code = (uint64_t)m.sched[jr];
            float* y0 = y + row_off(a.ymap, r, 0);
            float* y1 = y + row_off(a.ymap, r, STEREO ? 1 : 0);
            float ga[OS_SUB][DE], gb[OS_SUB][DE];
            const bool looks_back = tb[DP_LOOKBACK] != 0.0f;
            if (tb[DP_ONESHOT] != 0.0f || looks_back) {   // uniform
                Knee q;
                knee_setup(q, log_threshold[pr], log_ratio[pr], KIND != 0 ? log_knee[pr] : 0.0f, KIND, GATE ? 1 : 0);
                OsIn in;
                os_load<true>(a, x + row_off(a.xmap, r, 0), x + row_off(a.xmap, r, STEREO ? 1 : 0), true, tb, s, lane, in);
                os_finish<true>(a, in, m.skip_rows ? nullptr : y0, y1, true, u1 ? u1 + (int64_t)r * a.L : nullptr, tb, q, s, lane,
                                ga, gb, looks_back ? lb.gran + (size_t)r * lb.ntiles : nullptr);
            } else if (((unsigned)code & 15u) != 0u) {   // the row kernel's row: read back what it wrote
#pragma unroll
                for (int k = 0; k < OS_SUB; ++k) {
                    ld4<true>(y0, n0 + 256 * k, a.L, true, ga[k]);
                    if (STEREO) ld4<true>(y1, n0 + 256 * k, a.L, true, gb[k]);
                }
            }
            settle(code, ga, gb);
        }
    } else {
        // The same walk, one row DEFERRED: row jr is loaded, scanned and -- if it looks back -- its aggregate published
        // before row jr - 1 is finished.  A look-back row then asks for its predecessors' aggregates a whole row time
        // after they were published (the waves of a graph walk the rows side by side), instead of right behind its own
        // publication, when the tiles before it are at the same point of the same row: without the deferral every row of
        // every wave waits out a hand-off (1-3 us of a ~6 us row).  The rows are still finished, and added to the
        // routing sums, in increasing order.
        float pxa[OS_SUB][DE], pxb[OS_SUB][DE], pexcl[OS_SUB];
        float ptotal[OS_SUB], pcarry = 0.0f;      // uniform
        int pkind = 0;                            // 0 nothing pending, 1 computed row, 2 look-back row, 3 read-back row
        unsigned prow = 0;
        uint64_t pcode = 0;
        auto finish = [&]() {
            if (pkind == 1 || pkind == 2) {       // uniform
                const unsigned pr = prow % a.prows;
                const float* tb = tab + (size_t)pr * DP_TAB;
                Knee q;
                knee_setup(q, log_threshold[pr], log_ratio[pr], KIND != 0 ? log_knee[pr] : 0.0f, KIND, GATE ? 1 : 0);
                const float carry = pkind == 2 ? os_lookback(tb, s, lane, lb.gran + (size_t)prow * lb.ntiles) : pcarry;
                float ga[OS_SUB][DE], gb[OS_SUB][DE];
                os_emit_lean<true>(a, pxa, pxb, pexcl, ptotal, carry, m.skip_rows ? nullptr : y + row_off(a.ymap, prow, 0),
                                   y + row_off(a.ymap, prow, STEREO ? 1 : 0), u1 ? u1 + (int64_t)prow * a.L : nullptr, tb, q, s,
                                   lane, ga, gb);
                settle(pcode, ga, gb);
            } else {
                settle(pcode, pxa, pxb);          // a row the row kernel wrote (read back below), or one nobody sums
            }
        };
        int walked = 0;
        for (int jr = 0; jr < m.inner; ++jr) {
            const unsigned r = g * (unsigned)m.inner + (unsigned)jr;
            if (NA == 0 && (int64_t)r >= a.R) break;      // (the last group of a call without a sum may be short)
            const unsigned pr = r % a.prows;
            const float* tb = tab + (size_t)pr * DP_TAB;
            const uint64_t code = NA ? (uint64_t)m.sched[jr] : 0ull;
            const bool looks_back = tb[DP_LOOKBACK] != 0.0f;
            OsIn in;
            float cexcl[OS_SUB], ctotal[OS_SUB], ccarry = 0.0f;
            int ckind = 3;
            if ((NA != 0 && tb[DP_ONESHOT] != 0.0f) || looks_back) {   // uniform
                os_load<true>(a, x + row_off(a.xmap, r, 0), x + row_off(a.xmap, r, STEREO ? 1 : 0), true, tb, s, lane, in);
                OsMid cmid;
                os_scan<true>(a, in, tb, s, lane, cmid, looks_back ? lb.gran + (size_t)r * lb.ntiles : nullptr);
#pragma unroll
                for (int k = 0; k < OS_SUB; ++k) {
                    cexcl[k] = cmid.excl[k];
                    ctotal[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cmid.total[k])));
                }
                ccarry = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, cmid.carry)));
                ckind = looks_back ? 2 : 1;
            } else if (NA != 0 && ((unsigned)code & 15u) != 0u) {   // the row kernel's row: read back what it wrote
                const float* y0 = y + row_off(a.ymap, r, 0);
                const float* y1 = y + row_off(a.ymap, r, STEREO ? 1 : 0);
#pragma unroll
                for (int k = 0; k < OS_SUB; ++k) {
                    ld4<true>(y0, n0 + 256 * k, a.L, true, in.xa[k]);
                    if (STEREO) ld4<true>(y1, n0 + 256 * k, a.L, true, in.xb[k]);
                }
            }
            if (walked > 0) finish();
            ++walked;
#pragma unroll
            for (int k = 0; k < OS_SUB; ++k) {
#pragma unroll
                for (int i = 0; i < DE; ++i) {
                    pxa[k][i] = in.xa[k][i];
                    pxb[k][i] = in.xb[k][i];
                }
                pexcl[k] = cexcl[k];
                ptotal[k] = ctotal[k];
            }
            pcarry = ccarry;
            pkind = ckind;
            prow = r;
            pcode = code;
        }
        if (walked > 0) finish();
    }
    for (int e = m.n_pre; e < m.n_pre + m.n_post; ++e) extra(e);
}

}  // namespace gfx

using namespace gfx;

extern "C" {

size_t gfx_dynamics_ws_bytes(int64_t param_rows) {
    return param_rows <= 0 ? 0 : (size_t)param_rows * DP_TAB * sizeof(float);
}

// pole table | 16 control words (tickets, "some row looks back") | one 8-byte granule per row and 512-sample tile
static size_t dyn_lb_offset(int64_t param_rows) { return ((size_t)param_rows * DP_TAB * sizeof(float) + 255) & ~(size_t)255; }
size_t gfx_dynamics_ws_bytes_ex(int64_t param_rows, int64_t R, int64_t L) {
    if (param_rows <= 0 || R <= 0 || L <= 0) return 0;
    return dyn_lb_offset(param_rows) + 64 + (size_t)R * (size_t)((L + OS_WTILE - 1) / OS_WTILE) * 8;
}

static thread_local const char* t_dyn_last_kernel = "";   // see gfx_dynamics_last_kernel

static int dynamics_fused_launch(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* log_threshold,
                                 const float* log_ratio, const float* log_knee, const float* z_alpha, int64_t param_rows,
                                 int64_t R, int64_t C, int64_t L, int smoother, int64_t iir_len, int knee, int gate,
                                 float* u1, void* ws, size_t ws_bytes, void* stream, const MixArgs* mix, int mix_na = 0) {
    if (param_rows < 1 || param_rows > R) return GFX_EINVAL;
    if (u1 && smoother != 1) return GFX_EINVAL;
    if (!x || !y || !log_threshold || !log_ratio || R <= 0 || L <= 0 || (C != 1 && C != 2)) return GFX_EINVAL;
    if (knee < 0 || knee > 2 || (knee != 0 && !log_knee)) return GFX_EINVAL;
    if (smoother != 0 && smoother != 1) return GFX_EINVAL;
    if (smoother == 1 && (!z_alpha || iir_len < 1)) return GFX_EINVAL;
    if (R > 0x7fffffffLL) return GFX_EINVAL;
    if (ws && ws_bytes < gfx_dynamics_ws_bytes(param_rows)) return GFX_ENOSPC;
    DynArgs a;
    a.xmap = xmap; a.ymap = ymap; a.R = R; a.L = L; a.N = iir_len; a.C = (int)C;
    a.smoother = smoother; a.knee = knee; a.gate = gate;
    a.prows = (unsigned)param_rows;
    hipStream_t st = (hipStream_t)stream;
    const int64_t ntiles = (L + DTILE - 1) / DTILE;
    // With a workspace and a smoother: the pole table, then the dependency-free one-shot grid for the rows whose
    // history fits (decided per row on the device), then the row kernel for the others (same table, complementary test).
    const float* tab = nullptr;
    const int64_t ngroups = (L + OS_GTILE - 1) / OS_GTILE;
    // (tile grids: 8 runs of whole rows / graphs, one per XCD -- see lb_block_index)
    const bool oneshot = ws && smoother == 1 && L > OS_WTILE && (R + 8) * ngroups <= 0x7ffffff0LL;
    if (mix && !oneshot) return GFX_EINVAL;
    LbArgs lb = {nullptr, nullptr, 0, 0};
    auto tile_grid = [&](int64_t units) { return dim3((unsigned)(((units + 7) / 8) * ngroups * 8)); };
    if (oneshot) {
        float* t = (float*)ws;
        // the look-back walks move whole aligned float4 (as the fused routing sum does: its entry point checked already)
        const bool lb_ok = mix || (al16(x, xmap) && al16(y, ymap) && ((uintptr_t)u1 & 15) == 0 && (L & 3) == 0);
        if (lb_ok && ws_bytes >= gfx_dynamics_ws_bytes_ex(param_rows, R, L)) {   // room for the look-back granules: rows with
            char* base = (char*)ws + dyn_lb_offset(param_rows);                  // a long smoother memory stay on the tile grid
            lb.ctrl = (unsigned*)base;
            lb.gran = (unsigned long long*)(base + 64);
            lb.ntiles = (unsigned)((L + OS_WTILE - 1) / OS_WTILE);
            if (hipMemsetAsync(base, 0, 64 + (size_t)R * lb.ntiles * 8, st) != hipSuccess) return GFX_ELAUNCH;
        }
        hipLaunchKernelGGL(dyn_pole_table_kernel, dim3((unsigned)param_rows), dim3(64), 0, st, z_alpha, t, param_rows, iir_len,
                           lb.gran ? lb.ctrl + 8 : (unsigned*)nullptr);
        tab = t;
        if (!mix) {
            const unsigned nblocks = (unsigned)(R * ngroups);
            a.nchunks = 1;
            a.chunk_tiles = 1;
            const LbArgs none = {nullptr, nullptr, 0, 0};   // (look-back rows are produced by the row-group walk below)
            hipLaunchKernelGGL(dyn_oneshot_kernel, tile_grid(R), dim3(DT), 0, st, x, y, log_threshold,
                               log_ratio, log_knee, (const float*)t, a, (unsigned)ngroups, nblocks, u1, none);
        }
    }
    // Few rows: one workgroup per row walks the whole length serially (~2 us per tile) and the launch is bound by
    // that latency, not by bandwidth.  Split every row into time chunks then; a chunk re-scans N samples of history
    // (exact, the smoother is an N-tap FIR), so chunks are kept at least as long as that history.
    const int64_t warm = smoother == 1 ? (iir_len + DTILE - 1) / DTILE : 0;
    int64_t nchunks = 1;
    while (!u1 && R * nchunks < 2048 && nchunks < 16 && ntiles / (2 * nchunks) >= (warm > 4 ? warm : 4)) nchunks *= 2;
    a.nchunks = (int)nchunks;
    a.chunk_tiles = (ntiles + nchunks - 1) / nchunks;
    if (R * nchunks > 0x7fffffffLL) return GFX_EINVAL;
    hipLaunchKernelGGL(dyn_fused_kernel, dim3((unsigned)(R * nchunks)), dim3(DT), 0, st, x, y,
                       log_threshold, log_ratio, log_knee, z_alpha, a, u1, tab);
    if (!mix && lb.gran) {
        // look-back rows of a call without a routing sum: waves walk groups of 16 rows tile by tile, one row deferred (the
        // schedule of the fused sum without accumulators); leaves at once when the pole table found no such row
        constexpr int LB_GROUP = 16;
        const int64_t units = (R + LB_GROUP - 1) / LB_GROUP;
        const unsigned nblocks = (unsigned)(units * ngroups);
        MixArgs none;
        none.sched = nullptr; none.out = nullptr; none.sb = none.sv = none.sc = 0; none.inner = LB_GROUP;
        none.extras = nullptr; none.n_pre = none.n_post = 0; none.skip_rows = 0;
        a.nchunks = 1;
        a.chunk_tiles = 1;
        lb.split = 1;
        const dim3 grid = tile_grid(units), blk(DT);
        with_bool(C == 2, [&](auto stereo) {
            with_knee(knee, gate != 0, [&](auto kn, auto gt) {
                hipLaunchKernelGGL((dyn_oneshot_mix_kernel<0, stereo(), kn(), gt(), true>), grid, blk, 0, st, x, y, log_threshold,
                                   log_ratio, log_knee, tab, a, (unsigned)ngroups, nblocks, u1, none, lb);
            });
        });
    }
    if (mix) {   // after the row kernel: its rows are read back by the tiles that sum them
        const unsigned nblocks = (unsigned)((R / mix->inner) * ngroups);
        a.nchunks = 1;
        a.chunk_tiles = 1;
        const dim3 grid = tile_grid(R / mix->inner), blk(DT);
        // both forms of the walk when some row may look back (which one runs is decided on the device), else the plain one
        lb.split = lb.gran ? 1 : 0;
        with_bool(C == 2, [&](auto stereo) {
            with_knee(knee, gate != 0, [&](auto kn, auto gt) {
                auto walk = [&](auto na, auto defer) {
                    hipLaunchKernelGGL((dyn_oneshot_mix_kernel<na(), stereo(), kn(), gt(), defer()>), grid, blk, 0, st, x, y,
                                       log_threshold, log_ratio, log_knee, tab, a, (unsigned)ngroups, nblocks, u1, *mix, lb);
                };
                auto walks = [&](auto na) {
                    walk(na, std::false_type{});
                    if (lb.split) walk(na, std::true_type{});
                };
                if (mix_na <= 2) walks(std::integral_constant<int, 2>{});
                else walks(std::integral_constant<int, 4>{});
            });
        });
    }
    const int rc = GFX_LAUNCH_OK();
    // (a call without a routing sum whose workspace holds the look-back granules also launches the row-group walk,
    // dyn_oneshot_mix_kernel<0, ...>: which of the two produced the rows is decided on the device, so both are named)
    if (rc == GFX_OK)
        t_dyn_last_kernel = mix ? "dyn_oneshot_mix_kernel"
                                : (oneshot ? (lb.gran ? "dyn_oneshot_kernel+dyn_oneshot_mix_kernel" : "dyn_oneshot_kernel")
                                           : "dyn_fused_kernel");
    return rc;
}

const char* gfx_dynamics_last_kernel(void) { return t_dyn_last_kernel; }

int gfx_dynamics_fused_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* log_threshold,
                           const float* log_ratio, const float* log_knee, const float* z_alpha, int64_t param_rows,
                           int64_t R, int64_t C, int64_t L, int smoother, int64_t iir_len, int knee, int gate,
                           float* u1, void* ws, size_t ws_bytes, void* stream) {
    return dynamics_fused_launch(x, xmap, y, ymap, log_threshold, log_ratio, log_knee, z_alpha, param_rows, R, C, L, smoother,
                                 iir_len, knee, gate, u1, ws, ws_bytes, stream, nullptr);
}

int gfx_dynamics_fused_mix_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* log_threshold,
                               const float* log_ratio, const float* log_knee, const float* z_alpha, int64_t param_rows,
                               int64_t R, int64_t C, int64_t L, int smoother, int64_t iir_len, int knee, int gate,
                               float* u1, void* ws, size_t ws_bytes, const int64_t* sched, int64_t inner, int64_t n_acc,
                               float* mix, int64_t mix_sb, int64_t mix_sv, int64_t mix_sc, const int64_t* extras,
                               int64_t n_pre, int64_t n_post, int flags, void* stream) {
    if (!sched || !mix || inner < 1 || inner > 65535 || n_acc < 1 || n_acc > 4 || R % inner != 0 || !ws || smoother != 1)
        return GFX_EINVAL;
    if (n_pre < 0 || n_post < 0 || n_pre + n_post > 65535 || (n_pre + n_post > 0 && !extras)) return GFX_EINVAL;
    // every access of the fused kernel is a whole aligned float4 (the element-wise paths would triple its code size)
    const int64_t strides = xmap.stride_outer | xmap.stride_inner | xmap.stride_ch | ymap.stride_outer | ymap.stride_inner |
                            ymap.stride_ch | mix_sb | mix_sv | mix_sc;
    if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)mix | (uintptr_t)u1) & 15) != 0 || (strides & 3) != 0 || (L & 3) != 0)
        return GFX_EINVAL;
    MixArgs m;
    m.sched = sched; m.out = mix; m.sb = mix_sb; m.sv = mix_sv; m.sc = mix_sc; m.inner = (int)inner;
    m.extras = extras; m.n_pre = (int)n_pre; m.n_post = (int)n_post;
    m.skip_rows = (flags & GFX_MIX_SKIP_ROWS) ? 1 : 0;
    return dynamics_fused_launch(x, xmap, y, ymap, log_threshold, log_ratio, log_knee, z_alpha, param_rows, R, C, L, smoother,
                                 iir_len, knee, gate, u1, ws, ws_bytes, stream, &m, (int)n_acc);
}

}  // extern "C"

// The backward, the standalone stages and the ballistics adjoint are files of their own for the reader and part of this
// translation unit for the compiler.  Compiled alone, every call of load4() in them passes lo = 0; the compiler then folds
// that constant into load4() BEFORE it inlines it instead of after, and six kernels come out different (same register
// totals): measured on the MI355X against the one-file build, ballistics_bwd_kernel 5.10 -> 7.55 ms in chunks and 26.6 ->
// 44.1 ms in whole rows (9216 x 131072), onepole_kernel<true> 2.50 -> 2.52 ms, dyn_bwd_u1_kernel within the noise.  Here
// dyn_stream's run-time `lo` keeps load4() general until it is inlined and every kernel is the machine code it has been
// (tools/kernel_asm_diff.py).
#include "dynamics_bwd.hpp"
#include "dyn_elementwise.hpp"
#include "ballistics_bwd.hpp"
