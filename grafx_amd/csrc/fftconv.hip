// Overlap-save FIR convolution on LDS FFT tiles (gfx950).
//
// Replaces the reference's convolve() — core/convolution.py:119-134 — for the case where
// it equals a true linear convolution (P = L + N - 1 even; see DESIGN.md for the odd-P quirk,
// which is layered on top of the *full* convolution this file produces).
//
// Kernels
//   fftconv1_kernel N <= 8193: load x tile -> FFT -> x H -> IFFT -> store valid samples (fused)
//   xspec_kernel    N  > 8193: x window -> FFT -> split spectra (Xe, Xo pairs in thread layout) to HBM/L2
//   macinv_pair_kernel  N > 8193: two output tiles per 512-thread workgroup, sum_p X[i-p] * H[p] in registers -> 2 x IFFT -> store
//   macinv_kernel   the same with one output tile per 256-thread workgroup (GFX_SCHED_TILE)
//   winmac_kernel   one output tile per row: every window transformed and multiplied in place (fftconv_window_kernels.hpp)
//   gfx_fftconv_pipe_*  the hand-scheduled persistent form of fftconv1_kernel (generated assembly; fftconv_pipe.hip)
//   fftconv1_state_kernel / xspec_state_kernel / winmac_state_kernel: the window-loading kernels with the N - 1 samples
//                   before the row read from a carried history (streaming, gfx_fftconv_state_f32); the next history is
//                   history_tail_kernel's (common.hip)
//   corr1_kernel / gfx_corr_pipe (generated assembly): the filter gradient (gfx_fir_grad_f32).  Kept in this file because
//                   corr1_kernel compiles to other machine code in a file of its own (EXPERIMENTS.md).
// The filter spectra (hspec_kernel) are fir_spectrum.hip's; what the files share is fftconv_tile.hpp.
//
// Algorithmic bytes: 4*(C_in + C_out) per output frame per row (read x once, write y once);
// the tile overlap (N-1 of 16384 samples) is re-read through L2.
#include "fftconv_pipe.hpp"
#include "fftconv_tile.hpp"

namespace gfx {

// ------------------------------------------------------------------------------------------------
// window j of x starts at off - O + j * hop; windows that miss [0, L) are skipped.
__device__ __forceinline__ bool window_live(int64_t s, int64_t L) { return s + TILE_F > 0 && s < L; }

#define FC_STATE 0
#include "fftconv_window_kernels.hpp"   // fftconv1_kernel, xspec_kernel, winmac_kernel
#undef FC_STATE
#define FC_STATE 1
#include "fftconv_window_kernels.hpp"   // fftconv1_state_kernel, xspec_state_kernel, winmac_state_kernel
#undef FC_STATE

// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TILE_T, 2) void macinv_kernel(const float2* __restrict__ Zs, const float4* __restrict__ Hs,
                                                           float* __restrict__ y, ConvArgs a, int64_t nwin,
                                                           const float2* __restrict__ twtab,
                                                           uint32_t* __restrict__ rowmax = nullptr) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const unsigned lb = xcd_logical_block();
    if (lb >= (unsigned)a.nblocks) return;
    const unsigned ntiles = (unsigned)a.ntiles;
    const unsigned rco = lb / ntiles;
    const int64_t tile = lb - rco * ntiles;
    const unsigned r = rco / (unsigned)a.Cout;
    const int c = (int)(rco - r * (unsigned)a.Cout);
    float* yrow = y + row_off(a.ymap, r, c);
    const f4v* H = reinterpret_cast<const f4v*>(Hs) + ((int64_t)(r % a.hrows) * a.Cf + (a.Cf == 1 ? 0 : c)) * a.nparts * H_TILE_F4;
    const f4v* Z = reinterpret_cast<const f4v*>(Zs) + ((int64_t)r * a.Cin + (a.Cin == 1 ? 0 : c)) * nwin * H_TILE_F4;

    cx ye[H_SLOTS], yo[H_SLOTS];
#pragma unroll
    for (int s = 0; s < H_SLOTS; ++s) ye[s] = yo[s] = cx{0.0f, 0.0f};
    const cx wj = to_cx(twtab[TILE_T + t]);  // W_8192^t

    for (int p = 0; p < a.nparts; ++p) {
        const int64_t j = tile - p;
        if (!window_live(a.off - a.O + j * a.hop, a.L)) continue;
        // every operand of the turn requested up front (left to itself the compiler fetches each pair right before its
        // product and waits for it: 34 serialised trips to L2 per turn, 3.8 instead of 1.9 ms at cfg3)
        const rsrc_t zr = make_rsrc(Z + (j + a.nparts - 1) * H_TILE_F4, (int64_t)H_TILE_F4 * 16);
        const rsrc_t hr = make_rsrc(H + (int64_t)p * H_TILE_F4, (int64_t)H_TILE_F4 * 16);
        f4v xreg[H_SLOTS], hreg[H_SLOTS];
#pragma unroll
        for (int q = 0; q < H_SLOTS; ++q) {
            xreg[q] = buf_load_f4(zr, 16u * (uint32_t)t, 4096u * q);
            hreg[q] = buf_load_f4(hr, 16u * (uint32_t)t, 4096u * q);
        }
        __builtin_amdgcn_sched_barrier(0);
        for_each_pair(t, wj, [&](int slot, int, int, cx wk, bool) {
            pair_product_acc(xreg[slot].lo, xreg[slot].hi, hreg[slot], wk, ye[slot], yo[slot]);
        });
    }

    cx pz[2][16], v[32];
    for_each_pair(t, wj, [&](int slot, int ia, int ib, cx, bool self) {
        cx za, zb;
        pair_merge(ye[slot], yo[slot], za, zb);
        NAT(pz, ia) = za;
        if (!self) NAT(pz, ib) = zb;
    });
    TileTw tw;
    tile_twiddles(tw, twtab, t);
    tile_inverse(pz, v, tw, lds, t);
    store_valid(v, yrow, tile * a.V, a.O, a.Lout, t);
    if (rowmax) tile_rowmax(v, rowmax, rco, tile * a.V, a.O, a.Lout, t);
}

// ---- two consecutive output tiles per 512-thread workgroup ---------------------------------------------------------
// Output tiles i and i + 1 of a row meet the windows i + 1, i, ..., i + 1 - nparts; window i + 1 - k multiplies partition k
// for tile i + 1 and partition k - 1 for tile i.  One workgroup of two 256-thread groups walks those nparts + 1 windows:
// per turn it fetches ONE window spectrum and ONE filter partition (the other partition is the one of the turn before, kept
// in registers), i.e. (nparts + 1) + nparts tile-sized operands per tile PAIR where macinv_kernel fetches 2 nparts per tile
// (60 001 taps: 17 against 32) -- the loop is bound by what the CUs' L1 can take in, not by arithmetic.
// Registers decide the shape: two accumulator sets, a window and two partitions are 340 registers per thread for a
// 256-thread tile (round 4's first attempt, tools/experiments/r4_macinv2: spills, serialised loads, 1.6x slower).  Here
// the mirrored bin pairs of a thread are split between the two groups -- group G multiplies pairs 8G .. 8G + 7 of BOTH
// tiles -- so everything halves: 2 x 36 accumulators, 2 x 36 for two window sets (the running one and the next), 2 x 36
// for the partitions.  After the loop the groups swap halves through LDS (group 0 gets tile i complete, group 1 tile i + 1) and run
// the two inverse transforms side by side.  Every tile adds the same products in the same order as in macinv_kernel (equal
// to the last bit or two: the compiler contracts the twiddle arithmetic of the two kernels differently).
//
// Mirrored pairs of a group, the same straight-line code for every lane: slot i < 8 of group G is pair 8 G + i of threads
// t != 0 -- bins (row 0, k3) and (row 1, 15 - k3), k3 = 8 G + i, rows = the two butterflies bf of tile_forward's layout --
// and, for thread 0, whose bins pair up INSIDE a row, (row 0: k3 = i with 16 - i; i = 0 with itself) in group 0 and
// (row 1: k3 = i with 15 - i) in group 1; group 0 has a ninth slot for thread 0's self-paired bin (row 0, k3 = 8).  These
// are for_each_pair's slots, in which both the filter partitions (hspec_kernel) and the window spectra (xspec_kernel) are
// stored, so the difference is data, not control flow: a per-lane slot base in the load offset (thread 0 of group 1:
// slots 9.. instead of 8..), W^(t + 512 k3) from a per-lane base (thread 0 of group 1: W_32^17, so that base x
// W_32^(16 + 2 i) = W_32^(1 + 2 i), its pairs' factor), and selects where the finished halves are put into place.  A
// divergent branch for thread 0 would double the code and, worse, blur the compiler's wait counts at its join (every turn
// would start by waiting for all outstanding loads).
//
// Flat 16-entry layout of a group's half tile: e < 8 "lower" = row G, k3 = e;  e >= 8 "upper" = k3 = e of row
// (G == 0) == (t != 0).
template <int G>
__device__ __forceinline__ void macinv_pair_half(const f4v* __restrict__ Z, const f4v* __restrict__ H, const ConvArgs& a,
                                                 int64_t tile, bool two, int t, cx wj, cx* lds_other,
                                                 cx (&own)[16]) {
    constexpr int NS = G ? 8 : 9;
    cx aye[NS], ayo[NS], bye[NS], byo[NS];   // tile i ("a") and tile i + 1 ("b")
#pragma unroll
    for (int s = 0; s < NS; ++s) aye[s] = ayo[s] = bye[s] = byo[s] = cx{0.0f, 0.0f};

    const bool z = t == 0;
    // window and partition slots alike (16-byte entries, slot * 256 + t): group 1 multiplies slots 8.. (thread 0: 9..)
    const uint32_t hv = 16u * (uint32_t)(t + (G ? (z ? 9 : 8) * TILE_T : 0));
    const cx w32_17 = {-0.98078528040323044913f, 0.19509032201612826785f};
    const cx wbase = (G && z) ? w32_17 : wj;

    // turns k_lo .. k_hi: the windows tile + 1 - k that overlap the signal (window starts fall with k) and that one of the
    // two tiles uses (turn 0: tile i + 1 only, turn nparts: tile i only)
    const int64_t s0 = a.off - a.O + (tile + 1) * a.hop;                  // start of the window of turn 0
    int k_lo = two ? 0 : 1, k_hi = a.nparts;
    if (s0 >= a.L) k_lo = max(k_lo, (int)((s0 - a.L) / a.hop) + 1);       // first k with s0 - k hop < L
    if (s0 + TILE_F <= (int64_t)k_hi * a.hop) k_hi = (int)((s0 + TILE_F - 1) / a.hop);   // last k with s0 - k hop + TILE_F > 0

    // Operands come through two range-checked descriptors: the nparts partitions of this row's filter (partition k at
    // k * 68 KB: a request for partition nparts -- the last turn has none for tile i + 1 -- falls outside and reads as
    // zeros), and one window spectrum at a time (an empty descriptor for the turn after the last).  So every turn is
    // the same straight-line code, with no test around a load or a product.
    // (Tried and dropped: the turns in a cyclic order that makes all pairs of a row read the same window in the same turn
    // -- the L2 hit rate was not what held the loop back: 2.36 against 2.25 ms with xspec at cfg3, all nparts + 1 turns
    // taken by every pair.)
    const rsrc_t hr = make_rsrc(H, (int64_t)a.nparts * H_TILE_F4 * 16);
    auto window = [&](int k) {
        return make_rsrc(Z + (tile + 1 - k + a.nparts - 1) * H_TILE_F4, k <= k_hi ? (int64_t)H_TILE_F4 * 16 : 0);
    };
    // One turn: the window of turn k (w) times partition k - 1 (ha) for tile i, then times partition k (hb) for tile i + 1.
    // The operands of turn k + 1 are requested a full turn ahead, in two bursts: its window into the second window
    // register set at the start of the turn, its NEW partition (k + 1, tile i + 1's) into the registers of ha once all of
    // tile i's products are done -- so the next turn runs with (ha, hb) and the two window sets exchanged.  (Requests
    // slot by slot IN PLACE -- a slot's next operands into its own registers right after its products, no second window
    // set -- measured the same to 1.5 %: the loop is bound by what the address unit moves, not by when it is asked.)
    if (k_lo <= k_hi) {
        f4v w0[NS], w1[NS], h0[NS], h1[NS];
        auto req_w = [&](f4v (&w)[NS], int k) {
            const rsrc_t zr = window(k);
#pragma unroll
            for (int i = 0; i < NS; ++i) w[i] = buf_load_f4(zr, hv, 4096u * i);
        };
        auto req_h = [&](f4v (&h)[NS], int k) {   // k = -1 / nparts: outside the descriptor, zeros
            const uint32_t hoff = k < 0 ? 0x40000000u : (uint32_t)k * (uint32_t)(H_TILE_F4 * 16);
#pragma unroll
            for (int i = 0; i < NS; ++i) h[i] = buf_load_f4(hr, hv, hoff + 4096u * i);
        };
        auto bturn = [&](int k, f4v (&w)[NS], f4v (&wn)[NS], f4v (&ha)[NS], f4v (&hb)[NS]) {
            req_w(wn, k + 1);
            __builtin_amdgcn_sched_barrier(0);
            cx wjt = wbase;
            asm volatile("" : "+v"(wjt));   // the slots' W^(t + 512 k3) recomputed every turn (2 instructions each), not kept: 16 registers
#pragma unroll
            for (int i = 0; i < NS; ++i)
                pair_product_acc(w[i].lo, w[i].hi, ha[i], mul_w16(wjt, 8 * G + i), aye[i], ayo[i]);
            __builtin_amdgcn_sched_barrier(0);
            req_h(ha, k + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < NS; ++i)
                pair_product_acc(w[i].lo, w[i].hi, hb[i], mul_w16(wjt, 8 * G + i), bye[i], byo[i]);
            __builtin_amdgcn_sched_barrier(0);
        };
        req_h(h0, k_lo - 1);
        req_w(w0, k_lo);
        req_h(h1, k_lo);
        __builtin_amdgcn_sched_barrier(0);
        for (int k = k_lo; k <= k_hi; k += 2) {
            bturn(k, w0, w1, h0, h1);
            if (k + 1 <= k_hi) bturn(k + 1, w1, w0, h1, h0);
        }
    }

    // the finished half tiles in the flat layout: this group's half of ITS tile stays in registers (own), its half of the
    // other group's tile goes through LDS
    auto place = [&](const cx (&ye)[NS], const cx (&yo)[NS], cx (&flat)[16]) {
        cx za[NS], zb[NS];
#pragma unroll
        for (int i = 0; i < NS; ++i) pair_merge(ye[i], yo[i], za[i], zb[i]);
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            if (G == 0) {
                flat[j] = za[j];
                flat[8 + j] = z ? (j == 0 ? za[NS - 1] : zb[8 - j]) : zb[7 - j];
            } else {
                flat[j] = z ? za[j] : zb[7 - j];
                flat[8 + j] = z ? zb[7 - j] : za[j];
            }
        }
    };
    cx other[16];
    if (G == 0) {
        place(aye, ayo, own);
        place(bye, byo, other);
    } else {
        place(bye, byo, own);
        place(aye, ayo, other);
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) lds_other[e * TILE_T + t] = other[e];
}

// own / got: the flat rows of this group's pairs and of the other group's (see above) -> the [2][16] layout tile_inverse takes
template <int G>
__device__ __forceinline__ void macinv_pair_gather(const cx (&own)[16], const cx* lds_mine, int t, cx (&pz)[2][16]) {
    cx got[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) got[e] = lds_mine[e * TILE_T + t];
    const bool z = t == 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        pz[G][brev(i, 4)] = own[i];
        pz[1 - G][brev(i, 4)] = got[i];
        // upper halves: own is row (G == 0) == (t != 0), got the other one
        const cx up_own = own[8 + i], up_got = got[8 + i];
        const bool own_is_row1 = (G == 0) != z;
        pz[1][brev(8 + i, 4)] = own_is_row1 ? up_own : up_got;
        pz[0][brev(8 + i, 4)] = own_is_row1 ? up_got : up_own;
    }
}

__global__ __launch_bounds__(2 * TILE_T, 1) void macinv_pair_kernel(const float2* __restrict__ Zs,
                                                                    const float4* __restrict__ Hs,
                                                                    float* __restrict__ y, ConvArgs a, int64_t nwin,
                                                                    const float2* __restrict__ twtab,
                                                                    uint32_t* __restrict__ rowmax = nullptr) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x & (TILE_T - 1);
    const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
    const unsigned lb = xcd_logical_block();
    if (lb >= (unsigned)a.nblocks) return;
    const unsigned npairs = (unsigned)((a.ntiles + 1) >> 1);
    const unsigned rco = lb / npairs;
    const int64_t tile = 2 * (int64_t)(lb - rco * npairs);
    const bool two = tile + 1 < a.ntiles;
    const unsigned r = rco / (unsigned)a.Cout;
    const int c = (int)(rco - r * (unsigned)a.Cout);
    float* yrow = y + row_off(a.ymap, r, c);
    const f4v* H = reinterpret_cast<const f4v*>(Hs) + ((int64_t)(r % a.hrows) * a.Cf + (a.Cf == 1 ? 0 : c)) * a.nparts * H_TILE_F4;
    const f4v* Z = reinterpret_cast<const f4v*>(Zs) + ((int64_t)r * a.Cin + (a.Cin == 1 ? 0 : c)) * nwin * H_TILE_F4;
    const cx wj = to_cx(twtab[TILE_T + t]);  // W_8192^t
    cx* lds_mine = lds + grp * TILE_LDS_F2;
    cx* lds_other = lds + (1 - grp) * TILE_LDS_F2;

    cx own[16], pz[2][16], v[32];
    if (grp == 0) macinv_pair_half<0>(Z, H, a, tile, two, t, wj, lds_other, own);
    else macinv_pair_half<1>(Z, H, a, tile, two, t, wj, lds_other, own);
    __syncthreads();
    if (grp == 0) macinv_pair_gather<0>(own, lds_mine, t, pz);
    else macinv_pair_gather<1>(own, lds_mine, t, pz);
    __syncthreads();
    TileTw tw;
    tile_twiddles(tw, twtab, t);
    tile_inverse(pz, v, tw, lds_mine, t);
    if (grp == 0 || two) store_valid(v, yrow, (tile + grp) * a.V, a.O, a.Lout, t);
    if (rowmax && (grp == 0 || two)) tile_rowmax(v, rowmax, rco, (tile + grp) * a.V, a.O, a.Lout, t);
}

// Filter gradient of the short-filter convolution, gh[r,c,k] = sum_n g[r,cg,n] x[r,cx,n+off-k], k < N <= 8193, as a
// tile-wise circular correlation: per tile i the V-sample slice x[iV, iV+V) (zero-padded to the tile) is correlated with
// the window g[iV-off, iV-off+16384) -- C = conj(X) G, written with the same polyphase product as the convolution
// (he = conj(Xe), ho = conj(Xo) conj(W^k)) -- summed over the tiles of the row; the first N lags of the inverse
// transform are the gradient.  x and g are read exactly once and nothing else touches memory (the partitioned form
// writes and re-reads 12.5 GB of spectra at the console sizes).
// The tiles are summed in the FREQUENCY domain: conj(X_i) G_i is accumulated over the tiles of the row in registers
// (68 VGPRs of polyphase accumulators) and inverse-transformed once per row -- two transforms per tile.  The twiddles are
// re-fetched for every transform (L2-resident table) instead of being held, which is what lets the accumulators fit
// (256 VGPRs + 160 B of scratch; summing the inverse transforms of every tile in the output row instead -- three
// transforms per tile, no accumulator registers -- is 9 % slower: 8.0 vs 7.3 ms at 8192 rows).
__global__ __launch_bounds__(TILE_T, 2) void corr1_kernel(const float* __restrict__ x, const float* __restrict__ g,
                                                           float* __restrict__ gh, CorrArgs a,
                                                           const float2* __restrict__ twtab) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const unsigned rco = xcd_logical_block();
    if (rco >= (unsigned)a.nblocks) return;
    const unsigned r = rco / (unsigned)a.Cout;
    const int c = (int)(rco - r * (unsigned)a.Cout);
    const float* xrow = x + row_off(a.xmap, r, a.Cx == 1 ? 0 : c);
    const float* grow = g + row_off(a.gmap, r, a.Cg == 1 ? 0 : c);
    const cx wj = to_cx(twtab[TILE_T + t]);  // W_8192^t
    const float sc = 1.0f / (4.0f * TILE_M);
    cx ye[H_SLOTS], yo[H_SLOTS];
#pragma unroll
    for (int q = 0; q < H_SLOTS; ++q) ye[q] = yo[q] = cx{0.0f, 0.0f};
    auto fresh_twiddles = [&](TileTw& tw) {
        int tt = t;
        asm volatile("" : "+v"(tt));  // a new load every time: the compiler must not keep 32 VGPRs of twiddles alive
        tile_twiddles(tw, twtab, tt);
    };
    for (int64_t i = 0; i < a.ntiles; ++i) {
        const int64_t s = i * a.V;
        f4v hreg[H_SLOTS];
        {
            cx v[32], w[2][16];
            TileTw tw;
            const int64_t xend = s + a.V < a.L ? s + a.V : a.L;
            load_window<false>(v, xrow, s, xend, t, 1.0f);   // (the two-form loader costs this kernel 500 B of scratch)
            fresh_twiddles(tw);
            tile_forward(v, w, tw, lds, t);
            for_each_pair(t, wj, [&](int slot, int ia, int ib, cx wk, bool) {
                cx xe, xo;
                pair_split(NAT(w, ia), NAT(w, ib), xe, xo);
                hreg[slot] = __builtin_shufflevector(cconj(xe) * sc, cmulc(cconj(xo), wk) * sc, 0, 1, 2, 3);
            });
        }
        __syncthreads();  // S2 reads of the x transform are done before the g transform's S1 writes
        {
            cx v[32], w[2][16];
            TileTw tw;
            load_window<false>(v, grow, s - a.off, a.Lg, t, 1.0f);
            fresh_twiddles(tw);
            tile_forward(v, w, tw, lds, t);
            for_each_pair(t, wj, [&](int slot, int ia, int ib, cx wk, bool) {
                cx ge, go;
                pair_split(NAT(w, ia), NAT(w, ib), ge, go);
                pair_product_acc(ge, go, hreg[slot], wk, ye[slot], yo[slot]);
            });
        }
        __syncthreads();
    }
    cx pz[2][16], v[32];
    for_each_pair(t, wj, [&](int slot, int ia, int ib, cx, bool self) {
        cx za, zb;
        pair_merge(ye[slot], yo[slot], za, zb);
        NAT(pz, ia) = za;
        if (!self) NAT(pz, ib) = zb;
    });
    TileTw tw;
    fresh_twiddles(tw);
    tile_inverse(pz, v, tw, lds, t);
    store_valid(v, gh + ((int64_t)r * a.Cout + c) * a.N, 0, 0, a.N, t);
}

static thread_local const char* t_last_kernel = "";   // see gfx_fftconv_last_kernel

// One launch of fftconv_sched on pad8(nblocks) workgroups, through launch() of common.hpp (the LDS opt-in, the launch, its
// check).  On success `name` (unless null) is what gfx_fftconv_last_kernel returns.  Every launch of this file's kernels goes
// through here, so none runs without its opt-in.
template <typename K, typename... Args>
static int launch_tile(K kernel, const char* name, int64_t nblocks, unsigned threads, size_t lds, hipStream_t st, Args... args) {
    if (launch(kernel, dim3(pad8(nblocks)), dim3(threads), lds, st, args...) != GFX_OK) return GFX_ELAUNCH;
    if (name) t_last_kernel = name;
    return GFX_OK;
}

// state_call (gfx_fftconv_state_f32): never the persistent kernels; zi: the rows' carried history (NULL: silence, which is
// what the stateless kernels compute)
static int fftconv_sched(const float* x, gfx_rowmap_t xmap, const void* Hs, int64_t h_rows, int64_t part_len, float* y,
                         gfx_rowmap_t ymap, float* xcopy, gfx_rowmap_t cmap, int64_t R, int64_t C_in, int64_t C_f,
                         int64_t L, int64_t Lout, int64_t off, int64_t N, void* ws, size_t ws_bytes, int schedule,
                         void* stream, uint32_t* rowmax, int* rowmax_written, bool state_call, const float* zi) {
    if (schedule != GFX_SCHED_AUTO && schedule != GFX_SCHED_TILE && schedule != GFX_SCHED_PIPE) return GFX_EINVAL;
    if (!x || !Hs || !y || R <= 0 || L <= 0 || Lout <= 0 || N <= 0) return GFX_EINVAL;
    if (h_rows < 1 || h_rows > R || h_rows > 0x7fffffffLL) return GFX_EINVAL;
    if (xcopy && (off != 0 || Lout < L || C_in < C_f || N > TILE_M + 1 || cmap.inner <= 0 || cmap.inner > 0x7fffffffLL))
        return GFX_EINVAL;
    if (C_in < 1 || C_f < 1 || (C_in != C_f && C_in != 1 && C_f != 1)) return GFX_EINVAL;
    if (xmap.inner <= 0 || ymap.inner <= 0 || xmap.inner > 0x7fffffffLL || ymap.inner > 0x7fffffffLL) return GFX_EINVAL;
    const ConvGeom g = conv_geom(N, Lout, part_len);
    if (!g.ok) return GFX_EINVAL;
    ConvArgs a;
    a.xmap = xmap; a.ymap = ymap; a.cmap = cmap;
    a.hrows = (unsigned)h_rows;
    a.L = L; a.Lout = Lout; a.off = off;
    a.O = g.O; a.V = g.V; a.hop = g.hop; a.ntiles = g.ntiles; a.nparts = (int)g.nparts;
    a.Cin = (int)C_in; a.Cf = (int)C_f; a.Cout = (int)(C_in > C_f ? C_in : C_f);
    a.nblocks = R * a.Cout * g.ntiles;
    if (a.nblocks > 0x7ffffff0LL) return GFX_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const float2* tw = tile_twiddle_table(st);
    if (!tw) return GFX_ELAUNCH;

    // the persistent hand-scheduled kernel: by name, or by AUTO once a launch is large enough to fill its pipeline
    PipeModule* pm = pipe_module();   // (loaded on the first call on a device, whatever the schedule: never mid-capture)
    if (schedule == GFX_SCHED_AUTO && auto_schedule() != GFX_SCHED_AUTO) schedule = auto_schedule();
    if (state_call && schedule == GFX_SCHED_PIPE) schedule = GFX_SCHED_AUTO;   // (the override only steers what can be steered)
    const int pv = pm && !state_call ? pipe_variant(a, g, xcopy != nullptr, N) : -1;
    if (schedule == GFX_SCHED_PIPE && pv < 0) {
        if (auto_schedule() == GFX_SCHED_PIPE) schedule = GFX_SCHED_TILE;   // the override only steers what can be steered
        else return GFX_EINVAL;
    }
    if (schedule == GFX_SCHED_PIPE || (schedule == GFX_SCHED_AUTO && pv >= 0 && a.nblocks >= 16 * pipe_cus(pm))) {
        // (the shipped code object is generated without the rowmax knob: this kernel takes even output lengths only, and the
        // one consumer of the maxima -- the odd-length aliasing -- has an odd one)
        const int rc = launch_pipe(pm, pv, x, Hs, y, xcopy, a, tw, st);
        if (rc == GFX_OK) t_last_kernel = pipe_variant_name(pv);
        return rc;
    }
    const float4* H4 = (const float4*)Hs;
    float* const no_copy = nullptr;
    uint32_t* const no_rowmax = nullptr;
    int rc;
    if (g.nparts == 1) {
        if (zi)
            return launch_tile(fftconv1_state_kernel<false>, "fftconv1_state_kernel<false>", a.nblocks, TILE_T, TILE_LDS_BYTES, st,
                               x, H4, y, no_copy, a, tw, no_rowmax, zi, N);
        if (xcopy)
            rc = launch_tile(fftconv1_kernel<true>, "fftconv1_kernel<true>", a.nblocks, TILE_T, TILE_LDS_BYTES, st, x, H4, y,
                             xcopy, a, tw, rowmax);
        else
            rc = launch_tile(fftconv1_kernel<false>, "fftconv1_kernel<false>", a.nblocks, TILE_T, TILE_LDS_BYTES, st, x, H4, y,
                             no_copy, a, tw, rowmax);
        if (rc == GFX_OK && rowmax && rowmax_written) *rowmax_written = 1;
        return rc;
    }
    if (g.ntiles == 1) {
        if (zi)
            return launch_tile(winmac_state_kernel, "winmac_state_kernel", a.nblocks, TILE_T, TILE_LDS_BYTES, st, x, H4, y, a, tw,
                               zi, N);
        return launch_tile(winmac_kernel, "winmac_kernel", a.nblocks, TILE_T, TILE_LDS_BYTES, st, x, H4, y, a, tw);
    }
    const int64_t nwin = g.ntiles + g.nparts - 1;
    const size_t need = (size_t)R * C_in * nwin * H_TILE_F4 * sizeof(float4);
    if (!ws || ws_bytes < need) return GFX_ENOSPC;
    ConvArgs ax = a;
    ax.nblocks = R * C_in * nwin;
    if (ax.nblocks > 0x7ffffff0LL) return GFX_EINVAL;
    // (the name of the pair of launches is set by the second one)
    if (zi) {
        rc = launch_tile(xspec_state_kernel, nullptr, ax.nblocks, TILE_T, TILE_LDS_BYTES, st, x, (float2*)ws, ax, nwin, tw, zi, N);
        // The product kernels consume spectra and know the signal only through which windows exist.  With a history every
        // window that starts before the row end does (xspec_body), which is what they compute for a signal that begins
        // nparts hops earlier: the same kernels, told off = nparts * hop and L + nparts * hop.  (They use off and L for
        // nothing else; rows, tiles and stores go by Lout, O and V.)
        a.off += (int64_t)g.nparts * g.hop;
        a.L += (int64_t)g.nparts * g.hop;
    } else {
        rc = launch_tile(xspec_kernel, nullptr, ax.nblocks, TILE_T, TILE_LDS_BYTES, st, x, (float2*)ws, ax, nwin, tw);
    }
    if (rc != GFX_OK) return rc;
    // (the pair kernel asks for "partition -1" at byte offset 0x40000000 and counts on the descriptor's range check to
    // return zeros: the filter's partitions must end below that offset -- ~126 M taps; longer filters take macinv_kernel)
    if (schedule != GFX_SCHED_TILE && (int64_t)(g.nparts + 1) * H_TILE_F4 * 16 < 0x40000000LL) {
        // two consecutive output tiles per 512-thread workgroup: each window spectrum and filter partition fetched once a pair
        ConvArgs ap = a;
        ap.nblocks = R * a.Cout * ((g.ntiles + 1) / 2);
        rc = launch_tile(macinv_pair_kernel, zi ? "xspec_state_kernel+macinv_pair_kernel" : "xspec_kernel+macinv_pair_kernel",
                         ap.nblocks, 2 * TILE_T, 2 * TILE_LDS_BYTES, st, (const float2*)ws, H4, y, ap, nwin, tw, rowmax);
    } else {
        rc = launch_tile(macinv_kernel, zi ? "xspec_state_kernel+macinv_kernel" : "xspec_kernel+macinv_kernel", a.nblocks, TILE_T,
                         TILE_LDS_BYTES, st, (const float2*)ws, H4, y, a, nwin, tw, rowmax);
    }
    if (rc == GFX_OK && rowmax && rowmax_written) *rowmax_written = 1;
    return rc;
}

}  // namespace gfx

using namespace gfx;

extern "C" {

int64_t gfx_fftconv_nparts(int64_t N) { return N <= 0 ? 0 : conv_geom(N, 1).nparts; }

int64_t gfx_fftconv_part_len(int64_t N, int64_t Lout) {
    if (N <= TILE_M + 1 || Lout <= 0 || Lout > TILE_M - 2) return 0;  // default geometry
    return (TILE_F - Lout) & ~int64_t(1);
}

size_t gfx_fftconv_workspace_bytes(int64_t R, int64_t C_in, int64_t L, int64_t Lout, int64_t off, int64_t N,
                                   int64_t part_len) {
    (void)L;
    (void)off;
    if (R <= 0 || N <= 0 || Lout <= 0) return 0;
    const ConvGeom g = conv_geom(N, Lout, part_len);
    if (!g.ok || g.nparts == 1 || g.ntiles == 1) return 0;  // one output tile: windows are transformed in place
    return (size_t)R * C_in * (g.ntiles + g.nparts - 1) * H_TILE_F4 * sizeof(float4);
}

int gfx_fftconv_f32(const float* x, gfx_rowmap_t xmap, const void* Hs, int64_t h_rows, int64_t part_len, float* y,
                    gfx_rowmap_t ymap, float* xcopy, gfx_rowmap_t cmap, int64_t R, int64_t C_in, int64_t C_f, int64_t L,
                    int64_t Lout, int64_t off, int64_t N, void* ws, size_t ws_bytes, int schedule, uint32_t* rowmax,
                    int* rowmax_written, void* stream) {
    if (!rowmax != !rowmax_written || (rowmax && schedule != GFX_SCHED_AUTO)) return GFX_EINVAL;
    if (rowmax_written) *rowmax_written = 0;
    return fftconv_sched(x, xmap, Hs, h_rows, part_len, y, ymap, xcopy, cmap, R, C_in, C_f, L, Lout, off, N, ws, ws_bytes,
                         schedule, stream, rowmax, rowmax_written, false, nullptr);
}

int gfx_fftconv_state_f32(const float* x, gfx_rowmap_t xmap, const void* Hs, int64_t h_rows, float* y, gfx_rowmap_t ymap,
                          const float* zi, float* zf, int64_t R, int64_t C_in, int64_t C_f, int64_t L, int64_t N, void* ws,
                          size_t ws_bytes, int schedule, void* stream) {
    if (schedule != GFX_SCHED_AUTO && schedule != GFX_SCHED_TILE) return GFX_EINVAL;
    if (R <= 0 || C_in < 1 || L <= 0 || N <= 0) return GFX_EINVAL;
    const int64_t H = N - 1;                                   // samples of state per row-channel
    if (H == 0) zi = nullptr, zf = nullptr;                    // one tap: no memory
    if (H >= (int64_t(1) << 29)) return GFX_EINVAL;            // the history is addressed by 32-bit byte offsets
    // the state is written while the history may still be read
    if (zi && zf && ranges_meet(zi, R * C_in * H, zf, R * C_in * H)) return GFX_EINVAL;
    if (zf && history_tail_blocks(R, C_in, H) > MAX_GRID_X) return GFX_EINVAL;
    const gfx_rowmap_t none = {1, 0, 0, 0};
    const int rc = fftconv_sched(x, xmap, Hs, h_rows, 0, y, ymap, nullptr, none, R, C_in, C_f, L, L, 0, N, ws, ws_bytes,
                                 schedule, stream, nullptr, nullptr, true, zi);
    if (rc != GFX_OK || !zf) return rc;
    return launch_history_tail(x, xmap, zi, zf, R, C_in, L, H, nullptr, nullptr, (hipStream_t)stream);
}

const char* gfx_fftconv_last_kernel(void) { return t_last_kernel; }

int gfx_fir_grad_f32(const float* x, gfx_rowmap_t xmap, const float* g, gfx_rowmap_t gmap, float* gh, int64_t R,
                     int64_t C_x, int64_t C_g, int64_t L, int64_t Lg, int64_t N, int64_t off, void* stream) {
    if (!x || !g || !gh || R <= 0 || L <= 0 || Lg <= 0 || N <= 0 || N > TILE_M + 1) return GFX_EINVAL;
    if (C_x < 1 || C_g < 1 || (C_x != C_g && C_x != 1 && C_g != 1)) return GFX_EINVAL;
    if (xmap.inner <= 0 || gmap.inner <= 0 || xmap.inner > 0x7fffffffLL || gmap.inner > 0x7fffffffLL) return GFX_EINVAL;
    if (off < -TILE_M || off > TILE_M) return GFX_EINVAL;  // |window start - tile start| stays within the 32-bit clip math
    CorrArgs a;
    a.xmap = xmap; a.gmap = gmap;
    a.L = L; a.Lg = Lg; a.off = off; a.N = N;
    a.V = TILE_F - (N & ~int64_t(1));  // tile slice: V + N - 1 <= 16384, V even
    a.ntiles = (L + a.V - 1) / a.V;
    a.Cx = (int)C_x; a.Cg = (int)C_g; a.Cout = (int)(C_x > C_g ? C_x : C_g);
    a.nblocks = R * a.Cout;
    if (a.nblocks > 0x7ffffff0LL) return GFX_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const float2* tw = tile_twiddle_table(st);
    if (!tw) return GFX_ELAUNCH;
    PipeModule* pm = pipe_module();
    if (pm && corr_pipe_ok(a) && auto_schedule() != GFX_SCHED_TILE) return launch_corr_pipe(pm, x, g, gh, a, tw, st);
    if (allow_lds(corr1_kernel, TILE_LDS_BYTES)) return GFX_ELAUNCH;
    hipLaunchKernelGGL(corr1_kernel, dim3(pad8(a.nblocks)), dim3(TILE_T), TILE_LDS_BYTES, st, x, g, gh, a, tw);
    return hipGetLastError() == hipSuccess ? GFX_OK : GFX_ELAUNCH;
}

}  // extern "C"
