// The three compiler-built kernels of fftconv.hip that load signal windows -- fftconv1_kernel, xspec_kernel, winmac_kernel --
// as text that fftconv.hip includes twice: FC_STATE 0 gives the stateless kernels, FC_STATE 1 their twins that read the
// N - 1 samples before the row from a carried history zi (R, C_in, N - 1) instead of taking them as zeros
// (fftconv1_state_kernel, xspec_state_kernel, winmac_state_kernel; gfx_fftconv_state_f32: off = 0, Lout = L).  Two
// inclusions rather than a template parameter or a shared body function because the stateless kernels must stay
// instruction for instruction what they were (tools/kernel_asm_diff.py): inlined from a function, the same source came
// out of the optimiser a few instructions different (as csrc/biquad_kernel.hpp found before).
#ifndef FC_STATE
#error "fftconv_window_kernels.hpp is kernel text of fftconv.hip: define FC_STATE to 0 or 1 before including it"
#endif
#undef FC_KERNEL
#undef FC_STATE_PARAMS
#if FC_STATE
#define FC_KERNEL(name) name##_state_kernel
#define FC_STATE_PARAMS , const float* __restrict__ zi = nullptr, int64_t N = 0
#else
#define FC_KERNEL(name) name##_kernel
#define FC_STATE_PARAMS
#endif

// ------------------------------------------------------------------------------------------------
template <bool TEE>
__global__ __launch_bounds__(TILE_T, 2) void FC_KERNEL(fftconv1)(const float* __restrict__ x, const float4* __restrict__ Hs,
                                                             float* __restrict__ y, float* __restrict__ xcopy,
                                                             ConvArgs a, const float2* __restrict__ twtab,
                                                             uint32_t* __restrict__ rowmax = nullptr FC_STATE_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const unsigned lb = xcd_logical_block();
    if (lb >= (unsigned)a.nblocks) return;
    const unsigned ntiles = (unsigned)a.ntiles;
    const unsigned rco = lb / ntiles;
    const int64_t tile = lb - rco * ntiles;
    const unsigned r = rco / (unsigned)a.Cout;
    const int c = (int)(rco - r * (unsigned)a.Cout);
    const float* xrow = x + row_off(a.xmap, r, a.Cin == 1 ? 0 : c);
    float* yrow = y + row_off(a.ymap, r, c);
    const rsrc_t H = make_rsrc(Hs + ((int64_t)(r % a.hrows) * a.Cf + (a.Cf == 1 ? 0 : c)) * H_TILE_F4, H_TILE_F4 * 16);

    // Every global load of the tile is issued up front: the window, the twiddles, and the filter spectrum
    // (needed only after the forward transform, by which time it has long arrived).  Left to itself the
    // compiler issues each spectrum load right before its use and waits for it: 16 serialised L2 round trips.
    TileTw tw;
    cx v[32], w[2][16];
    f4v hreg[H_SLOTS];
#if FC_STATE   // (only the first tile starts before the row)
    load_window_hist(v, xrow, zi + ((int64_t)r * a.Cin + (a.Cin == 1 ? 0 : c)) * (N - 1), tile * a.V - a.O, a.L, N, t);
#else
    load_window(v, xrow, a.off + tile * a.V - a.O, a.L, t, 1.0f);
#endif
    tile_twiddles(tw, twtab, t);
#pragma unroll
    for (int q = 0; q < H_SLOTS; ++q) hreg[q] = buf_load_f4(H, 16u * (uint32_t)t, 4096u * q);
    __builtin_amdgcn_sched_barrier(0);
    // off == 0 here: the window's valid part is x[tile*V, tile*V + V) itself
    if (TEE) store_valid<true>(v, xcopy + row_off(a.cmap, r, c), tile * a.V, a.O, a.L, t);
    tile_forward(v, w, tw, lds, t);
    for_each_pair(t, tw.base(), [&](int slot, int ia, int ib, cx wk, bool self) {
        cx xe, xo, ye, yo, za, zb;
        pair_split(NAT(w, ia), NAT(w, ib), xe, xo);
        pair_product(xe, xo, hreg[slot], wk, ye, yo);
        pair_merge(ye, yo, za, zb);
        NAT(w, ia) = za;
        if (!self) NAT(w, ib) = zb;
    });
    // no barrier here: the inverse starts by writing S2 rows j = t and 512 - t, the very rows (and the only rows)
    // this thread read at the end of the forward transform -- nobody else touches them in between
    tile_inverse(w, v, tw, lds, t);
    store_valid(v, yrow, tile * a.V, a.O, a.Lout, t);
    if (rowmax) tile_rowmax(v, rowmax, rco, tile * a.V, a.O, a.Lout, t);   // (see tile_rowmax)
}

// ------------------------------------------------------------------------------------------------
// window j (j = jj - (nparts-1)) of x starts at off - O + j*V; windows that miss [0, L) are skipped.
__global__ __launch_bounds__(TILE_T, 2) void FC_KERNEL(xspec)(const float* __restrict__ x, float2* __restrict__ Zs,
                                                          ConvArgs a, int64_t nwin,
                                                          const float2* __restrict__ twtab FC_STATE_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const unsigned lb = xcd_logical_block();
    if (lb >= (unsigned)a.nblocks) return;
    const unsigned rcx = lb / (unsigned)nwin;
    const int64_t jj = lb - rcx * (unsigned)nwin;
    const int64_t s = a.off - a.O + (jj - (a.nparts - 1)) * a.hop;
#if FC_STATE
    // the earliest window, [-nparts * 8192, -(nparts - 2) * 8192), still reaches the history, which goes back to
    // -(N - 1) <= -(nparts - 1) * 8192: every window that starts before the row end holds samples
    if (s >= a.L) return;
#else
    if (!window_live(s, a.L)) return;
#endif
    const unsigned xr = rcx / (unsigned)a.Cin;
    const float* xrow = x + row_off(a.xmap, xr, (int)(rcx - xr * (unsigned)a.Cin));
    TileTw tw;
    cx v[32], w[2][16];
#if FC_STATE
    load_window_hist(v, xrow, zi + (int64_t)rcx * (N - 1), s, a.L, N, t);
#else
    load_window(v, xrow, s, a.L, t, 1.0f);
#endif
    tile_twiddles(tw, twtab, t);
    tile_forward(v, w, tw, lds, t);
    // stored the way the filter spectra are: per mirrored bin pair one 16-byte entry (Xe, Xo) at [slot][t] (the seventeenth
    // slot: thread 0 only), already split -- the product kernels fetch a pair with ONE instruction where two 8-byte rows
    // cost the CU's address unit twice as much (a vector-memory instruction occupies it ~22 cycles whatever its width, and
    // that is what bounds their loop), and thread 0's different pairing is settled here, once, instead of in every turn.
    f4v* out = reinterpret_cast<f4v*>(Zs) + (int64_t)lb * H_TILE_F4;
    for_each_pair(t, tw.base(), [&](int slot, int ia, int ib, cx, bool) {
        cx xe, xo;
        pair_split(NAT(w, ia), NAT(w, ib), xe, xo);
        // (streamed: the product kernel starts after ALL windows are written, by when only the last tenth is still in
        // a cache -- cfg3 2.05 -> 2.02 ms with the product kernel)
        __builtin_nontemporal_store(__builtin_shufflevector(xe, xo, 0, 1, 2, 3), &out[slot * TILE_T + t]);
    });
}

// One output tile per row (ntiles == 1, the filter-gradient shape: a long "filter", few outputs): every signal window
// meets exactly one filter partition, so its spectrum is used once -- transform it here instead of writing it to
// a workspace (xspec_kernel) and reading it back (macinv_kernel).
__global__ __launch_bounds__(TILE_T, 2) void FC_KERNEL(winmac)(const float* __restrict__ x, const float4* __restrict__ Hs,
                                                           float* __restrict__ y, ConvArgs a,
                                                           const float2* __restrict__ twtab FC_STATE_PARAMS) {
    extern __shared__ __attribute__((aligned(16))) cx lds[];
    const int t = threadIdx.x;
    const unsigned rco = xcd_logical_block();
    if (rco >= (unsigned)a.nblocks) return;
    const unsigned r = rco / (unsigned)a.Cout;
    const int c = (int)(rco - r * (unsigned)a.Cout);
    const float* xrow = x + row_off(a.xmap, r, a.Cin == 1 ? 0 : c);
    float* yrow = y + row_off(a.ymap, r, c);
    const f4v* H = reinterpret_cast<const f4v*>(Hs) + ((int64_t)(r % a.hrows) * a.Cf + (a.Cf == 1 ? 0 : c)) * a.nparts * H_TILE_F4;

    cx ye[H_SLOTS], yo[H_SLOTS];
#pragma unroll
    for (int s = 0; s < H_SLOTS; ++s) ye[s] = yo[s] = cx{0.0f, 0.0f};
    TileTw tw;
    tile_twiddles(tw, twtab, t);
    for (int p = 0; p < a.nparts; ++p) {
        const int64_t s = a.off - a.O - (int64_t)p * a.hop;  // window of partition p for output tile 0
#if !FC_STATE   // (with a history -- the streaming case proper: a short block, a long filter -- the window of every
        // partition holds samples, see the spectrum kernel above: every partition takes its turn; s < 0 <= L)
        if (!window_live(s, a.L)) continue;
#endif
        const f4v* Hp = H + (int64_t)p * H_TILE_F4;
        cx v[32], w[2][16];
#if FC_STATE
        load_window_hist(v, xrow, zi + ((int64_t)r * a.Cin + (a.Cin == 1 ? 0 : c)) * (N - 1), s, a.L, N, t);
#else
        load_window(v, xrow, s, a.L, t, 1.0f);
#endif
        tile_forward(v, w, tw, lds, t);
        for_each_pair(t, tw.base(), [&](int slot, int ia, int ib, cx wk, bool) {
            cx xe, xo;
            pair_split(NAT(w, ia), NAT(w, ib), xe, xo);
            pair_product_acc(xe, xo, Hp[slot * TILE_T + t], wk, ye[slot], yo[slot]);
        });
        __syncthreads();  // S2 reads of this window are done before the next window's S1 writes
    }
    cx pz[2][16], v[32];
    for_each_pair(t, tw.base(), [&](int slot, int ia, int ib, cx, bool self) {
        cx za, zb;
        pair_merge(ye[slot], yo[slot], za, zb);
        NAT(pz, ia) = za;
        if (!self) NAT(pz, ib) = zb;
    });
    tile_inverse(pz, v, tw, lds, t);
    store_valid(v, yrow, 0, a.O, a.Lout, t);
}
