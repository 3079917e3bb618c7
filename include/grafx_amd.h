/* grafx_amd — C ABI of the MI355X-native hot path of sh-lee97/grafx.
 *
 * The reference is pure Python/PyTorch: its "FFI" for this path is the set of
 * native calls its processors make through torch.  Each entry
 * point below replaces one of those call sites; the file:line cited is the
 * reference interface it stands in for (paths relative to
 * /root/reference/src/grafx/processors unless noted).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless marked "host";
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued on it and
 *     callers pass every workspace (sizes from the *_bytes queries).  ONE
 *     exception: the first call on a device of any entry point built on the FFT
 *     tile (fftconv, fir_spectrum, fir_grad, iir_fsm, odd_alias) allocates that
 *     device's 80 KB twiddle table with hipMalloc, fills it on `stream` and waits
 *     for it (hipStreamSynchronize) under a process-wide mutex; the table lives
 *     for the process.  The first fftconv / fir_grad call on a device also loads
 *     the code object of the hand-scheduled kernels (GFX_SCHED_PIPE; gfx950
 *     assembly embedded in the library, hipModuleLoadData: device memory for its
 *     ~0.5 MB of code).  After those first calls nothing allocates or
 *     synchronises (make them outside a stream capture).
 *     The device is the CURRENT device (hipGetDevice): make the tensors' device
 *     current before calling (grafx_amd/ops.py does);
 *   - return 0 on success, a negative GFX_E* code on error; never throws;
 *   - signals are fp32; a "row" is one (batch x node) item, channels inside.
 *
 * Row addressing (gfx_rowmap_t): element (r, c, n) of a signal lives at
 *     base + (r / inner) * stride_outer + (r % inner) * stride_inner
 *          + c * stride_ch + n                                   [floats]
 * so kernels read and write slices of render_grafx's (B, V, C, L) signal
 * buffer in place (inner = nodes of this type, stride_outer = V*C*L,
 * stride_inner = C*L) as well as plain contiguous (R, C, L) tensors
 * (inner = R, stride_inner = C*L).
 *
 * Aliasing: no array a call writes may share an element with an array the
 * call reads, with another array it writes, or with itself (a row map whose
 * rows land on the same floats).  Every kernel takes its pointers
 * __restrict__, and most read more than the element they store -- a halo of
 * the neighbouring tile, the samples a smoother remembers, x and gy again
 * after gx -- so a shared element is a wrong answer that depends on timing,
 * exact in-place use (y == x) included.  Two row ranges of one buffer that
 * interleave without touching are fine.  ONE exception:
 * gfx_biquad_cascade_state_f32 takes zi == zf and updates the state in place.
 * The library sees strides, not extents, so it cannot check this: the caller
 * does (grafx_amd/ops.py refuses such a call before anything is launched).
 */
#ifndef GRAFX_AMD_H
#define GRAFX_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GFX_OK 0
#define GFX_EINVAL -1   /* bad argument (shape, null pointer, unsupported size) */
#define GFX_ENOSPC -2   /* workspace too small */
#define GFX_ELAUNCH -3  /* HIP launch failed */

typedef struct {
    int64_t inner;
    int64_t stride_outer;
    int64_t stride_inner;
    int64_t stride_ch;
} gfx_rowmap_t;

/* library / device sanity: gfx_abi_version returns GFX_ABI_VERSION of the header the library was built from -- entries keep
 * their names when their argument lists change, so a binding compares it before the first call (version 1 had one entry per
 * argument list: INTEGRATION.md maps its names to these); gfx_device_info fills *n_cu, *lds_bytes if non-null (host ptrs). */
#define GFX_ABI_VERSION 2
int gfx_abi_version(void);
int gfx_device_info(int* n_cu, size_t* lds_bytes);

/* ---- FIR convolution core --------------------------------------------------------------
 * replaces convolve(): core/convolution.py:119-134 (torch.fft.rfft x2, irfft), and
 * FIRConvolution._native_forward: core/convolution.py:82-83.
 *
 * y[r, c, n] = sum_k h[r, c_f, k] * x[r, c_x, n + off - k],  n in [0, Lout)
 * (x is zero outside [0, L); channel dims broadcast 1<->C like torch).
 * off = 0, Lout = L            -> mode "causal"
 * off = N/2, Lout = L          -> mode "zerophase"
 * off = 0, Lout = L + N - 1    -> the full linear convolution
 * Overlap-save on 16384-sample LDS FFT tiles; filters longer than 8193 taps are
 * split into 8192-tap partitions (frequency-domain delay line).
 *
 * Step 1: gfx_fir_spectrum_f32 turns the taps h (RCf rows of N, contiguous) into the
 * tile spectra `Hs` (private layout, gfx_fir_spectrum_bytes bytes).  `gain` (nullable) scales
 * row-channel rc by gain[rc / gain_div].
 * Step 2: gfx_fftconv_f32 streams x through the tiles.
 * `part_len`: 0 for the default filter partitioning, or the value of gfx_fftconv_part_len(N, Lout) -- longer
 * partitions (fewer of them, fewer signal windows) for "long filter, short output" problems such as the filter
 * gradient of a training step (N = signal length taps, Lout = filter taps); the spectra, both size queries and the
 * convolution must then be given the same part_len.
 */
int64_t gfx_fftconv_nparts(int64_t N);
int64_t gfx_fftconv_part_len(int64_t N, int64_t Lout);
size_t gfx_fir_spectrum_bytes(int64_t RCf, int64_t N, int64_t part_len);
size_t gfx_fftconv_workspace_bytes(int64_t R, int64_t C_in, int64_t L, int64_t Lout, int64_t off, int64_t N,
                                   int64_t part_len);
int gfx_fir_spectrum_f32(const float* h, const float* gain, int64_t gain_div, void* Hs,
                         int64_t RCf, int64_t N, int64_t part_len, void* stream);
/* Spectra of the time-reversed signal rows: filter (r, c) has the L taps x[r, c, L-1-k], read in place through
 * `xmap` -- the "filter" of the filter-gradient correlation (autograd of convolve(): grad_h[k] = sum_n g[n] x[n+off-k])
 * without materialising x.flip(-1).  Buffer size: gfx_fir_spectrum_bytes(R * C, L, part_len). */
int gfx_fir_spectrum_rev_f32(const float* x, gfx_rowmap_t xmap, int64_t R, int64_t C, int64_t L, int64_t part_len,
                             void* Hs, void* stream);
/* Filter gradient of a short-filter convolve() (autograd of core/convolution.py:119-134), N <= 8193 taps:
 *   gh[r, c, k] = sum_n g[r, c_g, n] x[r, c_x, n + off - k],  k in [0, N),  x zero outside [0, L), g outside [0, Lg)
 * (channels broadcast 1 <-> 2; gh is (R, max(C_x, C_g), N) contiguous).  One pass over x and g, no workspace. */
int gfx_fir_grad_f32(const float* x, gfx_rowmap_t xmap, const float* g, gfx_rowmap_t gmap, float* gh,
                     int64_t R, int64_t C_x, int64_t C_g, int64_t L, int64_t Lg, int64_t N, int64_t off, void* stream);

/* The convolution.  `h_rows` <= R: row r convolves with filter (r % h_rows) -- rows are batch-major
 * (r = b * nodes + node), so h_rows = nodes shares one filter per node across the batch, which is what render_grafx's
 * 4-D path means by un-batched parameters (render/graph.py:68-75 expands them B times; here the spectra are built once
 * per node and every batch row reads them); h_rows = R is one filter per row.
 * `xcopy` (nullable: no tee) additionally receives a copy of the input rows (rows addressed by `cmap`, same
 * R x C_in x L) from the registers that already hold them.  render_grafx keeps every node's signal in one buffer
 * (render/graph.py:104-106: `signal_buffer[:, :num_sources] = input_signals`); when the first stage is a convolution
 * this folds that copy into the stage's kernel.  Only for the causal single-partition case (off == 0, Lout >= L -- the
 * full-length convolution the odd-length aliasing starts from included --, C_in == max(C_in, C_f), N <= 8193); anything
 * else returns GFX_EINVAL.
 * `schedule`, for filters of N <= 8193 taps (same results to rounding):
 *   GFX_SCHED_TILE  one 16384-sample tile per 256-thread workgroup (fftconv1_kernel, compiler-scheduled).
 *   GFX_SCHED_PIPE  the hand-scheduled persistent form of the same tile (generated gfx950 assembly, explicit register
 *                   allocation: the next tile's window, the filter spectrum and the output stores are interleaved
 *                   with the arithmetic of the running tile).  GFX_EINVAL where it does not apply.
 *   GFX_SCHED_AUTO  the faster of the two for the shape at hand.
 * For longer filters (partitioned convolution: xspec_kernel + a product kernel) GFX_SCHED_TILE selects one output tile per
 * 256-thread workgroup (macinv_kernel) and GFX_SCHED_AUTO two consecutive ones per 512-thread workgroup (macinv_pair_kernel:
 * each window spectrum and filter partition fetched once per pair; equal to a few units in the last place of the largest
 * output); GFX_SCHED_PIPE: GFX_EINVAL.
 * (Round-2 experiments -- ping-pong, half-size exchanges, 512-thread tile -- live in tools/experiments/r2_schedules.)
 * `rowmax`, `rowmax_written`: both NULL, or both given under GFX_SCHED_AUTO (one of them alone, or another schedule with
 * them: GFX_EINVAL).  Given, the call may leave the bits of max |y| of every output row-channel in `rowmax`
 * (R * max(C_in, C_f) words, zeroed by the caller, row-major (row, channel)): the compiler-built tile kernels (one
 * partition, and the partitioned convolution's product kernels) take them as a by-product of their stores (one atomic
 * maximum per wave and tile) and set *rowmax_written = 1; the hand-scheduled kernel and the one-output-tile form leave the
 * words alone and *rowmax_written = 0.  For the full-length convolution that feeds the odd-length aliasing
 * (core/convolution.py:119-134), whose two-rows-per-transform form scales the second row of a pair by these maxima
 * (gfx_odd_alias_pair_f32's rowmax): the separate pass over z is not needed then. */
#define GFX_SCHED_AUTO 0
#define GFX_SCHED_TILE 1
#define GFX_SCHED_PIPE 2
int gfx_fftconv_f32(const float* x, gfx_rowmap_t xmap, const void* Hs, int64_t h_rows, int64_t part_len,
                    float* y, gfx_rowmap_t ymap, float* xcopy, gfx_rowmap_t cmap,
                    int64_t R, int64_t C_in, int64_t C_f, int64_t L, int64_t Lout, int64_t off, int64_t N,
                    void* ws, size_t ws_bytes, int schedule, uint32_t* rowmax, int* rowmax_written, void* stream);

/* State across calls: one block of a streamed CAUSAL convolution (Lout = L, off = 0, default partition geometry).
 *   y[r, c, n] = sum_k h[r % h_rows, c_f, k] xx[r, c_x, n - k],  n in [0, L),  xx = zi || x
 * zi, zf: contiguous float32 (R, C_in, N - 1), oldest sample first -- the last N - 1 input samples before / after this
 * block.  zi == NULL: silence before the block; zf == NULL: no state wanted.  zf = the last N - 1 samples of zi || x: a
 * copy (bit-exact; for L < N - 1 the old history shifts), written by a small kernel of its own, stream-ordered after the
 * convolution.  The window loaders of the tile kernels read the history in place where the stateless kernels take zeros
 * (fftconv1_state_kernel, xspec_state_kernel, winmac_state_kernel): no concatenated copy of the signal, no allocation.
 * Blocks of a signal cut anywhere, each entering with the zf of the block before, concatenate to the linear convolution
 * of the whole.  zi and zf must not overlap: GFX_EINVAL.  N = 1 has an empty state (zi, zf ignored).  Workspace:
 * gfx_fftconv_workspace_bytes(R, C_in, L, L, 0, N, 0).  schedule: GFX_SCHED_AUTO or GFX_SCHED_TILE (which product kernel
 * a partitioned convolution takes, as in gfx_fftconv_f32); a call with state never takes the hand-scheduled
 * kernels: GFX_SCHED_PIPE is GFX_EINVAL.  Everything else (row maps, channel broadcast, h_rows, row-count limits) as
 * gfx_fftconv_f32. */
int gfx_fftconv_state_f32(const float* x, gfx_rowmap_t xmap, const void* Hs, int64_t h_rows, float* y, gfx_rowmap_t ymap,
                          const float* zi, float* zf, int64_t R, int64_t C_in, int64_t C_f, int64_t L, int64_t N,
                          void* ws, size_t ws_bytes, int schedule, void* stream);

/* Diagnostic: the name -- as rocprofv3's kernel trace prints it -- of the (dominant) kernel that the calling thread's last
 * successful gfx_fftconv_* call launched: "gfx_fftconv_pipe_t1_o8", "fftconv1_kernel<true>", "winmac_kernel",
 * "xspec_kernel+macinv_pair_kernel"; "" before the first call.  The string is static.  (bench.py labels its live per-launch
 * timings with it, so that the line's `roofline.kernel` is a name a profile of the same command contains.) */
const char* gfx_fftconv_last_kernel(void);

/* Short filters (N <= gfx_fir_direct_max_taps() = 512) as batched Toeplitz GEMMs on the fp32 matrix cores, taps given
 * directly (no spectra): the direct-form counterpart of gfx_fftconv_f32 with the same meaning of every argument
 *   y[r, c, n] = sum_k h[r % h_rows, c_f, k] x[r, c_x, n + off - k],  n in [0, Lout),  x zero outside [0, L)
 * h is (h_rows * C_f, N) contiguous.  Replaces convolve() / FIRConvolution for short FIRs (core/convolution.py:85-134,
 * filter.py:34-39); exact fp32 (v_mfma_f32_16x16x4_f32).  MFMA-bound above ~64 taps, HBM-bound below. */
int64_t gfx_fir_direct_max_taps(void);
int gfx_fir_direct_f32(const float* x, gfx_rowmap_t xmap, const float* h, int64_t h_rows, float* y, gfx_rowmap_t ymap,
                       int64_t R, int64_t C_in, int64_t C_f, int64_t L, int64_t Lout, int64_t off, int64_t N,
                       void* stream);

/* ---- the reference's odd-length aliasing ----------------------------------------------------
 * convolve() (core/convolution.py:119-134) inverts a P-point spectrum (P = Lx + Lh - 1) with irfft's default length
 * 2 (P // 2): for odd P the result is  y = irfft_{P-1}(rfft_P(z))  of the linear convolution z -- what every reference
 * default length produces.  gfx_odd_alias_f32 computes y[:, lo : lo + len] from z (rows x P, contiguous) with two
 * chirp-z transforms on the LDS FFT tile (no FFT library, fp32); 3 <= P <= 11,184,811 odd (NFFT up to 64 x 32 x 8192), rows
 * <= 16383 per call, else the size queries return 0.  `plan` (per P: chirps and their spectra) comes from gfx_odd_alias_plan_f32, which needs a
 * workspace of gfx_odd_alias_workspace_bytes(1, P); the transform needs gfx_odd_alias_workspace_bytes(rows, P).
 * gfx_odd_alias_adjoint_f32 is the transposed map (the gradient the reference gets from differentiating its
 * rfft / irfft pair): gz (rows x P, contiguous) from gy (rows x len, row stride ldg), the gradient with respect to
 * y[:, lo : lo + len]; same plan, same workspace size. */
size_t gfx_odd_alias_plan_bytes(int64_t P);
size_t gfx_odd_alias_workspace_bytes(int64_t rows, int64_t P);
int gfx_odd_alias_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream);
/* `ymap` (nullable): the output rows are written straight into a signal addressed through a row map instead of y + r * ldy
 * (ldy is ignored then): row q = row0 + r of the call is row q / C, channel q % C of `y` (a strided (B, n, C, len) view of
 * render_grafx's signal buffer, render/core.py:80-98), so that a stage on the aliasing path needs no copy of its result
 * into the buffer.  `z` holds `rows` rows of this call.  ymap == NULL: C and row0 are ignored. */
int gfx_odd_alias_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                      const void* plan, void* ws, size_t ws_bytes, const gfx_rowmap_t* ymap, int64_t C, int64_t row0,
                      void* stream);
int gfx_odd_alias_adjoint_f32(const float* gy, int64_t ldg, int64_t lo, int64_t len, float* gz, int64_t rows, int64_t P,
                              const void* plan, void* ws, size_t ws_bytes, void* stream);
/* The same maps with the transforms carried in double precision (fp32 data in and out, own plan and workspace, both
 * twice the size): for the energy envelope of the dynamics processors (core/envelope.py:34-49), whose aliased result
 * feeds log() and a gain curve -- the ~1e-6-of-peak noise floor of an fp32 transform pair is amplified beyond the
 * parity bound on quiet passages.  Same geometry limits and error codes. */
size_t gfx_odd_alias_precise_plan_bytes(int64_t P);
size_t gfx_odd_alias_precise_workspace_bytes(int64_t rows, int64_t P);
int gfx_odd_alias_precise_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream);
int gfx_odd_alias_precise_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                              const void* plan, void* ws, size_t ws_bytes, void* stream);
int gfx_odd_alias_precise_adjoint_f32(const float* gy, int64_t ldg, int64_t lo, int64_t len, float* gz, int64_t rows,
                                      int64_t P, const void* plan, void* ws, size_t ws_bytes, void* stream);
/* The forward maps with TWO real rows per complex transform (csrc/czt_pair.hip): the pair z1 + i z2 goes through the
 * two chirp-z transforms as one complex row with the spectrum kept on both sides (P bins) and comes out as
 * A z1 + i A z2 -- 2P - 1 points per pair instead of (3P - 1) / 2 per row, a third fewer bytes through each of the same
 * passes.  Rows 2r and 2r + 1 of a call form a pair (an odd row count leaves the last row alone); the second row of a pair
 * goes through scaled by the exact power of two that brings it to the first row's binade (from max |z| of the rows: a pass
 * of the call itself, one word per row behind the workspace, or -- `rowmax` != NULL -- words the producer of z left:
 * gfx_fftconv_f32's rowmax), so every row keeps an error relative to its own peak.  3 <= P <= 8 388 607 odd (2P - 1 <= 2^24 points), else the size queries return
 * 0 and the calls GFX_EINVAL (use the one-row forms above); own plan (gfx_odd_alias_pair_plan_f32, workspace of
 * gfx_odd_alias_pair_workspace_bytes(1, P)) and workspace (gfx_odd_alias_pair_workspace_bytes(rows, P)); `ymap`, C, row0
 * as in gfx_odd_alias_f32, and row0 must be even.  The `precise` forms carry the transforms in double (plan and
 * workspace twice the size) and can fuse the envelope smoother's relu (core/envelope.py:48) into the last pass
 * (`relu` != 0): no separate clamp over the rows.  Same results as the one-row forms up to rounding (tests/test_gpu_odd_alias_pair.py). */
size_t gfx_odd_alias_pair_plan_bytes(int64_t P);
size_t gfx_odd_alias_pair_workspace_bytes(int64_t rows, int64_t P);
int gfx_odd_alias_pair_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream);
int gfx_odd_alias_pair_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                           const void* plan, void* ws, size_t ws_bytes, const gfx_rowmap_t* ymap, int64_t C, int64_t row0,
                           const uint32_t* rowmax, void* stream);
size_t gfx_odd_alias_pair_precise_plan_bytes(int64_t P);
size_t gfx_odd_alias_pair_precise_workspace_bytes(int64_t rows, int64_t P);
int gfx_odd_alias_pair_precise_plan_f32(void* plan, int64_t P, void* ws, size_t ws_bytes, void* stream);
int gfx_odd_alias_pair_precise_f32(const float* z, float* y, int64_t ldy, int64_t lo, int64_t len, int64_t rows, int64_t P,
                                   const void* plan, void* ws, size_t ws_bytes, const uint32_t* rowmax, int relu,
                                   void* stream);

/* ---- small inverse real DFT (parameter-side front-ends) ---------------------------------------
 * y = irfft(X, n) for any n <= 8192 as a direct sum (twiddles tabulated in LDS), K = n/2 + 1 bins per row, X complex
 * (rows, K, 2) or real (rows, K) when is_real; the result is rotated by `roll` and multiplied by `window` (n, nullable):
 *   y[row, (m + roll) mod n] = window[(m + roll) mod n] * irfft(X[row], n)[m]
 * Replaces the FFT-library calls of the zero-phase FIR design (core/fir.py:20-27: irfft, roll, window) and of the
 * surrogate delay (core/delay.py:73-76). */
int gfx_irdft_f32(const float* X, int is_real, float* y, int64_t rows, int64_t K, int64_t n, int64_t roll,
                  const float* window, void* stream);
/* The forward twin: X[row, k] = sum_m x[row, m] e^{-2 pi i k m / n}, k = 0 .. n/2 (torch.fft.rfft), X (rows, K, 2), any
 * n <= 8192, direct sum.  It is the adjoint of gfx_irdft_f32 up to the bin weights, i.e. the gradient of every
 * frequency-sampled front-end (core/iir.py:150 irfft(n=fsm_fir_len), reverb.py:176-184 istft frames): the training path's
 * parameter-side transforms stay off the FFT library. */
int gfx_rdft_f32(const float* x, float* X, int64_t rows, int64_t K, int64_t n, void* stream);

/* ---- frequency-sampled IIR -------------------------------------------------------------
 * replaces IIRFilter._process_fsm / iir_fsm / delay: core/iir.py:147-150, 263-276
 * (complex64 response of the biquad cascade on the N-point grid, then torch.fft.irfft(n=N)).
 * Bs, As: (RC, K, 3) contiguous; h: (RC, N) taps out.  N <= 4096 (Bluestein on the LDS tile).
 * `plan` is a per-N constant (gfx_iir_fsm_plan_bytes bytes) filled once by gfx_iir_fsm_plan_f32.
 */
/* 1 when gfx_iir_fsm_fir_f32 has a native kernel for fsm_fir_len = N: 1 <= N <= 4096 (Bluestein on one LDS tile; needs the
 * plan of gfx_iir_fsm_plan_f32) and N = 8192, 16384 (the tile's own inverse real transform; `plan` may be NULL). */
int gfx_iir_fsm_native(int64_t N);
size_t gfx_iir_fsm_plan_bytes(int64_t N);
int gfx_iir_fsm_plan_f32(void* plan, int64_t N, void* stream);
int gfx_iir_fsm_fir_f32(const float* Bs, const float* As, const void* plan, float* h,
                        int64_t RC, int64_t K, int64_t N, void* stream);
/* The same taps from coefficients given in DOUBLE precision: the cascade response is evaluated in double at the exact
 * sample points exp(-2 pi i d k / N) and rounded once -- for cascades whose float32 coefficients lose the filter (the
 * third-octave GraphicEqualizer's 9 Hz wide bands: 1 +- beta with beta = 6.5e-4; reference eq.py:339-436, core/geq.py),
 * where the reference's own float32 result is 1e-4 .. 4e-4 from a float64 evaluation of its formulas. */
int gfx_iir_fsm_fir_f64c_f32(const double* Bs, const double* As, const void* plan, float* h, int64_t RC, int64_t K,
                             int64_t N, void* stream);
/* Gradient of gfx_iir_fsm_fir_f32's taps with respect to the coefficients (what autograd derives from core/iir.py:147-152):
 * G = rfft(dL/dh, n = N) as (RC, N / 2 + 1) interleaved complex64 (gfx_rdft_f32), `delays` = the (3, N / 2 + 1) complex64
 * table e^(-j phi[d, k]) of the forward pass (float32 phases); gB / gA: (RC, K, 3), either may be NULL.  Double precision
 * inside (the sums over the bins cancel to 1e-5 of their terms); one launch instead of ~40 complex128 torch kernels. */
int gfx_iir_fsm_bwd_f32(const float* Bs, const float* As, const float* G, const float* delays, float* gB, float* gA,
                        int64_t RC, int64_t K, int64_t N, void* stream);

/* coefficient front-ends (elementwise over n = rows*channels items of K biquads)
 * gfx_peq_coeffs_f32    replaces ParametricEqualizer.forward's activations + RBJ formulas:
 *                       eq.py:291-314, filter.py:593-604, 645-656, 687-705, 736-754
 * gfx_biquad_coeffs_f32 replaces BiquadFilter.forward's stability activations: filter.py:144-153
 *                       (A0 nullable = "normalized" off)
 */
int gfx_peq_coeffs_f32(const float* w0, const float* q_inv, const float* log_gain, float* Bs, float* As,
                       int64_t n, int64_t K, int use_shelving, void* stream);
int gfx_biquad_coeffs_f32(const float* Bin, const float* A1_pre, const float* A2_pre, const float* A0,
                          float* Bs, float* As, int64_t n, void* stream);
/* autograd of gfx_peq_coeffs_f32: (dL/dBs, dL/dAs) (n, K, 3) -> dL/d(w0, q_inv, log_gain) (n, K), the chain rule
 * through the RBJ formulas and the activations in one elementwise pass (what torch autograd does with ~120 kernels). */
int gfx_peq_coeffs_bwd_f32(const float* w0, const float* q_inv, const float* log_gain, const float* gBs,
                           const float* gAs, float* gw0, float* gq_inv, float* glog_gain,
                           int64_t n, int64_t K, int use_shelving, void* stream);

/* ---- dynamics ---------------------------------------------------------------------------
 * gfx_dynamics_fused_f32 replaces Compressor.forward / NoiseGate.forward (dynamics.py:361-409,
 *   598-641) for energy_smoother in {None (smoother=0), "iir" (smoother=1)} and no gain
 *   smoother: energy -> truncated one-pole (exact recursive form, iir_len taps) -> log ->
 *   knee (0 hard, 1 quadratic, 2 exponential; gate=1 selects NoiseGate's curves) -> exp -> y.
 *   Per-row parameters are (R) arrays (the reference's (R,1) tensors).
 * The remaining entry points are the same stages as separate launches, for configurations
 * the fused kernel does not cover (ballistics, gain smoothing, odd-P compatibility):
 *   gfx_energy_f32       e = mean_c x^2                                   dynamics.py:390
 *   gfx_onepole_f32      TruncatedOnePoleIIRFilter on (R,L) rows -> (R,Lout), optional relu
 *                        core/envelope.py:34-60 (Lout = L + iir_len - 1 gives the full convolution)
 *   gfx_onepole_fir_f32  its taps h[n] = (1-a) exp(n log a)              core/envelope.py:51-60
 *   gfx_ballistics_*     Ballistics / torchcomp.compressor_core          core/envelope.py:84-101
 *                        (z_alpha: (R,2); the recursion is torchcomp's published one, the wheel is absent: see DESIGN.md)
 *   gfx_dyn_gain_f32     env -> gain: log(env+1e-5) -> knee [-> exp unless log_out]
 *   gfx_apply_gain_f32   y = (exp_gain ? exp(g) : g)[:,None,:] * x        dynamics.py:405
 *   gfx_stereo_gain_f32  StereoGain.forward                               stereo.py:38-41
 */
/* Parameters may be shared across the batch: row r reads parameter row (r % param_rows); param_rows = R is one set per row.
 * `ws`: a workspace of gfx_dynamics_ws_bytes(param_rows) bytes (scratch for this call), or NULL: one workgroup per row.
 * `u1` (R, L), optional: receives the un-truncated smoother scan (1 - a) * U, kept for gfx_dynamics_bwd_f32
 * (u1_is_scratch = 0) -- one extra 4-byte store per sample.  With a workspace the smoothed configuration runs as
 * dependency-free one-shot tiles: every
 * 1024-sample tile of every row is its own workgroup, which re-reads the H = ceil(log 1e-12 / log a) most recent
 * samples before the tile to rebuild the smoother state (exact to 1e-12 of the peak energy: the smoother is a FIR with
 * taps (1 - a) a^k) -- the access shape of a plain copy, where one workgroup per row is a set of long scattered
 * streams.  Rows whose history does not fit (H > 256, or a live a^N truncation term) are picked out on the device from
 * a per-row pole table and produced by the row kernel in the same call; no host synchronisation. */
size_t gfx_dynamics_ws_bytes(int64_t param_rows);
/* The workspace that also keeps rows with a LONG smoother memory on the tile grid (round 5): with
 * gfx_dynamics_ws_bytes_ex(param_rows, R, L) bytes -- the pole table, 64 bytes of counters and 8 bytes per row and
 * 512-sample tile -- a row whose history is longer than a tile may re-read (256 < H <= 64 * 512 samples, truncation term
 * dead) gets the state entering each tile from the AGGREGATES of the tiles before it: every tile publishes the state it
 * would leave from a zero entry state as soon as its own samples are scanned, then reads the ceil(H / 512) aggregates
 * before it (an in-launch hand-off through 8-byte granules, zeroed by a memset on the stream in front of the launch;
 * workgroups take their logical index from a ticket counter, so no tile ever waits for a workgroup that has not
 * started).  Only rows with a LIVE truncation term (a^iir_len > 1e-12) are left to the row kernel.  A workspace of
 * gfx_dynamics_ws_bytes(param_rows) bytes keeps the round-4 behaviour (those rows on the row kernel too). */
size_t gfx_dynamics_ws_bytes_ex(int64_t param_rows, int64_t R, int64_t L);
int gfx_dynamics_fused_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap,
                           const float* log_threshold, const float* log_ratio, const float* log_knee,
                           const float* z_alpha, int64_t param_rows, int64_t R, int64_t C, int64_t L,
                           int smoother, int64_t iir_len, int knee, int gate, float* u1,
                           void* ws, size_t ws_bytes, void* stream);
/* Diagnostic, the twin of gfx_fftconv_last_kernel: the name -- as rocprofv3's kernel trace prints it -- of the kernel that
 * carries the rows of the calling thread's last successful gfx_dynamics_fused_* call: "dyn_oneshot_mix_kernel" (tiles with
 * the routing sums), "dyn_oneshot_kernel" (tiles; rows the pole table rejects ride on dyn_fused_kernel in the same call),
 * "dyn_oneshot_kernel+dyn_oneshot_mix_kernel" (the same with the look-back workspace: rows with a long smoother memory
 * are produced by the row-group walk, an instance of the routing-sum kernel without sums -- which of the two ran is
 * decided on the device) or "dyn_fused_kernel" (one workgroup per row: no workspace, or no smoother); "" before the first call. */
const char* gfx_dynamics_last_kernel(void);
/* The same with the routing sum that follows fused in (render/core.py:36-112, a "mix" stage that sums this call's rows):
 * rows come in graphs of `inner` consecutive rows (r = g * inner + j, R % inner == 0); destination d of graph g is
 * written to mix + g * mix_sb + d * mix_sv + c * mix_sc, every row's output to y as before.  Per destination the rows
 * are added in increasing j, from 0.0f -- the order of the gather-sum kernels, so the sums are identical to that separate
 * pass.  A destination holds one of n_acc <= 4 accumulators between its first and its last source; sched (device memory,
 * `inner` entries) says per row j: bits 0..3 = accumulators the row is added to; byte 1 + a = destination + 1 to store
 * accumulator a to (and clear it) after this row, 0 = none (the caller colours the live ranges:
 * grafx_amd.ops.mix_schedule).  `extras` (nullable; n_pre + n_post pairs of int64) names sources of the sum that are not
 * rows of this call but finished rows of the same buffer: (row offset from `mix` in units of mix_sv, code as in sched);
 * the first n_pre are added before the call's rows, the others after them.  Needs the one-pole smoother, the workspace and
 * 16-byte aligned rows with L % 4 == 0; GFX_EINVAL otherwise (callers run the two stages separately then).
 * `flags`: 0, or GFX_MIX_SKIP_ROWS: the call's own rows are NOT stored by the tile kernels -- for a render whose
 * caller wants the output node only (grafx_amd.render.render_grafx(keep_signal_buffer=False)) and a stage whose rows
 * nothing but the fused routing sums reads: the stage then moves 8 instead of 16 bytes per stereo sample plus the sums.
 * (Rows the pole table leaves to the row kernel are still written: the summing tiles read them back from y.) */
#define GFX_MIX_SKIP_ROWS 1
int gfx_dynamics_fused_mix_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* log_threshold,
                               const float* log_ratio, const float* log_knee, const float* z_alpha, int64_t param_rows,
                               int64_t R, int64_t C, int64_t L, int smoother, int64_t iir_len, int knee, int gate,
                               float* u1, void* ws, size_t ws_bytes, const int64_t* sched, int64_t inner, int64_t n_acc,
                               float* mix, int64_t mix_sb, int64_t mix_sv, int64_t mix_sc, const int64_t* extras,
                               int64_t n_pre, int64_t n_post, int flags, void* stream);
int gfx_energy_f32(const float* x, gfx_rowmap_t xmap, float* e, int64_t R, int64_t C, int64_t L, void* stream);
int gfx_onepole_f32(const float* u, const float* z_alpha, float* out, int64_t R, int64_t L, int64_t Lout,
                    int64_t iir_len, int relu, void* stream);
/* gfx_onepole_f32 on the energy mean_c x^2 of a signal read in place through its row map (dynamics.py:390 + core/envelope.py:
 * 34-60 in one pass: no energy buffer), optionally leaving the bits of max |out| of every row in `rowmax` (R words; NULL: not
 * wanted) -- the by-product the odd-length aliasing of a full-length result (Lout = L + iir_len - 1) scales its pairs by. */
int gfx_onepole_energy_f32(const float* x, gfx_rowmap_t xmap, int64_t C, const float* z_alpha, float* out, int64_t R,
                           int64_t L, int64_t Lout, int64_t iir_len, int relu, uint32_t* rowmax, void* stream);
int gfx_onepole_fir_f32(const float* z_alpha, float* h, int64_t R, int64_t iir_len, void* stream);
/* Ballistics.forward (core/envelope.py:84-101): at, rt = sigmoid(z_alpha[:, 0]), sigmoid(z_alpha[:, 1]);  y[-1] = 1;
 * c = at if u[n] < y[n-1] else rt;  y[n] = (1 - c) y[n-1] + c u[n], the two products and the sum rounded separately
 * (torchcomp's CPU loop).  u, y: (R, L).  `is_coef` != 0: z_alpha holds at, rt themselves (no sigmoid) -- how the parity
 * tests hand the oracle's coefficients over.
 * ws == NULL: every row is walked whole, one lane per row.  With a workspace of gfx_ballistics_ws_bytes(R) bytes (scratch
 * for this call: one flag per row) the same values, bit for bit, are produced from chunks of the rows: a row is cut into up
 * to 64 chunks that start from a warmed-up guess and are accepted only if every chunk is entered with exactly the state
 * its left neighbour ends with; rows that fail that check, or whose slower coefficient needs a longer warm-up than a
 * chunk, are walked whole by a second launch in the same call (no host synchronisation).
 * State across calls: y[-1] = zi[r] instead of 1 for signal row r (zi: (R), NULL = 1; never indexed by param_rows) and
 * y[L-1] of every row is left in zf ((R), NULL = not wanted), in the sequential recursion's bits whichever schedule
 * produced them: a signal cut anywhere and processed block by block, each block entering with the zf of the block
 * before, gives the one-call output bit for bit (gfx_dynamics_ballistics_f32: the one-call ENVELOPE; the gain computer's
 * output is the same bits when the blocks take the same kernel form, L % 4 == 0 on aligned rows).  Later launches of a
 * call re-read zi for the rows they walk again, so zi and zf must not overlap: GFX_EINVAL. */
size_t gfx_ballistics_ws_bytes(int64_t R);
int gfx_ballistics_f32(const float* u, const float* z_alpha, int is_coef, const float* zi, float* zf, float* y, int64_t R,
                       int64_t L, void* ws, size_t ws_bytes, void* stream);
/* The same recursion over the energy of a signal, env = ballistics(mean_c x^2) (dynamics.py:390 followed by
 * core/envelope.py:84-101 -- Compressor / NoiseGate with energy_smoother="ballistics"): x (R, C, L) addressed through xmap
 * is read once, the energy never reaches memory.  env: (R, L). */
int gfx_ballistics_energy_f32(const float* x, gfx_rowmap_t xmap, int64_t C, const float* z_alpha, int is_coef,
                              const float* zi, float* zf, float* env, int64_t R, int64_t L, void* ws, size_t ws_bytes,
                              void* stream);
/* Compressor / NoiseGate with energy_smoother="ballistics" and no gain smoother as ONE pass over the signal
 * (dynamics.py:390-405 with core/envelope.py:84-101 inside): energy -> attack / release recursion (the float32 sequential
 * recursion exactly, as above) -> log -> knee -> exp -> y = gain * x.  x, y: (R, C, L) through their row maps (in-place
 * slices of the render buffer); per-row parameters as gfx_dynamics_fused_f32 (row r reads row r % param_rows),
 * z_alpha: (param_rows, 2); ws: gfx_ballistics_ws_bytes(R) bytes, or NULL for the whole-row walk only. */
int gfx_dynamics_ballistics_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* log_threshold,
                                const float* log_ratio, const float* log_knee, const float* z_alpha, int64_t param_rows,
                                int64_t R, int64_t C, int64_t L, int knee, int gate, const float* zi, float* zf, void* ws,
                                size_t ws_bytes, void* stream);
/* Adjoint of the recursion above given the forward input x, output y and g = dL/dy:
 * gx = dL/dx (R, L), gz = dL/dz_alpha (R, 2).  The attack/release choice is treated as locally constant.
 * State: y[-1] = zi[r] (NULL = 1), and gzi (R; NULL = not wanted) receives dL/dzi = (1 - c[0]) lambda[0], the carry that
 * leaves sample 0.  A cotangent of zf is a cotangent of y[L-1]: the caller adds it to g[:, L-1].
 * ws == NULL: every row is walked whole by one lane, whatever the geometry (no GFX_ENOSPC for a missing workspace).  With
 * ws of gfx_ballistics_bwd_ws_bytes(R, L) bytes (per-chunk partial sums of the two coefficient gradients, added in a fixed
 * order) the rows are cut into chunks that different workgroups walk (the adjoint is linear and a contraction: each chunk
 * starts 2048 samples later in time with a zero carry, exact to (1 - c)^2048 <= 6e-10 for coefficients >= 0.0103; a
 * 64-row group with a slower row is walked whole); a geometry of one chunk takes the whole-row walk all the same. */
size_t gfx_ballistics_bwd_ws_bytes(int64_t R, int64_t L);
int gfx_ballistics_bwd_f32(const float* x, const float* y, const float* g, const float* z_alpha, const float* zi, float* gx,
                           float* gz, float* gzi, int64_t R, int64_t L, void* ws, size_t ws_bytes, void* stream);
int gfx_dyn_gain_f32(const float* env, float* gain, const float* log_threshold, const float* log_ratio,
                     const float* log_knee, int64_t R, int64_t L, int knee, int gate, int log_out, void* stream);
/* Backward of the gain computer, for the training path (forward: gfx_dynamics_fused_f32).
 * gfx_dyn_gain_bwd_f32, one pass over x, the output gradient gy and the (smoothed) energy env (R, L):
 *   gain = exp(g(log(env + 1e-5)))                       -> gain (R, L)
 *   dg   = gain * sum_c gy[c] x[c];   denv = dg * dg/dG / (env + 1e-5)   -> denv (R, L)
 *   gparams[r, 0..2] += sum_n dg * (dg/dlog_threshold, dg/dlog_ratio, dg/dlog_knee)   (caller zero-fills)
 * with the partials of dynamics.py:444-489 / 676-721 (region masks piecewise constant, as in torch autograd).
 * gfx_dyn_dx_f32: gx = gain * gy + (2/C) * de * x, de = dL/d(mean_c x^2) (denv pushed back through the smoother). */
int gfx_dyn_gain_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, const float* env,
                         const float* log_threshold, const float* log_ratio, const float* log_knee,
                         int64_t R, int64_t C, int64_t L, int knee, int gate,
                         float* gain, float* denv, float* gparams, void* stream);
int gfx_dyn_dx_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, const float* gain,
                   const float* de, float* gx, int64_t R, int64_t C, int64_t L, void* stream);
/* The whole backward of Compressor / NoiseGate with the one-pole energy smoother and no gain smoother (reference: autograd
 * through dynamics.py:390-405 and core/envelope.py:34-60): one pass backward in time over (x, gy, u1) -- the smoother's
 * adjoint scan and gx = gain * gy + (2/C) * de * x, the gain computer's derivatives recomputed from u1 where they are
 * needed.  gx rows addressed by gxmap (e.g. a slice of the render's gradient buffer); gparams (R,3).  dalpha (R),
 * optional: dL/d(pole) of the smoother before the sigmoid/clamp chain rule, accumulated by the same pass from u1 and its
 * own adjoint scan (the D = dU/da scan of core/envelope.py's truncated filter is moved onto the adjoint side, so no third
 * scan is needed).
 * `u1` (R, L) = (1-a) x the un-truncated one-pole scan of the energy:
 *   u1_is_scratch = 0  the scan the forward pass kept (gfx_dynamics_fused_f32's u1); it is only read.
 *   u1_is_scratch = 1  R x L floats of scratch: the scan is rebuilt from x here, so the forward pass of a training step
 *                      has nothing to store.
 * `ws`: gfx_dynamics_bwd_ws_bytes(R, L) bytes of scratch for this call, or NULL: every row on the row kernel (with
 * u1_is_scratch = 1: scan x into u1, then the backward pass).  With a workspace, rows with a short smoother memory --
 * chosen per row on the device, exactly as in gfx_dynamics_fused_f32 -- run as dependency-free one-shot tiles walking
 * backward in time, the others on the row kernel.  The tiles' shares of the per-row sums (gparams, dalpha) go through the
 * workspace and are added in a fixed order: no float atomics, the gradients are the same bits from run to run.  Under
 * u1_is_scratch = 1 the one-shot tiles rebuild the scan from x inside the tile (in the backward walk it is a suffix scan;
 * the state entering a tile from its far end is the dot product of the H samples beyond it), so for those rows the
 * scratch is never touched; the rows of the row kernel get their scan written to the scratch first. */
size_t gfx_dynamics_bwd_ws_bytes(int64_t R, int64_t L);
int gfx_dynamics_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap,
                         const float* log_threshold, const float* log_ratio, const float* log_knee,
                         const float* z_alpha, int64_t R, int64_t C, int64_t L, int64_t iir_len, int knee, int gate,
                         float* gx, gfx_rowmap_t gxmap, float* gparams, float* u1, int u1_is_scratch, float* dalpha,
                         void* ws, size_t ws_bytes, void* stream);
/* Pole gradient of TruncatedOnePoleIIRFilter (core/envelope.py:34-60) from the un-truncated scan U of its input and
 * the scan S of U:  da[r] = sum_n g[r,n] (c0 U[n] + c2 U[n-N]) + g[r,n+1] (c1 S[n] + c3 S[n-N]),  coef = (R, 4). */
int gfx_onepole_dz_f32(const float* g, const float* U, const float* D, const float* coef, float* da, int64_t R,
                       int64_t L, int64_t N, void* stream);
int gfx_apply_gain_f32(const float* x, gfx_rowmap_t xmap, const float* g, float* y, gfx_rowmap_t ymap,
                       int64_t R, int64_t C, int64_t L, int exp_gain, void* stream);
/* Gain computer and gain stage in one pass over an envelope a smoother left in memory (dynamics.py:394-405):
 * y[r,c,n] = exp(g(log(env[r,n] + 1e-5))) * x[r,c,n], g the knee of gfx_dyn_gain_f32; row r reads parameter row r % param_rows. */
int gfx_dyn_gain_apply_f32(const float* x, gfx_rowmap_t xmap, const float* env, float* y, gfx_rowmap_t ymap,
                           const float* log_threshold, const float* log_ratio, const float* log_knee, int64_t param_rows,
                           int64_t R, int64_t C, int64_t L, int knee, int gate, void* stream);
int gfx_stereo_gain_f32(const float* x, gfx_rowmap_t xmap, const float* log_gain, float* y, gfx_rowmap_t ymap,
                        int64_t R, int64_t C_in, int64_t L, void* stream);
/* StereoGain with the routing sum behind it fused in (the gain / pan stage in front of a bus): y as above, and the mix
 * destinations as gfx_dynamics_fused_mix_f32 produces them -- same sched / n_acc / extras words, same summation order,
 * identical sums.  log_gain is (R, 2); rows in graphs of `inner` (the row maps' `inner`); needs 16-byte aligned rows and
 * L % 4 == 0, GFX_EINVAL otherwise (callers run gfx_stereo_gain_f32 and the gather-sum then). */
int gfx_stereo_gain_mix_f32(const float* x, gfx_rowmap_t xmap, const float* log_gain, float* y, gfx_rowmap_t ymap,
                            int64_t R, int64_t C_in, int64_t L, const int64_t* sched, int64_t inner, int64_t n_acc,
                            float* mix, int64_t mix_sb, int64_t mix_sv, int64_t mix_sc, const int64_t* extras,
                            int64_t n_pre, int64_t n_post, void* stream);

/* Forward STFT of real rows: what torch.stft(x, n_fft, hop, window, center=True, pad_mode="reflect", return_complex=True)
 * returns, out = (rows, n_fft / 2 + 1, 1 + T / hop) complex64 (interleaved re, im).  Replaces the torch.stft call of
 * STFTMaskedNoiseReverb.sample_noise (reverb.py:116-128, fixed_noise=False).  n_fft even, <= 2048; rows <= 65535. */
int gfx_stft_f32(const float* x, const float* window, float* out, int64_t rows, int64_t T, int64_t n_fft, int64_t hop,
                 void* stream);
/* ---- STFT-masked noise reverb: impulse response ------------------------------------------
 * replaces STFTMaskedNoiseReverb.compute_stft_mask + compute_ir (reverb.py:161-200: mask, torch.istft),
 * ms_to_lr (core/midside.py:4-8) and the energy of normalize_impulse (core/utils.py:14-18).
 * noise_stft: one noise spectrum shared by all rows (`noise_rows` = 1: (2, n_fft/2+1, num_frames) complex64 as interleaved
 * floats, the module's buffer) or one per row (`noise_rows` = R: (R, 2, n_fft/2+1, num_frames)) --
 * STFTMaskedNoiseReverb(fixed_noise=False) draws fresh noise for every row (reverb.py:63, 80-82, 165);
 * init/delta: (R, 2, n_fft/2+1); gain_env (nullable): (R, 2, num_frames); window: (n_fft).
 * Outputs ir (R, 2, ir_len), un-normalised, and row_gain (R) = 1/sqrt(mean_c sum_t ir^2 + 1e-12),
 * to be passed as `gain` (gain_div = 2) to gfx_fir_spectrum_f32.
 * `basis` is a per-(n_fft, window) constant from gfx_istft_basis_f32 (gfx_istft_basis_bytes: the windowed (kpad, n_fft)
 * matrix, the un-windowed half basis (n_fft/2+1, 2, roundup(n_fft/2+1, 16)) that the n_fft <= 384 matrix kernel uses, and
 * the n_fft complex factors e^(2 pi i k / n_fft), e^(2 pi i p / (n_fft/2)) of the FFT form, GFX_ISTFT_FFT below).
 * `schedule`: how the frames are transformed (same results to rounding):
 *   GFX_ISTFT_GEMM  the inverse real DFT of a frame as a matrix product on the fp32 matrix cores (any even n_fft), the frames
 *                   written to the workspace and overlap-added by a second kernel.
 *   GFX_ISTFT_FFT   n_fft = 384 with hop = 192 (the reference's defaults, reverb.py:48-49) only, else GFX_EINVAL: a 192-point
 *                   complex FFT per frame (eight lanes a frame, 8 x 24 points), windowed and overlap-added in LDS; one
 *                   workgroup finishes 31 blocks of 192 samples of both channels of a row -- ~70x less arithmetic, and the
 *                   frames never reach memory.
 *   GFX_ISTFT_AUTO  FFT where it applies.
 * Workspace: gfx_stft_reverb_workspace_bytes with the same schedule (the FFT form keeps no frames).
 */
#define GFX_ISTFT_AUTO 0
#define GFX_ISTFT_GEMM 1
#define GFX_ISTFT_FFT 2
size_t gfx_istft_basis_bytes(int64_t n_fft);
int gfx_istft_basis_f32(const float* window, float* basis, int64_t n_fft, void* stream);
size_t gfx_stft_reverb_workspace_bytes(int64_t R, int64_t ir_len, int64_t n_fft, int64_t hop, int64_t num_frames,
                                       int schedule);
int gfx_stft_reverb_ir_f32(const float* noise_stft, int64_t noise_rows, const float* init_log_magnitude,
                           const float* delta_log_magnitude, const float* gain_env_log_magnitude,
                           const float* window, const float* basis, float* ir, float* row_gain, int64_t R,
                           int64_t ir_len, int64_t n_fft, int64_t hop, int64_t num_frames, int ms_to_lr, void* ws,
                           size_t ws_bytes, int schedule, void* stream);
/* Backward of gfx_stft_reverb_ir_f32 in its FFT form (n_fft = 384, hop = 192, num_frames = 1 + ir_len / 192; anything else
 * is GFX_EINVAL): the gradients of the parameters from grad_ir = dL/dh (R, 2, ir_len), h the taps the forward call with the
 * same noise, parameters, window, basis and ms_to_lr produced.
 *   ir, row_gain both given: h = row_gain * ir (normalize_impulse applied), `ir` (R, 2, ir_len) and `row_gain` (R) being that
 *                            forward call's outputs;  both null: h = ir, the un-normalised taps.
 *   noise_stft / noise_rows, init, delta, gain_env (nullable), window, basis: as in the forward; the noise gets no gradient.
 * Outputs, each nullable (not computed), not all of them: g_init, g_delta (R, 2, 193); g_gain_env (R, 2, num_frames), which
 * needs gain_env.  Every element of a given output is written.
 * One workgroup takes 16 frames of both channels of a row: a 192-point complex FFT per frame, frames and spectra stay in
 * LDS.  Sums use no atomics: the per-workgroup bin sums and (normalised) the block sums of grad_ir * ir are stored in `ws`
 * (gfx_stft_reverb_ir_bwd_ws_bytes: R * (ceil(2 ir_len / 4096) + ceil(num_frames / 16) * 4 * 193) floats) and added in
 * double in a fixed order, so results are bit-identical from run to run.  Nothing is allocated or synchronised.
 * R <= 32767 per call. */
size_t gfx_stft_reverb_ir_bwd_ws_bytes(int64_t R, int64_t ir_len);
int gfx_stft_reverb_ir_bwd_f32(const float* grad_ir, const float* ir, const float* row_gain, const float* noise_stft,
                               int64_t noise_rows, const float* init_log_magnitude, const float* delta_log_magnitude,
                               const float* gain_env_log_magnitude, const float* window, const float* basis,
                               float* g_init, float* g_delta, float* g_gain_env, int64_t R, int64_t ir_len, int64_t n_fft,
                               int64_t hop, int64_t num_frames, int ms_to_lr, void* ws, size_t ws_bytes, void* stream);

/* ---- routing ----------------------------------------------------------------------------
 * replaces read_single_tensor("index") + aggregate_tensor("sum"/"scatter") + inplace_write_tensor
 * (reference src/grafx/render/core.py:36-50, 101-112, 80-98) for the (B, V, C, L) signal buffer:
 *   out[b, j, c, n] = sum_{e in [seg_ptr[j], seg_ptr[j+1])} buf[b, src_idx[e], c, n]
 * buf/out are addressed by (batch, node, channel) strides in floats; src_idx (E) and
 * seg_ptr (J+1) are int64 device arrays (edges sorted by destination).
 */
int gfx_gather_sum_f32(const float* buf, int64_t buf_sb, int64_t buf_sv, int64_t buf_sc,
                       const int64_t* src_idx, const int64_t* seg_ptr,
                       float* out, int64_t out_sb, int64_t out_sv, int64_t out_sc,
                       int64_t B, int64_t J, int64_t C, int64_t L, void* stream);
/* Same result for fan-out routing (one source feeding several of the J <= 32 destinations; more than 8 is the shape of
 * a routing sum's adjoint: a few bus gradients onto every strip): every
 * distinct source row unique_src[u] is read once and added to the destinations whose bit is set in
 * dest_mask[u].  Needs 16-byte aligned rows (returns GFX_EINVAL otherwise: use gfx_gather_sum_f32). */
int gfx_gather_sum_fanout_f32(const float* buf, int64_t buf_sb, int64_t buf_sv, int64_t buf_sc,
                              const int64_t* unique_src, const int64_t* dest_mask, int64_t U,
                              float* out, int64_t out_sb, int64_t out_sv, int64_t out_sc,
                              int64_t B, int64_t J, int64_t C, int64_t L, void* stream);

/* ---- exact recursive biquad cascade -------------------------------------------------------
 * replaces IIRFilter._process_lfilter / _process_ssm: core/iir.py:154-261 (torchaudio.functional.lfilter per
 * section / the state-space form on torchlpc).  K second-order sections in series per row-channel, zero initial
 * state, coefficients normalised by a0:  y = b0 w[n] + b1 w[n-1] + b2 w[n-2],  w[n] = x[n] - a1 w[n-1] - a2 w[n-2].
 * A parallel scan over time (matrix powers of the 2x2 transition matrix), no FFT.
 * Bs, As: (R, C_f, K, 3) contiguous; channels broadcast 1<->C like gfx_fftconv_f32; K <= 32.
 * ssm_quirk != 0 reproduces upstream's "ssm" backend for K > 1, which feeds the ORIGINAL input to the
 * recursive part of every section (core/iir.py:226-246); for K == 1 both settings are the same filter. */
int gfx_biquad_cascade_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* Bs,
                           const float* As, int64_t R, int64_t C_in, int64_t C_f, int64_t K, int64_t L, int ssm_quirk,
                           void* stream);
/* The same cascade with the filter state carried across calls, for block-wise processing of a long signal.
 * zi, zf: (R, C_out, K, 2) contiguous, C_out = max(C_in, C_f): per row-channel and section (w[n-1], w[n-2]) of the
 * a0-normalised direct-form-II recursion above -- zi the state entering sample 0, zf = (w[L-1], w[L-2]), the state
 * after the LAST sample (not after the kernel's zero-padded last tile).  Either may be NULL (zero state in / state not
 * stored), and zi == zf updates the state in place.  Under ssm_quirk the state is still every section's own w.
 * With zi = zf = NULL the output is that of gfx_biquad_cascade_f32. */
int gfx_biquad_cascade_state_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, const float* Bs,
                                 const float* As, const float* zi, float* zf, int64_t R, int64_t C_in, int64_t C_f,
                                 int64_t K, int64_t L, int ssm_quirk, void* stream);
/* Backward of the cascade (ssm_quirk = 0) without anything of the signal's size kept from the forward: everything is
 * rebuilt from x.  g = dL/dy (R, C_out, L) through gmap, gzf = dL/dzf (R, C_out, K, 2) or NULL (zero); zi as the forward
 * call had it (NULL: silence).  Outputs, each NULL when not wanted (not all of them): gx = dL/dx (R, C_in, L) through
 * gxmap, gB / gA = dL/dBs, dL/dAs (R, C_f, K, 3), gzi = dL/dzi (R, C_out, K, 2).  With C_out <= 2 channel broadcasts are
 * summed inside the call (a pair of row-channels is then a row's two channels).  With C_out > 2 a broadcast side cannot
 * be reduced here: gB / gA with C_f == 1, or gx with C_in == 1, return GFX_EINVAL -- pass the broadcast side expanded
 * to C_out channels (x through a row map with stride_ch = 0) and add the channels of the result, as grafx_amd/ops.py
 * does.  Every element of a given output is written.  With lam_i the adjoint state of section i
 * (lam[m] = r[m] - a1 lam[m+1] - a2 lam[m+2], r[m] = sum_d b_d g_i[m+d] + the zf cotangent at m = L-1, L-2) and w_i the
 * section's direct-form-II state:  g_{i-1} = lam_i, gx = lam_1,
 *   db_d = sum_n g_i[n] w_i[n-d],  da_d = -sum_n lam_i[n] w_i[n-d],  gB_d = db_d / a0,  gA_{1,2} = da / a0,
 *   gA_0 = -(b . db + a . da) / a0,  gzi = (r[-1] - a1 lam[0] - a2 lam[1], r[-2] - a2 lam[0]).
 * Two passes, one wave per pair of row-channels: a forward walk over x that stores every section's entering state per
 * 512-sample tile in `ws`, then a walk from the last tile to the first that rebuilds the sections' w from those and runs
 * the adjoint recursion.  No atomics; sums are taken per tile in fp32 in a fixed order and across tiles in double, so
 * results are bit-identical from run to run and a row's gradients do not depend on the other rows of the call.
 * gfx_biquad_cascade_bwd_ws_bytes = ceil(R * C_out / 2) * ceil(L / 512) * K * 16 bytes (0 for a zero or negative
 * argument); ws must be 16-byte aligned.  A workspace that is too small or bad geometry returns GFX_EINVAL before any
 * launch.  Nothing is allocated or synchronised.  K <= 32. */
size_t gfx_biquad_cascade_bwd_ws_bytes(int64_t R, int64_t C_out, int64_t K, int64_t L);
int gfx_biquad_cascade_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* g, gfx_rowmap_t gmap, float* gx,
                               gfx_rowmap_t gxmap, const float* Bs, const float* As, const float* zi, const float* gzf,
                               float* gB, float* gA, float* gzi, void* ws, size_t ws_bytes, int64_t R, int64_t C_in,
                               int64_t C_f, int64_t K, int64_t L, void* stream);

/* ---- noise-shaping reverb impulse response ------------------------------------------------
 * replaces the envelope synthesis of FilteredNoiseShapingReverb.forward (reverb.py:343-366):
 *   ir[r,c,t] = sum_k noise[c,k,t] * log_gain[r,c,k] * (exp(t*d) - sigmoid(z_fade_in_gain)*exp(t*f))
 *   d = sigmoid(log_decay)*(max_decay-min_decay)+min_decay,  f = sigmoid(log_fade_in)*(d-min_decay)+min_decay
 * (the fade-in term only when both fade pointers are non-null; the gain is the raw parameter, as upstream).
 * noise: (C, K, noise_stride) band-split noise, the first ir_len samples of every band row are used (pass an
 * offset pointer for the "pseudo-random" start).  Parameters (R, C, K) contiguous; ir (R, C, ir_len).  K <= 64. */
int gfx_noise_shaping_ir_f32(const float* noise, int64_t noise_stride, const float* log_decay, const float* log_gain,
                             const float* log_fade_in, const float* z_fade_in_gain, float* ir, int64_t R, int64_t C,
                             int64_t K, int64_t ir_len, float min_decay, float max_decay, void* stream);
/* Backward of gfx_noise_shaping_ir_f32: the gradients of the parameters from grad_ir = dL/dh (R, C, ir_len), h the taps the
 * forward call with the same noise (pointer and stride), parameters and decay range produced.
 *   ir, row_gain both given: h = row_gain * ir (normalize_impulse applied), `ir` (R, C, ir_len) being that forward call's
 *                            output and row_gain[r] = 1 / sqrt(mean_c sum_t ir[r,c,t]^2 + 1e-12) (R);
 *   both null:               h = ir, the un-normalised taps.
 * The fade pair is both null or both set, as in the forward.  Outputs (R, C, K), each nullable (not computed), not all of
 * them; g_log_fade_in and g_z_fade_in_gain need the fade pair.  Every element of a given output is written.
 * With e_d = exp(t d), e_f = exp(t f), fg = sigmoid(z_fade_in_gain) and v = dL/d(ir) (grad_ir, or for the normalised taps
 * row_gain grad_ir - row_gain^3 / C <grad_ir, ir>_row ir) the kernel takes, per (r, c, k), the four sums over t of
 * v noise {e_d, t e_d, e_f, t e_f}: one workgroup owns 2048 consecutive samples of one (r, c), keeps its grad_ir and ir
 * samples in registers and loops over the K bands.  No atomics: the per-workgroup sums (taken against grad_ir and against ir
 * separately, and the workgroup's share of <grad_ir, ir>) go to `ws` and a second kernel adds them in double in workgroup
 * order and applies the chain rule (sigmoid' = s (1 - s): 0 at a saturated parameter), so results are bit-identical from
 * run to run and a row's gradients do not depend on the other rows of the call.
 * gfx_noise_shaping_ir_bwd_ws_bytes = R * C * ceil(ir_len / 2048) * (8 K + 1) floats (0 for a zero or negative argument).
 * Nothing is allocated or synchronised.  K <= 64; R * C beyond one launch's grid is split on channel boundaries. */
size_t gfx_noise_shaping_ir_bwd_ws_bytes(int64_t R, int64_t C, int64_t K, int64_t ir_len);
int gfx_noise_shaping_ir_bwd_f32(const float* grad_ir, const float* ir, const float* row_gain, const float* noise,
                                 int64_t noise_stride, const float* log_decay, const float* log_gain,
                                 const float* log_fade_in, const float* z_fade_in_gain, float* g_log_decay,
                                 float* g_log_gain, float* g_log_fade_in, float* g_z_fade_in_gain, int64_t R, int64_t C,
                                 int64_t K, int64_t ir_len, float min_decay, float max_decay, void* ws, size_t ws_bytes,
                                 void* stream);

/* ---- memoryless waveshapers --------------------------------------------------------------
 * replaces the forward() of TanhDistortion (nonlinear.py:46-79), PiecewiseTanhDistortion (120-175),
 * PowerDistortion (210-233) and ChebyshevDistortion (270-307): one streaming pass.
 *   u = pre * (x - dc),  pre = exp(log_pre_gain[r]) (1 if null),  dc = dc[r*C + c] (0 if null)
 *   GFX_WS_TANH       y = tanh(u + b) - tanh(b),            b = p0[r] (0 if null)
 *   GFX_WS_PIECEWISE  p0 = log_hardness (R,2), p1 = z_threshold (R,2)  (upstream's split order is kept)
 *   GFX_WS_POWER      y = sum_k tanh(p0[r,k]) f(u^k),       k < K <= 32, f = tanh if use_tanh
 *   GFX_WS_CHEBYSHEV  y = sum_k tanh(p0[r,k]) f(T_k(u))
 * then y *= post, post = 1/pre if inverse_post_gain else exp(log_post_gain[r]) (1 if null).
 * gfx_row_mean_f32 computes the per-row-channel means the remove_dc option subtracts. */
#define GFX_WS_TANH 0
#define GFX_WS_PIECEWISE 1
#define GFX_WS_POWER 2
#define GFX_WS_CHEBYSHEV 3
int gfx_row_mean_f32(const float* x, gfx_rowmap_t xmap, float* mean, int64_t R, int64_t C, int64_t L, void* stream);
int gfx_waveshaper_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L,
                       int mode, int use_tanh, int inverse_post_gain, const float* log_pre_gain,
                       const float* log_post_gain, const float* p0, const float* p1, int64_t K, const float* dc,
                       void* stream);
/* Backward of gfx_waveshaper_f32 in one streaming pass over x and gy (same configuration, parameters and dc -- the
 * array gfx_row_mean_f32 produced for the forward; null without remove_dc).  With G = gy * post, s the shape before the
 * post gain:  gx = G s'(u) pre  (with dc: minus its own mean over time per row-channel, the adjoint of the centring),
 *   g_log_pre_gain (R)  = sum G (s'(u) u - [inverse_post_gain] s(u)),    g_log_post_gain (R) = sum G s(u),
 *   g_p0: (R) bias / (R,2) log_hardness / (R,K) basis weights,           g_p1: (R,2) z_threshold,
 * every sum over the row's C * L samples.  Each output may be null (not computed), not all of them; gx is addressed
 * through its own row map.  A gradient may only be asked for a parameter that was given
 * (g_log_post_gain: and used, i.e. not under inverse_post_gain).  Row sums are stored per workgroup in `ws`
 * (gfx_waveshaper_bwd_ws_bytes; K = 0 for the two tanh modes) and added in double in a fixed order: no atomics, results
 * are bit-identical from run to run.  ws may be null when only gx is asked and dc is null. */
size_t gfx_waveshaper_bwd_ws_bytes(int64_t R, int64_t C, int64_t L, int64_t K);
int gfx_waveshaper_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R, int64_t C,
                           int64_t L, int mode, int use_tanh, int inverse_post_gain, const float* log_pre_gain,
                           const float* log_post_gain, const float* p0, const float* p1, int64_t K, const float* dc,
                           float* gx, gfx_rowmap_t omap, float* g_log_pre_gain, float* g_log_post_gain, float* g_p0,
                           float* g_p1, void* ws, size_t ws_bytes, void* stream);

/* ---- oversampled (anti-aliased) waveshapers: interpolate by `factor`, shape, decimate, in one tile kernel ----
 * For every row-channel, with F = factor, xc = x - dc inside [0, L) and zero outside, taps zero outside [0, N):
 *   u[p] = sum_k xc[k] h_up[p + offset_up - k F]          0 <= p < F L
 *   v[p] = post s(pre u[p])                               0 <= p < F L, and zero outside (not s(0))
 *   y[m] = sum_p v[p] h_dn[m F + offset_dn - p]           0 <= m < L
 * s, pre, post, the modes and their parameters exactly those of gfx_waveshaper_f32; h_up and h_dn are device arrays
 * shared by every row.  The high-rate signals exist only in LDS: 8 bytes of traffic per sample.  y is addressed through its
 * own row map and may not share memory with x (tiles read each other's halos of x).
 * gfx_oversampled_waveshaper_bwd_f32 is the adjoint, with the outputs, the workspace rule and the refusals of
 * gfx_waveshaper_bwd_f32: gx is the input gradient (minus its mean per row-channel with dc), the parameter gradients are
 * the row sums of that entry taken over the F L high-rate samples, stored per tile and added in double in a fixed order
 * (no atomics, equal bits from run to run).  The taps get no gradient.
 *   gfx_oversampled_waveshaper_bwd_ws_bytes = 4 (R NS C nt + R C nt + R C),  nt = ceil(L / tile(factor)),
 *   NS = 2 + K (polynomial) or 6 (K = 0);  0 for a bad argument.
 * GFX_EINVAL before any launch: factor outside 1 .. 16, N_up or N_dn outside 1 .. 1024, an offset outside 0 .. N - 1, a null
 * filter, everything the waveshaper entries refuse, more than 2^31 - 1 workgroups (row-channels times tiles), a row map with
 * a negative stride, an output that overlaps an input.  A workspace that is too small is GFX_ENOSPC. */
int gfx_oversampled_waveshaper_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C,
                                   int64_t L, int64_t factor, const float* h_up, int64_t N_up, int64_t offset_up,
                                   const float* h_dn, int64_t N_dn, int64_t offset_dn, int mode, int use_tanh,
                                   int inverse_post_gain, const float* log_pre_gain, const float* log_post_gain,
                                   const float* p0, const float* p1, int64_t K, const float* dc, void* stream);
size_t gfx_oversampled_waveshaper_bwd_ws_bytes(int64_t R, int64_t C, int64_t L, int64_t K, int64_t factor);
int gfx_oversampled_waveshaper_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R,
                                       int64_t C, int64_t L, int64_t factor, const float* h_up, int64_t N_up,
                                       int64_t offset_up, const float* h_dn, int64_t N_dn, int64_t offset_dn, int mode,
                                       int use_tanh, int inverse_post_gain, const float* log_pre_gain,
                                       const float* log_post_gain, const float* p0, const float* p1, int64_t K,
                                       const float* dc, float* gx, gfx_rowmap_t omap, float* g_log_pre_gain,
                                       float* g_log_post_gain, float* g_p0, float* g_p1, void* ws, size_t ws_bytes,
                                       void* stream);

/* ---- look-ahead peak limiter with hold and FIR smoothing, in one tile kernel each way ----
 * For every row r of C channels, with T = exp(log_ceiling[r]), look-ahead D >= 0, hold H >= 0, window M = D + 1 + H and N
 * smoothing taps w (a device array shared by every row; the caller's: non-negative, summing to one):
 *   p[k]  = max_c |x[c, k]|                              x zero outside [0, L), or the state zi below 0
 *   pk[q] = max_{0 <= j < M} p[q - j]                    ties take the earliest index a(q)
 *   m[q]  = pk[q] > T ? T / pk[q] : 1
 *   s[n]  = sum_{0 <= j < N} w[j] m[n - j]               float32, from 0.0, ascending j
 *   y[c, n] = x[c, n + sigma - D] s[n + sigma]           0 <= n < L
 * sigma = 0 is the causal limiter of latency D, sigma = D the delay-compensated one.  N <= D + 1 makes |y| <= T up to
 * rounding.  zi / zf (null: none): the last S = M + N - 2 input samples, (R, C, S) contiguous, oldest first; zf is a copy of
 * the last S samples of zi || x, and blocks cut anywhere, each entering with the zf of the one before, give the bits of
 * the one-call output.  gain (null: not wanted): (R, L) contiguous, the applied s[n + sigma].  y is addressed through its
 * own row map and may not share memory with x (tiles read each other's halos of x).  Everything between x and y exists
 * in LDS only: 8 bytes of traffic per sample and channel.  Tile: T(M) = min(4096, max(1024, (155000 - 32 M) / 16 rounded
 * down to a multiple of 512)) samples of a row per workgroup; rows times tiles ride on grid.x.
 * gfx_limiter_bwd_f32 is the adjoint for a call without a state (gy, gx through their own row maps; either of gx and
 * g_log_ceiling (R) may be null, not both): the gradient of a window's maximum goes to the sample a(q), in the channel
 * of the lowest index that holds the peak.  The taps get no gradient.  The ceiling's sums are stored per tile in ws,
 *   gfx_limiter_bwd_ws_bytes = 8 R ceil(L / T(M)),   0 for a bad argument,
 * as doubles (ws 8-byte aligned) -- a tile's sum can be a thousand times the row's -- and added in a fixed order.  No atomics in either entry: equal bits from run to run, and a row's result does
 * not depend on the other rows of the call.
 * GFX_EINVAL before any launch: a null x, y / gy, log_ceiling or w; R, C or L <= 0; D or H < 0; M > 4096; N outside
 * 1 .. 1024 or above D + 1; sigma other than 0 and D; a state together with sigma > 0; zi overlapping zf; an empty row map
 * or one with a negative stride; an output that overlaps an input; more than 2^31 - 1 row-channels or workgroups; a
 * ceiling gradient without a workspace or with a misaligned one.  A workspace that is too small is GFX_ENOSPC. */
int gfx_limiter_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L,
                    const float* log_ceiling, const float* w, int64_t N, int64_t D, int64_t H, int64_t sigma, const float* zi,
                    float* zf, float* gain, void* stream);
size_t gfx_limiter_bwd_ws_bytes(int64_t R, int64_t L, int64_t D, int64_t H);
int gfx_limiter_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R, int64_t C, int64_t L,
                        const float* log_ceiling, const float* w, int64_t N, int64_t D, int64_t H, int64_t sigma, float* gx,
                        gfx_rowmap_t omap, float* g_log_ceiling, void* ws, size_t ws_bytes, void* stream);

/* ---- modulated delay line (chorus, vibrato, doubling): a delay whose length moves under a sine oscillator ----
 * For every row r of C channels and V voices, with p = pos_in[r] + n the absolute position of sample n (p = n without a
 * state), interp 0 (linear, j in {0, 1}) or 1 (third-order Lagrange on the nodes j in {-1, 0, 1, 2}):
 *   theta[v,c,n] = rate[r,v] p + phase[r,v,c]                            cycles; evaluated in double, reduced mod 1
 *   d[v,c,n]     = clamp(delay[r,v] + depth[r,v] sin(2 pi theta), 1, Dmax)    samples; in double
 *   i = floor(d),  f = float32(d - i)
 *   u[v,c,n]     = sum_j l_j(f) x[c, n - i - j]                          x zero, or the history zi, below the row's start
 *   y[c,n]       = dry[r] x[c,n] + sum_v gain[r,v,c] u[v,c,n]            0 <= n < L
 * linear: l_0 = 1 - f, l_1 = f.  cubic: l_-1 = -f(f-1)(f-2)/6, l_0 = (f+1)(f-1)(f-2)/2, l_1 = -(f+1)f(f-2)/2,
 * l_2 = (f+1)f(f-1)/6.  Dmax = max_delay, 2 .. 8192; V = 1 .. 8.  delay, depth, rate are (R, V), phase and gain (R, V, C),
 * dry (R), all contiguous.  y is one fmaf chain per sample: dry x first, then the voices ascending, then j ascending,
 * each term (gain l_j) x -- the same bits whatever tile, block or call a sample falls in.
 * The contract: 2 pi rate depth <= 1/2 samples per sample.  Then the read position n - i(n) never decreases and takes
 * each value at most twice, which the backward rests on.  Outside it (any finite parameters) every access stays inside
 * its buffer and the values are unspecified.
 * A state is the history zi / zf, the last S = Dmax + 2 input samples, (R, C, S) contiguous, oldest first, and the
 * position pos_in / pos_out, (R) int64 on the device: zf is a copy of the last S samples of zi || x, pos_out = pos_in + L,
 * and blocks cut anywhere, each entering with the state the one before left, give the bits of the one-call output.  zi
 * and pos_in are given together or both null (silence at position 0), so are zf and pos_out (null: not wanted).
 * y is addressed through its own row map and may not share memory with x.  Tile: 2048 samples of a row per workgroup,
 * the channels in turn; rows times tiles ride on grid.x.
 * gfx_moddelay_bwd_f32 is the adjoint for a call without a state (gy, gx through their own row maps).  Almost everywhere:
 * the clamp passes no gradient where it binds.  With e = gy gain sum_j l'_j(f) x[c, n - i - j]:
 *   gx[c,k] = dry gy[c,k] + sum_v gain sum_{n, j : n - i(n) - j = k} gy[c,n] l_j(f(n))    (float32, v then n ascending)
 *   g_gain[v,c] = sum_n gy u,  g_dry = sum_c sum_n gy x,  g_delay[v] = sum_c sum_n e,  g_depth[v] = sum_c sum_n e sin(2 pi theta),
 *   g_phase[v,c] = sum_n e depth 2 pi cos(2 pi theta),  g_rate[v] = sum_c sum_n e depth 2 pi cos(2 pi theta) p
 * Each of gx and the six parameter gradients (shaped like their parameters) may be null, not all.  The parameter
 * gradients are tile sums in double, stored in ws,
 *   gfx_moddelay_bwd_ws_bytes = 8 R ceil(L / 2048) (1 + 3 V + 2 V C),   0 for a bad argument,
 * (ws 8-byte aligned; not needed for gx alone) and added per row in a fixed order.  No atomics in either entry: equal bits
 * from run to run, and a row's result does not depend on the other rows of the call.
 * GFX_EINVAL before any launch: a null x, y / gy or parameter array; R, C or L <= 0; V outside 1 .. 8; interp other than
 * 0 and 1; max_delay outside 2 .. 8192; a history without a position or the reverse; zi overlapping zf or pos_in
 * pos_out; an empty row map or one with a negative stride; an output that overlaps an input; more than 2^31 - 1
 * row-channels or workgroups; nothing asked for; a parameter gradient without a workspace or with a misaligned one.  A
 * workspace that is too small is GFX_ENOSPC. */
int gfx_moddelay_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L, int64_t V,
                     int64_t interp, int64_t max_delay, const float* delay, const float* depth, const float* rate,
                     const float* phase, const float* gain, const float* dry, const float* zi, const int64_t* pos_in, float* zf,
                     int64_t* pos_out, void* stream);
size_t gfx_moddelay_bwd_ws_bytes(int64_t R, int64_t C, int64_t L, int64_t V);
int gfx_moddelay_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, int64_t R, int64_t C, int64_t L,
                         int64_t V, int64_t interp, int64_t max_delay, const float* delay, const float* depth, const float* rate,
                         const float* phase, const float* gain, const float* dry, float* gx, gfx_rowmap_t gxmap, float* g_delay,
                         float* g_depth, float* g_rate, float* g_phase, float* g_gain, float* g_dry, void* ws, size_t ws_bytes,
                         void* stream);

/* ---- feedback delay (echo, ping-pong): a delay line inside a damped feedback loop ----------
 * For every row r of C channels (C = 1 or 2), c, c' < C:
 *   i_c = floor(delay[r,c]),  f_c = delay[r,c] - i_c                     float32; 64 <= delay <= max_delay <= 65536
 *   s_c[n] = (1 - f_c) w_c[n - i_c] + f_c w_c[n - i_c - 1]               the line's output, linear interpolation
 *   q_c[n] = (1 - a[r,c]) s_c[n] + a[r,c] q_c[n - 1]                     the loop's one-pole damping, 0 <= a < 1
 *   w_c[n] = x_c[n] + sum_c' F[r,c,c'] q_c'[n]                           what enters the line
 *   y_c[n] = dry[r] x_c[n] + wet[r] q_c[n]                               0 <= n < L
 * delay and damping (a) are (R, C), feedback (F) is (R, C, C), dry and wet (R), all contiguous.  w and q are zero, or the
 * carried state, below the row's start.  The contract: max_c sum_c' |F[c,c']| < 1, 0 <= a < 1 and the delay's range.
 * Outside it (NaNs included) the delay is clamped to 64 .. max_delay before it is split, every access stays inside its
 * buffer, and the values are unspecified.
 * One workgroup walks a row, all channels together, in chunks of min(min_c i_c, 1024) samples; the rows ride on grid.x.
 * The line w lives in ws, (R, C, L) floats:  gfx_fbdelay_ws_bytes = 4 R C L,  0 for a bad argument.  After a call ws
 * holds w; q (nullable) receives the (R, C, L) contiguous signal q -- the two signals the backward reads.
 * A state is the history zi / zf, the last S = max_delay + 1 samples of w, (R, C, S) contiguous, oldest first, and q_in /
 * q_out, (R, C), the loop filter's last value.  zi and q_in are given together or both null (silence), so are zf and
 * q_out (null: not wanted).  The system is time-invariant: a state carries no position.  The chunk grid restarts at each
 * call, so blocks agree with the one call to rounding, not to the bit; the same sequence of calls gives the same bits.
 * y is addressed through its own row map and may not share memory with x.
 * gfx_fbdelay_bwd_f32 is the adjoint for a call without a state, from x, gy and the forward's q and w: n descending,
 *   lambda_c[n] = (1 - f_c) mu_c[n + i_c] + f_c mu_c[n + i_c + 1],  zeta_c[n] = wet gy_c[n] + sum_c' F[c',c] lambda_c'[n],
 *   mu_c[n] = (1 - a_c) zeta_c[n] + a_c mu_c[n + 1],                gx_c[n] = dry gy_c[n] + lambda_c[n],
 *   g_dry = sum_c sum_n gy x,  g_wet = sum_c sum_n gy q,  g_feedback[c,c'] = sum_n lambda_c q_c',
 *   g_delay[c] = sum_n mu_c (w_c[n - i_c - 1] - w_c[n - i_c]),  g_damping[c] = sum_n mu_c (q_c[n - 1] - s_c[n]) / (1 - a_c).
 * Each of gx and the five parameter gradients (shaped like their parameters) may be null, not all.  ws holds the tile
 * sums of the parameter gradients in double and the line mu:
 *   gfx_fbdelay_bwd_ws_bytes = 8 R ceil(L / 2048) (2 + 2 C + C C) + 4 R C L,   0 for a bad argument,
 * 8-byte aligned, always needed.  No atomics in either entry: equal bits from run to run, and a row's result does not
 * depend on the other rows of the call.
 * GFX_EINVAL before any launch: a null x, y / gy, q / w (backward) or parameter array; R, C or L <= 0; C > 2; max_delay
 * outside 64 .. 65536; a zi without q_in or the reverse, a zf without q_out or the reverse; zf overlapping zi; an empty
 * row map or one with a negative stride; an output that overlaps an input; more than 2^31 - 1 rows; nothing asked for; a
 * missing or misaligned workspace.  A workspace that is too small is GFX_ENOSPC. */
size_t gfx_fbdelay_ws_bytes(int64_t R, int64_t C, int64_t L);
int gfx_fbdelay_f32(const float* x, gfx_rowmap_t xmap, float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L,
                    int64_t max_delay, const float* delay, const float* damping, const float* feedback, const float* dry,
                    const float* wet, const float* zi, const float* q_in, float* zf, float* q_out, float* q, void* ws,
                    size_t ws_bytes, void* stream);
size_t gfx_fbdelay_bwd_ws_bytes(int64_t R, int64_t C, int64_t L);
int gfx_fbdelay_bwd_f32(const float* x, gfx_rowmap_t xmap, const float* gy, gfx_rowmap_t gmap, const float* q, const float* w,
                        int64_t R, int64_t C, int64_t L, int64_t max_delay, const float* delay, const float* damping,
                        const float* feedback, const float* dry, const float* wet, float* gx, gfx_rowmap_t gxmap, float* g_delay,
                        float* g_damping, float* g_feedback, float* g_dry, float* g_wet, void* ws, size_t ws_bytes, void* stream);

/* ---- multi-resolution STFT magnitude loss, one resolution per call ------------------------
 * replaces the call site of a training step's loss: torch.stft of the prediction and of the target, their magnitudes
 * and logs, and autograd through all of them.  For rows p = pred[r], t = target[r] of L samples,
 *   P = torch.stft(p, n_fft, hop, window=window, center=True, pad_mode="reflect", return_complex=True)   (T likewise)
 *   |P| = sqrt(max(P.re^2 + P.im^2, eps)),  |T| likewise
 *   sums[r] = (A, B, E, D) = (sum (|T|-|P|)^2, sum |T|^2, sum ||T|-|P||, sum |log|T| - log|P||)
 * over the n_fft / 2 + 1 bins of the 1 + L / hop frames; `window` holds n_fft floats.  The rows of pred, target and gpred
 * are single signals: row r lives at base + (r / inner) * stride_outer + (r % inner) * stride_inner of its row map
 * (stride_ch is not used), so the B * C rows of a (B, C, L) slice of a larger buffer are read in place.
 * gfx_stft_loss_sums_f32: one pass over pred and target; every workgroup transforms a run of consecutive frames in LDS
 * (one complex transform per frame: pred in the real part, target in the imaginary part) and leaves one partial
 * quadruple in `ws`; a second kernel adds a row's partials in their order, in double.  No atomics: equal bits from run
 * to run, and a row's sums do not depend on the other rows of the call.
 * gfx_stft_loss_bwd_f32: gpred[r] (=, or += with accumulate != 0) the gradient of cA A + cE E + cD D with respect to
 * pred[r], coef[r] = (cA, cE, cD).  Per bin, with live = P.re^2 + P.im^2 > eps,
 *   G = live * (2 cA (|P|-|T|) + cE sign(|P|-|T|) + cD sign(log|P|-log|T|) / |P|) * P / |P|
 * and a frame's gradient is window[j] * Re sum_{k <= n_fft/2} G_k e^{+2 pi i jk / n_fft} (every kept bin once),
 * overlap-added, the reflect padding folded back onto the samples it mirrors.  Gather form: a workgroup owns 4096
 * samples of a row, recomputes every frame that reaches them and stores each sample once -- no atomics, no zero-fill
 * before the call; the target gets no gradient.  Frames whose pred and target samples are the same floats count
 * |T|-|P| = 0 exactly in both entries.
 * n_fft: a power of two in [128, 2048]; 1 <= hop <= n_fft; n_fft / 2 < L <= 2^31 - 4097; eps > 0; anything else, a
 * null pointer (ws included), R <= 0 or an empty row map is GFX_EINVAL; a workspace below
 *   gfx_stft_loss_ws_bytes = R * ceil((1 + L / hop) * n_fft / 16384) * 16 bytes   (0 for a bad argument)
 * is GFX_ENOSPC (ws 16-byte aligned).  The backward takes the same workspace so that one buffer serves both calls of a
 * step; it launches nothing that touches it today.  Every check comes before the first launch. */
size_t gfx_stft_loss_ws_bytes(int64_t R, int64_t L, int64_t n_fft, int64_t hop);
int gfx_stft_loss_sums_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap, const float* window,
                           float* sums, int64_t R, int64_t L, int64_t n_fft, int64_t hop, float eps, void* ws,
                           size_t ws_bytes, void* stream);
int gfx_stft_loss_bwd_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap, const float* window,
                          const float* coef, float* gpred, gfx_rowmap_t gmap, int64_t R, int64_t L, int64_t n_fft,
                          int64_t hop, float eps, int accumulate, void* ws, size_t ws_bytes, void* stream);

/* ---- the same loss on a filterbank scale (mel, bark, third octaves, per-bin weights, a band limit) ----
 * fb is an (n_bins, n_fft / 2 + 1) matrix W of non-negative weights, dense and row-major.  With |P|_k, |T|_k per bin
 * and frame as above (the clamp stays on the bins),
 *   Pm[m] = sum_k W[m, k] |P|_k,   Tm[m] likewise,
 *   sums[r] = (A, B, E, D) = (sum (Tm-Pm)^2, sum Tm^2, sum |Tm-Pm|, sum |log Tm - log Pm|)
 * over the n_bins bands of the 1 + L / hop frames (the logarithm moves to the bands), and gfx_stft_band_loss_bwd_f32
 * gives the gradient of cA A + cE E + cD D with respect to pred[r]: per band and per bin
 *   g_m = 2 cA (Pm-Tm) + cE sign(Pm-Tm) + cD sign(log Pm - log Tm) / Pm
 *   G_k = live_k * (sum_m W[m, k] g_m) * P_k / |P|_k,     live_k = P.re^2 + P.im^2 > eps,
 * followed by the windowed one-sided inverse, the overlap-add and the reflection fold of gfx_stft_loss_bwd_f32.
 * Staircase contract: the non-zeros of row m are one run [row_lo[m], row_hi[m]) of bins, not empty and of positive
 * weight sum (so that log Pm exists), and row_lo, row_hi are non-decreasing in m.  The rows that touch bin k are then a
 * run too, [col_lo[k], col_hi[k]) (n_fft / 2 + 1 entries each; empty for a bin no row covers, whose G_k is 0).  Only
 * the band entries of fb are read.  The band arrays (int32, on the device) and the non-negativity of fb are the
 * caller's to guarantee: the entries cannot read device memory before a launch.  The kernels cut every run to
 * [0, n_fft / 2 + 1) and [0, n_bins), so wrong arrays give wrong numbers, not reads outside fb.
 * Rows, row maps, window, workspace (gfx_stft_loss_ws_bytes, the same buffer), accumulate, the treatment of frames whose
 * pred and target samples are the same floats, and the guarantees (no atomics, equal bits from run to run, a fixed group
 * of lanes reduces a band whatever its width, every gradient sample stored once) are those of the plain entries.
 * Refused with GFX_EINVAL: everything the plain entries refuse, a null fb or band array, n_bins outside
 * 1 .. n_fft / 2 + 1; a workspace too small is GFX_ENOSPC.  Every check comes before the first launch. */
int gfx_stft_band_loss_sums_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap,
                                const float* window, const float* fb, const int32_t* row_lo, const int32_t* row_hi,
                                int64_t n_bins, float* sums, int64_t R, int64_t L, int64_t n_fft, int64_t hop, float eps,
                                void* ws, size_t ws_bytes, void* stream);
int gfx_stft_band_loss_bwd_f32(const float* pred, gfx_rowmap_t pmap, const float* target, gfx_rowmap_t tmap,
                               const float* window, const float* fb, const int32_t* row_lo, const int32_t* row_hi,
                               const int32_t* col_lo, const int32_t* col_hi, int64_t n_bins, const float* coef, float* gpred,
                               gfx_rowmap_t gmap, int64_t R, int64_t L, int64_t n_fft, int64_t hop, float eps, int accumulate,
                               void* ws, size_t ws_bytes, void* stream);

/* ---- block energies behind a two-section biquad cascade with shared coefficients (ITU-R BS.1770 K-weighting) ----
 * Every row-channel of x (R rows of C channels through a row map with a channel stride, as gfx_biquad_cascade_f32: a
 * (B, C, L) slice of a (B, n, C, L) render buffer is read in place) goes through
 *   w_i[n] = u_{i-1}[n] - a1 w_i[n-1] - a2 w_i[n-2],   u_i[n] = b0 w_i[n] + b1 w_i[n-1] + b2 w_i[n-2],   i = 1, 2,
 * u_0 = x, y = u_2, from silence, and leaves
 *   energy[r, c, k] = sum of y[n]^2 over k * hop <= n < (k + 1) * hop,   k < n_sub = L / hop (floor)
 * as (R, C, n_sub) contiguous doubles; samples from n_sub * hop on belong to no sub-block.  `coef` is ten doubles in HOST
 * memory, (b0, b1, b2, a1, a2) per section, a0-normalised, shared by the whole call and read at the call: the powers of
 * the cascade's 4 x 4 state matrix that join runs of samples are built from it on the host.  Recursion, states, squares
 * and sums are in double; x is read as float32.
 * gfx_kweight_energy_bwd_f32: gx (=, or += with accumulate != 0) the gradient of sum genergy * energy with respect to x,
 * genergy (R, C, n_sub) contiguous doubles: with v[n] = 2 genergy[n / hop] y[n] (0 from n_sub * hop on) it is the adjoint
 * cascade applied to v, the same recursion run over the reversed signal.  y is rebuilt from x; nothing of the signal's
 * size is kept between the two calls.  Every gradient sample is stored once, float32, through gmap (as xmap).
 * Tile: 1024 samples of a row-channel per wave; rows may be of any length, a single long row is spread over the device.
 * No atomics: equal bits from run to run, and a row-channel's results do not depend on the other rows of the call.
 * Any hop in 1 .. L.  GFX_EINVAL: a null pointer (ws included), R, C or L <= 0, hop outside 1 .. L, an empty row map, a
 * coefficient that is not finite (or so large that a power of the state matrix is not), energy / genergy not 8-byte or ws
 * not 16-byte aligned, more than 2^31 - 1 row-channels or 2^33 - 4 tiles; a workspace below
 *   gfx_kweight_energy_ws_bytes = R * C * ceil(L / 1024) * 64 bytes   (0 for a zero or negative argument)
 * is GFX_ENOSPC.  One buffer serves both entries: per tile the entering state of the forward recursion (32 bytes) and
 * the parts of the sub-blocks that cross its edges, or the adjoint's entering state.  Every check comes before the
 * first launch. */
size_t gfx_kweight_energy_ws_bytes(int64_t R, int64_t C, int64_t L);
int gfx_kweight_energy_f32(const float* x, gfx_rowmap_t xmap, const double* coef, double* energy, int64_t R, int64_t C,
                           int64_t L, int64_t hop, void* ws, size_t ws_bytes, void* stream);
int gfx_kweight_energy_bwd_f32(const float* x, gfx_rowmap_t xmap, const double* coef, const double* genergy, float* gx,
                               gfx_rowmap_t gmap, int64_t R, int64_t C, int64_t L, int64_t hop, int accumulate, void* ws,
                               size_t ws_bytes, void* stream);

/* ---- rational polyphase FIR ("upfirdn"): sample-rate conversion, its adjoint, and the oversampled peak ----
 * Every row-channel of x (R rows of C channels of L samples through a row map with a channel stride, as
 * gfx_kweight_energy_f32: a (B, C, L) slice of a (B, n, C, L) render buffer is read and written in place) gives
 *   y[r, c, m] = sum_k x[r, c, k] h[m * down + offset - k * up],   0 <= m < M,
 * x zero outside [0, L), h zero outside [0, N): N float32 taps on the device, shared by every row.  About N / up products
 * per output.  y is stored once per sample through ymap (=, or += with accumulate != 0).  M is the caller's: any M >= 1;
 * outputs whose tap window misses [0, L) entirely are 0.0.  The adjoint with respect to x is the same entry with up and
 * down exchanged, the taps reversed, offset' = N - 1 - offset and M' = L.
 * Tile: GFX_UPFIRDN_TILE consecutive outputs of one row-channel per workgroup; the taps and the span of x under the tile
 * (under a part of it where down / up is large) are staged in LDS.  The tile's base index m * down + offset is formed in 64
 * bits.  Each output accumulates in float32 over ascending k: equal bits from run to run, and a row-channel's result does
 * not depend on the other rows of the call (taps {1.0f} with up = down = 1 return x's bits).  No workspace, no atomics.
 * gfx_upfirdn_absmax_f32 runs the same tiles without writing y and leaves, per row-channel, peak[r, c] = max_m |y[m]|
 * (R * C floats) and index[r, c] (R * C int64_t), the LOWEST m that attains it (0.0 and 0 for an all-zero row): per-tile
 * (value, index) pairs go to the workspace, a second kernel reduces a row's pairs.  No atomics.
 *   gfx_upfirdn_absmax_ws_bytes = R * C * ceil(M / GFX_UPFIRDN_TILE) * 16 bytes   (0 for a zero or negative argument)
 * GFX_EINVAL: a null pointer (ws included), R, C, L or M <= 0, an empty row map, up or down outside 1 .. 1024, N outside
 * 1 .. 16384, offset outside 0 .. N - 1, more than 2^31 - 1 row-channels or tiles in the call, ws not 16-byte or index not
 * 8-byte aligned; a workspace that is too small is GFX_ENOSPC.  Every check comes before the first launch. */
#define GFX_UPFIRDN_TILE 1024
int gfx_upfirdn_f32(const float* x, gfx_rowmap_t xmap, const float* h, int64_t N, int64_t up, int64_t down, int64_t offset,
                    float* y, gfx_rowmap_t ymap, int64_t R, int64_t C, int64_t L, int64_t M, int accumulate, void* stream);
size_t gfx_upfirdn_absmax_ws_bytes(int64_t R, int64_t C, int64_t M);
int gfx_upfirdn_absmax_f32(const float* x, gfx_rowmap_t xmap, const float* h, int64_t N, int64_t up, int64_t down,
                           int64_t offset, float* peak, int64_t* index, int64_t R, int64_t C, int64_t L, int64_t M, void* ws,
                           size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GRAFX_AMD_H */
