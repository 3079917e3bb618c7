"""Tensor-level wrappers over the C ABI (include/grafx_amd.h).

These take torch CUDA(=HIP) tensors, hand raw device pointers and the current
stream to libgrafx_amd.so and return torch tensors.  torch is only the memory
and stream plumbing; all arithmetic happens in the HIP kernels.  CPU tensors are
rejected: there is no fallback path.
"""
import ctypes
import os
from collections import namedtuple

import torch

from ._lib import RowMap, check, lib
from ._plumbing import (_apart, _cotangent, _expect, _int_in, _on_device, _output, _overlap, _pair_state, _param_grads,  # noqa: F401
                        _Pin, _ptr, _require_gpu, _row_chunks, _signal_grad, _state, _stream, _taps, _timed, _want, _workspace,
                        profiling, rowmap)


# The aliasing rule (include/grafx_amd.h): no tensor a call writes shares an element with one it reads, with another it
# writes, or with itself.  Every wrapper that writes caller memory names both sides where it takes them: ``apart=`` of
# _output for ``out``, _apart for what is written beside it (tee, zf, u1_out, odd_alias's out).  The read side is every
# signal, gradient, envelope, state and kept scan.  Left out: the small per-row parameter tensors and filter taps, which go
# through pin() / .contiguous(), and the opaque byte buffers the library's own wrappers make (spectra, plans).


# ----------------------------------------------------------------------------------------- FIR conv
def part_len_for(N, Lout):
    """Partition length the library prefers for an N-tap filter producing Lout samples per row (0 = default)."""
    return lib().gfx_fftconv_part_len(N, Lout)


@_on_device
def fir_spectrum(h, gain=None, gain_div=1, part_len=0):
    """Taps (RCf, N) -> opaque tile-spectrum buffer for :func:`fftconv` (same ``part_len`` there)."""
    _require_gpu(h, gain)
    h = h.contiguous()
    RCf, N = h.shape
    Hs = torch.empty(lib().gfx_fir_spectrum_bytes(RCf, N, part_len), dtype=torch.uint8, device=h.device)
    check(lib().gfx_fir_spectrum_f32(_ptr(h), _ptr(gain), gain_div, _ptr(Hs), RCf, N, part_len, _stream()),
          "gfx_fir_spectrum_f32")
    return Hs


@_on_device
def fir_spectrum_reversed(x, part_len=0):
    """Spectra of the time-reversed rows of ``x`` ((R,C,L) or a strided (B,n,C,L) view, read in place): what
    ``fir_spectrum(x.flip(-1).reshape(R * C, L), part_len=part_len)`` returns, without the flipped copy."""
    _require_gpu(x)
    xmap, R, C, L = rowmap(x)
    Hs = torch.empty(lib().gfx_fir_spectrum_bytes(R * C, L, part_len), dtype=torch.uint8, device=x.device)
    check(lib().gfx_fir_spectrum_rev_f32(_ptr(x), xmap, R, C, L, part_len, _ptr(Hs), _stream()),
          "gfx_fir_spectrum_rev_f32")
    return Hs


@_on_device
def fir_grad(x, g, N, off):
    """gh[r,c,k] = sum_n g[r,cg,n] x[r,cx,n+off-k], k < N <= 8193: the filter gradient of a short-filter convolution
    in one pass over x and g ((R,C,L) tensors or strided (B,n,C,L) views) -> (R, max(Cx,Cg), N)."""
    _require_gpu(x, g)
    xmap, R, Cx, L = rowmap(x)
    gmap, Rg, Cg, Lg = rowmap(g)
    if Rg != R:
        raise ValueError(f"fir_grad: {Rg} gradient rows for {R} signal rows")
    gh = torch.empty((R, max(Cx, Cg), N), dtype=torch.float32, device=x.device)
    with _timed("corr1_kernel", 4 * R * (Cx * L + Cg * Lg)):
        check(lib().gfx_fir_grad_f32(_ptr(x), xmap, _ptr(g), gmap, _ptr(gh), R, Cx, Cg, L, Lg, N, off, _stream()),
              "gfx_fir_grad_f32")
    return gh


def fftconv_can_tee(Cin, Cf, L, Lout, off, N):
    """Whether :func:`fftconv` can also write a copy of its input (the conditions of gfx_fftconv_f32's xcopy)."""
    return off == 0 and Lout >= L and Cin >= Cf and lib().gfx_fftconv_nparts(N) == 1


GFX_EINVAL = -1                                  # include/grafx_amd.h
GRID_YZ_MAX = 65535                              # workgroups along the second / third dimension of one launch
GRID_ROWS_I16_MAX = 32767                        # rows per launch of the kernels whose grids index rows in 16 bits (reverb)
SCHEDULES = {"auto": 0, "tile": 1, "pipe": 2}   # GFX_SCHED_* of include/grafx_amd.h
# What `schedule="auto"` means to fftconv(): "auto" (the library decides: the persistent hand-scheduled kernel for large
# launches it covers) or "pipe" (prefer that kernel at every size it covers -- tests and latency experiments).
FFTCONV_SCHEDULE = "auto"
# the full-length convolution in front of the odd-length aliasing leaves the rows' maxima for its pair scaling (round 6;
# False: the aliasing takes them in a pass of its own over z, as for every other producer of z)
ROWMAX_BYPRODUCT = True


@_on_device
def fftconv(x, Hs, N, Cf, Lout=None, off=0, out=None, tee=None, h_rows=None, part_len=0, schedule="auto", rowmax=None,
            zi=None, return_state=False):
    """y[r,c,n] = sum_k h[r % h_rows,cf,k] x[r,cx,n+off-k], n < Lout (x zero outside [0,L)).

    ``x`` / ``out`` may be (R,C,L) tensors or strided (B,n,C,L) views (see :func:`rowmap`).
    ``tee``: optional tensor shaped like ``x`` that receives a copy of ``x`` from the same kernel.
    ``h_rows``: number of filters in ``Hs`` when fewer than the signal rows (rows are batch-major, so
    ``h_rows = nodes`` shares one filter per node across the batch); default: one filter per row.
    ``schedule``: "auto" (the library picks), "tile" (one tile per workgroup, compiler-scheduled) or "pipe" (the
    hand-scheduled persistent kernel, N <= 8193); see gfx_fftconv_f32.
    ``rowmax`` (with schedule "auto"): a dict that receives ``rowmax["words"]`` -- an int32 tensor of R * max(C, Cf) words,
    the bits of max |y| of every output row-channel -- when the kernel that ran leaves them as a by-product
    (gfx_fftconv_f32's rowmax: the compiler-built tile kernels, one partition or many); untouched otherwise.  For odd_alias(rowmax=).
    ``zi`` / ``return_state``: block-wise processing, see :func:`fftconv_state` (causal only: ``off`` = 0, ``Lout`` = L; no
    ``tee``, ``rowmax`` or ``part_len``); with ``return_state`` the result is ``(y, zf)``.
    """
    if zi is not None or return_state:
        # the stateful entry is the causal convolution on the tile schedule and nothing else: say which argument does not go
        # with a carried history instead of ignoring it
        why = None
        if tee is not None:
            why = "tee: the input copy comes from the stateless one-partition kernels only"
        elif rowmax is not None:
            why = "rowmax: the row maxima feed the odd-length aliasing of one whole-signal call, which has no block form"
        elif part_len != 0:
            why = "part_len: a stateful call always takes the default partition geometry"
        elif off != 0:
            why = f"off={off}: a carried history is the past of a causal convolution (off = 0)"
        elif Lout is not None and Lout != x.shape[-1]:
            why = f"Lout={Lout}: a block of L samples gives L samples (the tail lives in the state, not in the output)"
        elif schedule not in ("auto", "tile"):
            why = f"schedule={schedule!r}: a stateful call always takes the tile schedule"
        if why is not None:
            raise ValueError(f"fftconv: zi / return_state cannot be combined with {why}")
        y, zf = fftconv_state(x, Hs, N, Cf, zi=zi, out=out, h_rows=h_rows, return_state=return_state)
        return (y, zf) if return_state else y
    _require_gpu(x, out, tee)
    xmap, R, Cin, L = rowmap(x)
    Lout = L if Lout is None else Lout
    Cout = max(Cin, Cf)
    h_rows = R if h_rows is None else h_rows
    _apart("fftconv", "tee", tee, (x,))
    out, ymap = _output(out, (R, Cout, Lout), x.device, "fftconv", longer=True, apart=(x, tee))
    if Hs.numel() != lib().gfx_fir_spectrum_bytes(h_rows * Cf, N, part_len):
        raise ValueError(f"filter spectra hold {Hs.numel()} bytes, expected {h_rows} x {Cf} filters of {N} taps")
    pin = _Pin()
    ws = pin.workspace(lib().gfx_fftconv_workspace_bytes(R, Cin, L, Lout, off, N, part_len), x.device)
    cmap = RowMap(1, 0, 0, 0)
    if tee is not None:
        cmap, Rc, Cc, Lc = rowmap(tee)
        if (Rc, Cc, Lc) != (R, Cin, L):
            raise ValueError(f"tee shape {tuple(tee.shape)} does not match the input {tuple(x.shape)}")
    want_max = rowmax is not None and schedule == "auto" and FFTCONV_SCHEDULE == "auto" and ROWMAX_BYPRODUCT
    words = torch.zeros(R * Cout, dtype=torch.int32, device=x.device) if want_max else None
    written = ctypes.c_int(0)

    def launch(sched):
        return lib().gfx_fftconv_f32(_ptr(x), xmap, _ptr(Hs), h_rows, part_len, _ptr(out), ymap, _ptr(tee), cmap, R, Cin, Cf,
                                     L, Lout, off, N, *ws, SCHEDULES[sched], _ptr(words),
                                     ctypes.byref(written) if want_max else None, _stream())

    # the record is keyed by the kernel's own name, as a profile prints it
    with _timed("fftconv", 4 * R * ((2 if tee is not None else 1) * Cin * L + Cout * Lout), last="gfx_fftconv_last_kernel"):
        rc = GFX_EINVAL
        if schedule == "auto" and FFTCONV_SCHEDULE == "pipe":
            rc = launch("pipe")
            if rc not in (0, GFX_EINVAL):  # only "not covered by the persistent kernel" falls back to the library's choice;
                check(rc, "gfx_fftconv_f32 (pipe)")   # a failed launch / code-object load must not be masked
        if rc != 0:
            check(launch(schedule), "gfx_fftconv_f32")
    if written.value:
        rowmax["words"] = words
    return out


@_on_device
def fftconv_state(x, Hs, N, Cf, zi=None, out=None, h_rows=None, return_state=True, zf=None, schedule="auto"):
    """One block of a streamed causal convolution: y[r,c,n] = sum_k h[r % h_rows,cf,k] xx[r,cx,n-k], n < L, where xx is
    the block ``x`` preceded by the carried history ``zi`` (R, C_in, N - 1), oldest sample first (None: silence), and
    zf = the last N - 1 samples of ``zi || x`` (a copy: bit-exact, also when L < N - 1 and the old history shifts).
    gfx_fftconv_state_f32: the window loader of the tile kernels reads the history in place -- no concatenated copy of
    the signal, no allocation beyond ``out`` / ``zf`` (pass both for none at all).  Blocks of a signal cut anywhere, each
    entering with the ``zf`` of the one before, concatenate to the linear convolution of the whole.

    ``x`` / ``out``: (R,C,L) tensors or strided (B,n,C,L) views; ``zf``: optional destination of the state (apart from
    ``x``, ``zi`` and ``out``); ``schedule``: "auto" or "tile" (never the persistent kernels).  -> (out, zf); zf is None
    unless ``return_state`` or a ``zf`` destination is given."""
    _require_gpu(x, out)
    if schedule not in ("auto", "tile"):
        raise ValueError(f"fftconv_state: schedule must be 'auto' or 'tile' (a stateful call never takes the persistent "
                         f"kernels), got {schedule!r}")
    xmap, R, Cin, L = rowmap(x)
    Cout = max(Cin, Cf)
    h_rows = R if h_rows is None else h_rows
    shape = (R, Cin, N - 1)      # rows, input channels, taps - 1: the input history, oldest sample first
    zi = _state(zi, shape, "fftconv_state", "zi")
    zf = _state(zf, shape, "fftconv_state", "zf")
    _apart("fftconv_state", "zf", zf, (x, zi))        # (the state is written while the history may still be read)
    out, ymap = _output(out, (R, Cout, L), x.device, "fftconv_state", longer=True, apart=(x, zi, zf))
    if Hs.numel() != lib().gfx_fir_spectrum_bytes(h_rows * Cf, N, 0):
        raise ValueError(f"filter spectra hold {Hs.numel()} bytes, expected {h_rows} x {Cf} filters of {N} taps")
    if zf is None and return_state:
        zf = torch.empty(shape, dtype=torch.float32, device=x.device)
    pin = _Pin()
    ws = pin.workspace(lib().gfx_fftconv_workspace_bytes(R, Cin, L, L, 0, N, 0), x.device)
    with _timed("fftconv", 4 * R * (Cin * (L + 2 * (N - 1)) + Cout * L), last="gfx_fftconv_last_kernel"):
        check(lib().gfx_fftconv_state_f32(_ptr(x), xmap, _ptr(Hs), h_rows, _ptr(out), ymap, _ptr(zi), _ptr(zf), R, Cin, Cf, L,
                                          N, *ws, SCHEDULES[schedule], _stream()), "gfx_fftconv_state_f32")
    return out, zf


@_on_device
def fir_direct(x, h, Lout=None, off=0, out=None, h_rows=None):
    """Short FIR (N <= 512 taps) on the fp32 matrix cores, taps given directly: same result as
    ``fftconv(x, fir_spectrum(h.reshape(-1, N)), N, Cf, Lout, off)``.  ``h``: (h_rows, Cf, N)."""
    _require_gpu(x, h, out)
    xmap, R, Cin, L = rowmap(x)
    h = h.contiguous()
    hr, Cf, N = h.shape
    h_rows = hr if h_rows is None else h_rows
    if hr != h_rows:
        raise ValueError(f"fir_direct: {hr} filter rows given, h_rows={h_rows}")
    Lout = L if Lout is None else Lout
    Cout = max(Cin, Cf)
    out, ymap = _output(out, (R, Cout, Lout), x.device, "fir_direct", longer=True, apart=(x,))
    with _timed("fir_mfma_kernel", 4 * R * (Cin * L + Cout * Lout)):
        check(lib().gfx_fir_direct_f32(_ptr(x), xmap, _ptr(h), h_rows, _ptr(out), ymap, R, Cin, Cf, L, Lout, off, N, _stream()),
              "gfx_fir_direct_f32")
    return out


# ----------------------------------------------------------------------------------------- small inverse real DFT
IRDFT_MAX_N = 8192


class FftLibraryWarning(UserWarning):
    """A parameter-sized transform left the library's own kernels for torch.fft (rocFFT): see fft_library_reached."""


def fft_library_reached(what):
    """The few parameter-sized transforms that are longer than the direct-sum / tile kernels cover (DESIGN.md section 8:
    never a signal, never on a BASELINE configuration) go to torch.fft -- and say so, once per call site."""
    import warnings

    warnings.warn(f"{what}: beyond the native transform sizes, computed by torch.fft (rocFFT)", FftLibraryWarning, stacklevel=3)


@_on_device
def irdft(X, n, roll=0, window=None):
    """irfft(X, n) for short transforms (n <= 8192, any n) as a direct sum on the GPU, rolled by ``roll`` and windowed:
    X (..., n//2 + 1) real or complex64 -> (..., n) float32 (gfx_irdft_f32)."""
    _require_gpu(window)
    if not X.is_cuda:
        _require_gpu(X)
    K = X.shape[-1]
    is_real = not X.is_complex()
    if X.dtype not in (torch.float32, torch.complex64):
        raise TypeError(f"irdft: float32 / complex64 input expected, got {X.dtype}")
    if window is not None and (window.dtype != torch.float32 or window.numel() != n):
        raise ValueError(f"irdft: the window must hold {n} float32 values, got {tuple(window.shape)} {window.dtype}")
    flat = (X if is_real else torch.view_as_real(X.contiguous())).reshape(-1, K, *(() if is_real else (2,))).contiguous()
    rows = flat.shape[0]
    y = torch.empty((rows, n), dtype=torch.float32, device=X.device)
    if rows == 0:        # an empty shard (gather_outputs / shard_batch produce them): torch.fft.irfft returned empty too
        return y.view(*X.shape[:-1], n)
    pin = _Pin()
    check(lib().gfx_irdft_f32(_ptr(flat), int(is_real), _ptr(y), rows, K, n, roll, pin(window), _stream()), "gfx_irdft_f32")
    return y.view(*X.shape[:-1], n)


@_on_device
def rdft(x, n=None):
    """rfft(x, n) along the last axis for short transforms (n <= 8192, any n) as a direct sum on the GPU (gfx_rdft_f32):
    x (..., n) float32 -> (..., n//2 + 1) complex64."""
    _require_gpu(x)
    n = x.shape[-1] if n is None else n
    if x.shape[-1] != n:
        raise ValueError(f"rdft: {x.shape[-1]} samples per row, n = {n}")
    K = n // 2 + 1
    flat = x.reshape(-1, n).contiguous()
    rows = flat.shape[0]
    X = torch.empty((rows, K, 2), dtype=torch.float32, device=x.device)
    for i, m in _row_chunks(rows, GRID_YZ_MAX):
        check(lib().gfx_rdft_f32(_ptr(flat[i:]), _ptr(X[i:]), m, K, n, _stream()), "gfx_rdft_f32")
    return torch.view_as_complex(X).view(*x.shape[:-1], K)


# ----------------------------------------------------------------------------------------- odd-length aliasing
_ALIAS_PLANS = {}          # (P, device) -> plan, most recently used last; at most _ALIAS_PLANS_MAX entries (up to 36 MB each, 72 MB precise)
_ALIAS_PLANS_MAX = max(1, int(os.environ.get("GRAFX_ALIAS_PLANS", "8")))


def set_alias_plan_cache(entries):
    """How many chirp plans of the odd-length aliasing (one per distinct P = Lx + Lh - 1 and precision, up to 36 / 72 MB
    each) stay cached per process; default 8, or GRAFX_ALIAS_PLANS.  A workload with many distinct lengths (ragged
    batches through upstream's default even tap counts) rebuilds a plan -- one small kernel chain and a stream
    synchronisation -- whenever a length falls out of the cache: size it to the number of distinct lengths in flight."""
    global _ALIAS_PLANS_MAX
    _ALIAS_PLANS_MAX = max(1, int(entries))



def odd_alias_supported(P):
    """Whether gfx_odd_alias_f32 handles a linear convolution of odd length P (3 <= P <= 11,184,811)."""
    return lib().gfx_odd_alias_plan_bytes(P) > 0


# Two real rows per complex chirp-z transform (csrc/czt_pair.hip) in odd_alias's forward calls: a third fewer bytes
# through every pass.  GRAFX_ALIAS_PAIRS=0 keeps one transform per row (round 4's path; also what rows beyond
# P = 8 388 607 and every adjoint take).
ALIAS_PAIRS = os.environ.get("GRAFX_ALIAS_PAIRS", "1") != "0"
ALIAS_ROWS_PER_CHUNK = int(os.environ.get("GRAFX_ALIAS_ROWS", "1024"))   # rows of one launch chain (and ALIAS_WS_CAP bytes at most)
ALIAS_ONE_ROW_MAX = 16383    # rows one call of gfx_odd_alias_f32 / _adjoint_f32 accepts (csrc/czt.hip: czt_alias)


_AliasFns = namedtuple("_AliasFns", "plan_bytes workspace_bytes plan forward adjoint tag")


def _alias_fns(precise, pairs=False):
    """The entries of the fp32 or the double-precision transforms and the prefix of their names; ``pairs``: the
    two-rows-per-transform forms (forward only: adjoint is None)."""
    L, tag = lib(), "gfx_odd_alias_" + ("pair_" if pairs else "") + ("precise_" if precise else "")
    return _AliasFns(getattr(L, tag + "plan_bytes"), getattr(L, tag + "workspace_bytes"), getattr(L, tag + "plan_f32"),
                     getattr(L, tag + "f32"), None if pairs else getattr(L, tag + "adjoint_f32"), tag)


def _alias_pairs(P, rows):
    """Whether a forward call of `rows` rows of length P goes two rows per transform."""
    return ALIAS_PAIRS and rows >= 2 and lib().gfx_odd_alias_pair_plan_bytes(P) > 0


def _alias_plan(P, device, precise=False, pairs=False):
    """The per-P chirp plan of the aliasing kernels (LRU of _ALIAS_PLANS_MAX, built on first use)."""
    fns = _alias_fns(precise, pairs)
    key = (P, device.type, device.index, bool(precise), bool(pairs))
    plan = _ALIAS_PLANS.pop(key, None)
    if plan is not None:
        _ALIAS_PLANS[key] = plan   # back in as the most recent
    if plan is None:
        if torch.cuda.is_current_stream_capturing():
            # a plan built during capture would live in the graph's private pool and be rebuilt on every replay
            raise RuntimeError(f"odd_alias: no plan for P={P} yet; run the call once outside the HIP-graph capture")
        plan = torch.empty(fns.plan_bytes(P), dtype=torch.uint8, device=device)
        w1 = torch.empty(fns.workspace_bytes(1, P), dtype=torch.uint8, device=device)
        check(fns.plan(_ptr(plan), P, _ptr(w1), w1.numel(), _stream()), fns.tag + "plan_f32")
        torch.cuda.current_stream(device).synchronize()   # the cached plan is complete before any stream can pick it up
        _ALIAS_PLANS[key] = plan
        while len(_ALIAS_PLANS) > _ALIAS_PLANS_MAX:
            old = _ALIAS_PLANS.pop(next(iter(_ALIAS_PLANS)))
            torch.cuda.synchronize(old.device)               # nobody on any stream still reads the evicted plan
            del old
    plan.record_stream(torch.cuda.current_stream(device))
    return plan


def built_once(cache, key, build, device, what):
    """``cache[key]`` for a device-side table that is built once and kept (the Bluestein plan of the fsm filters, the
    inverse-STFT bases and window envelope of the reverb, the delay table of the fsm taps' backward): on a miss ``build()``
    launches it on the current stream, and that stream is synchronised before the value enters the cache -- as
    :func:`_alias_plan` does, a cached table is complete before any other stream can pick it up.  A hit is one dict
    lookup.  A miss under a HIP-graph capture raises: the table would live in the graph's private pool."""
    if key in cache:
        return cache[key]
    on_gpu = device.type == "cuda"      # (a CPU tensor is refused by the entry the table is for, not here)
    if on_gpu and torch.cuda.is_current_stream_capturing():
        raise RuntimeError(f"{what}: not built yet; run the call once outside the HIP-graph capture")
    value = build()
    if on_gpu:
        torch.cuda.current_stream(device).synchronize()
    cache[key] = value
    return value


ALIAS_WS_CAP = 4 << 30     # bytes of chirp-z workspace per launch chain (rows go through in chunks that fit it; 1 -> 4 GB:
                           # -6 % on the console's 4608 equaliser rows, tools/czt_chunk_ab.py).  Never more than a quarter
                           # of the memory that is free when the call is made, and halved (down to one row) when the
                           # allocation fails: a workload that fitted with the 1 GB chains of round 3 still fits.


def set_alias_workspace_cap(nbytes):
    """Upper bound, in bytes, of the transient chirp-z workspace one odd_alias / odd_alias_adjoint launch chain may hold
    (default 4 GiB; the effective bound is also a quarter of the free device memory).  Returns the previous value."""
    global ALIAS_WS_CAP
    old, ALIAS_WS_CAP = ALIAS_WS_CAP, max(int(nbytes), 1)
    return old


def _alias_chunks(rows, P, rows_per_chunk, device, ws_bytes, pairs=False):
    cap = ALIAS_WS_CAP
    if not torch.cuda.is_current_stream_capturing():
        # free to this process = what the driver has left + what torch's caching allocator holds without using it
        # (in a long-running / training process the cache holds most of the device: the driver's figure alone would
        # collapse the chunks to a few rows)
        free = torch.cuda.mem_get_info(device)[0] + torch.cuda.memory_reserved(device) - torch.cuda.memory_allocated(device)
        cap = min(cap, max(free // 4, 1))
    unit = 2 if pairs else 1            # chunks of whole pairs: row 2r stays with row 2r + 1
    if not pairs:                       # the one-transform-per-row entries take ALIAS_ONE_ROW_MAX rows per call
        rows_per_chunk = min(rows_per_chunk, ALIAS_ONE_ROW_MAX)
    chunk = max(unit, min(rows, rows_per_chunk, unit * (cap // ws_bytes(unit, P))) // unit * unit)
    if chunk >= rows:
        chunk = rows
    while True:
        try:
            return chunk, torch.empty(ws_bytes(chunk, P), dtype=torch.uint8, device=device)
        except torch.OutOfMemoryError:
            if chunk <= unit:
                raise
            chunk = max(unit, chunk // 2 // unit * unit)


@_on_device
def odd_alias(z, lo=0, length=None, rows_per_chunk=None, precise=False, out=None, rowmax=None, relu=False):
    """irfft_{P-1}(rfft_P(z))[..., lo : lo + length] for z (..., P), P odd: the reference convolve()'s aliasing of a
    full linear convolution (core/convolution.py:123-126), on the chirp-z kernels.  Rows go through in chunks (1.6 MB of
    workspace per row at P ~ 135 k: 25 tiles of 8192 points).  ``precise``: transforms in double precision (twice the
    workspace), for results that feed a logarithm -- the energy envelope, core/envelope.py:34-49.
    ``rowmax``: int32 words, one per row of z, holding the bits of max |z| of the row (what fftconv(rowmax=) leaves): the
    two-rows-per-transform form then skips its own pass over z.  ``relu`` (with ``precise`` and pairs): the last pass stores
    max(y, 0) -- the envelope smoother's clamp (core/envelope.py:48) without a pass of its own."""
    _require_gpu(z)
    P = z.shape[-1]
    Q = P - 1
    length = Q - lo if length is None else length
    rows = z.numel() // P
    into, omap, Co = out is not None, None, 0
    if into:
        # ``out``: a (R, C, length) tensor or a strided (B, n, C, length) view whose rows, channels flattened, are z's
        # rows: the last column pass writes them in place (the entries' ymap; float transforms only)
        _require_gpu(out)
        rmap, Ro, Co, Lo = rowmap(out)
        if precise or Ro * Co != rows or Lo != length:
            raise ValueError(f"odd_alias: out {tuple(out.shape)} does not take {rows} rows of {length} samples")
        _apart("odd_alias", "out", out, (z, rowmax))     # before the plan, the workspace or a copy of z is made
        omap = ctypes.byref(rmap)
    flat = z.reshape(-1, P).contiguous()
    rows_per_chunk = ALIAS_ROWS_PER_CHUNK if rows_per_chunk is None else rows_per_chunk
    pairs = _alias_pairs(P, rows)
    plan = _alias_plan(P, z.device, precise, pairs)
    fns = _alias_fns(precise, pairs)
    chunk, ws = _alias_chunks(rows, P, rows_per_chunk, z.device, fns.workspace_bytes, pairs)
    if rowmax is not None and (not pairs or rowmax.numel() != rows or rowmax.dtype != torch.int32 or not rowmax.is_cuda):
        rowmax = None
    if relu and not (pairs and precise and out is None):
        raise ValueError("odd_alias: relu is fused into the two-rows-per-transform double-precision form only")
    if not into:
        out = torch.empty((rows, length), dtype=torch.float32, device=z.device)
    # one record per chunk: the column / tile / column passes of the two chirp-z transforms (czt.hip), read z + write y
    name = (("czt_pair_in_kernel+czt_rows_kernel+czt_pair_mid_kernel+czt_pair_out_kernel" if pairs
             else "czt_cols_fwd_kernel+czt_rows_kernel+czt_cols_inv_kernel") + ("<double>" if precise else "<float>"))
    for i, n in _row_chunks(rows, chunk):
        rm = None if rowmax is None else rowmax[i : i + n].data_ptr()
        # what follows the workspace in the entry's list: the double forms take no row map, the one-row forms no maxima
        tail = ((rm, int(relu)) if pairs else ()) if precise else (omap, Co, i) + ((rm,) if pairs else ())
        with _timed(name, 4 * n * (P + length)):
            check(fns.forward(_ptr(flat[i : i + n]), _ptr(out if into else out[i : i + n]), length, lo, length, n, P,
                              _ptr(plan), _ptr(ws), ws.numel(), *tail, _stream()), fns.tag + "f32")
    return out if into else out.view(*z.shape[:-1], length)


@_on_device
def odd_alias_adjoint(gy, P, lo=0, rows_per_chunk=1024, precise=False):
    """Transpose of odd_alias: the gradient with respect to z (..., P) given gy (..., length), the gradient with respect
    to odd_alias(z, lo, length) -- what autograd derives from the reference's rfft / irfft pair."""
    _require_gpu(gy)
    length = gy.shape[-1]
    plan = _alias_plan(P, gy.device, precise)
    fns = _alias_fns(precise)
    flat = gy.reshape(-1, length).contiguous()
    rows = flat.shape[0]
    out = torch.empty((rows, P), dtype=torch.float32, device=gy.device)
    chunk, ws = _alias_chunks(rows, P, rows_per_chunk, gy.device, fns.workspace_bytes)
    for i, n in _row_chunks(rows, chunk):
        check(fns.adjoint(_ptr(flat[i : i + n]), length, lo, length, _ptr(out[i : i + n]), n, P, _ptr(plan), _ptr(ws),
                          ws.numel(), _stream()), fns.tag + "adjoint_f32")
    return out.view(*gy.shape[:-1], P)


# ----------------------------------------------------------------------------------------- IIR (FSM)
def iir_fsm_native(N):
    """Whether the library has a native tap kernel for fsm_fir_len = N (1..4096, 8192, 16384)."""
    return bool(lib().gfx_iir_fsm_native(N))


def iir_fsm_plan(N, device):
    nbytes = lib().gfx_iir_fsm_plan_bytes(N)
    if nbytes == 0:
        if iir_fsm_native(N):
            return None  # power-of-two lengths above the Bluestein limit need no plan
        raise NotImplementedError(f"fsm_fir_len={N}: the HIP FSM kernels support 1 <= fsm_fir_len <= 4096, 8192 and 16384")
    plan = torch.empty(nbytes, dtype=torch.uint8, device=device)
    check(lib().gfx_iir_fsm_plan_f32(_ptr(plan), N, _stream()), "gfx_iir_fsm_plan_f32")
    return plan


@_on_device
def iir_fsm_fir(Bs, As, N, plan):
    """(R, Cf, K, 3) biquad coefficients -> (R*Cf, N) frequency-sampled FIR taps.  float64 coefficients take the
    double-precision response evaluation (gfx_iir_fsm_fir_f64c_f32); the taps are float32 either way."""
    if Bs.dtype == torch.float64 and As.dtype == torch.float64:
        if not (Bs.is_cuda and As.is_cuda):
            _require_gpu(Bs.float(), As.float())
    else:
        _require_gpu(Bs, As)
    Bs, As = Bs.contiguous(), As.contiguous()
    K = Bs.shape[-2]
    RC = Bs.numel() // (K * 3)
    h = torch.empty((RC, N), dtype=torch.float32, device=Bs.device)
    if Bs.dtype == torch.float64:   # coefficients carried in double precision (gfx_iir_fsm_fir_f64c_f32): float32 taps
        if As.dtype != torch.float64:
            raise TypeError("iir_fsm_fir: Bs and As must have the same dtype")
        check(lib().gfx_iir_fsm_fir_f64c_f32(Bs.data_ptr(), As.data_ptr(), _ptr(plan), _ptr(h), RC, K, N, _stream()),
              "gfx_iir_fsm_fir_f64c_f32")
        return h
    check(lib().gfx_iir_fsm_fir_f32(_ptr(Bs), _ptr(As), _ptr(plan), _ptr(h), RC, K, N, _stream()), "gfx_iir_fsm_fir_f32")
    return h


@_on_device
def iir_fsm_bwd(Bs, As, G, delays, N, want_B=True, want_A=True):
    """Gradient of iir_fsm_fir's taps with respect to (R, Cf, K, 3) float32 coefficients from G = rfft(dL/dh, n = N)
    ((R, Cf, N // 2 + 1) complex64) and the forward pass's (3, N // 2 + 1) complex64 delay table: one native launch in double
    precision (gfx_iir_fsm_bwd_f32) -> (gB, gA), None for the one not wanted."""
    _require_gpu(Bs, As)
    if not (G.is_cuda and delays.is_cuda):
        _require_gpu(torch.view_as_real(G), torch.view_as_real(delays))
    Bs, As = Bs.contiguous(), As.contiguous()
    K = Bs.shape[-2]
    RC = Bs.numel() // (K * 3)
    F = N // 2 + 1
    if G.dtype != torch.complex64 or delays.dtype != torch.complex64 or G.numel() != RC * F or tuple(delays.shape) != (3, F):
        raise ValueError(f"iir_fsm_bwd: G {tuple(G.shape)} {G.dtype} / delays {tuple(delays.shape)} {delays.dtype} do not "
                         f"match {RC} filters of {N} taps")
    Gr, Dr = torch.view_as_real(G.contiguous()), torch.view_as_real(delays.contiguous())
    gB = torch.empty_like(Bs) if want_B else None
    gA = torch.empty_like(As) if want_A else None
    check(lib().gfx_iir_fsm_bwd_f32(_ptr(Bs), _ptr(As), _ptr(Gr), _ptr(Dr), _ptr(gB), _ptr(gA), RC, K, N, _stream()),
          "gfx_iir_fsm_bwd_f32")
    return gB, gA


@_on_device
def peq_coeffs(w0, q_inv, log_gain, use_shelving=True):
    _require_gpu(w0, q_inv, log_gain)
    w0, q_inv, log_gain = w0.contiguous(), q_inv.contiguous(), log_gain.contiguous()
    K = w0.shape[-1]
    n = w0.numel() // K
    Bs = torch.empty((*w0.shape, 3), dtype=torch.float32, device=w0.device)
    As = torch.empty_like(Bs)
    check(lib().gfx_peq_coeffs_f32(_ptr(w0), _ptr(q_inv), _ptr(log_gain), _ptr(Bs), _ptr(As), n, K, int(use_shelving), _stream()),
          "gfx_peq_coeffs_f32")
    return Bs, As


@_on_device
def peq_coeffs_bwd(w0, q_inv, log_gain, gBs, gAs, use_shelving=True):
    """Gradient of :func:`peq_coeffs` -> (g_w0, g_q_inv, g_log_gain), each shaped like w0."""
    _require_gpu(w0, q_inv, log_gain, gBs, gAs)
    w0, q_inv, log_gain = w0.contiguous(), q_inv.contiguous(), log_gain.contiguous()
    _expect(gBs, (*w0.shape, 3), "peq_coeffs_bwd: gBs")
    _expect(gAs, (*w0.shape, 3), "peq_coeffs_bwd: gAs")
    K = w0.shape[-1]
    out = [torch.empty_like(w0) for _ in range(3)]
    pin = _Pin()
    check(lib().gfx_peq_coeffs_bwd_f32(_ptr(w0), _ptr(q_inv), _ptr(log_gain), pin(gBs), pin(gAs),
                                       *(_ptr(o) for o in out), w0.numel() // K, K, int(use_shelving), _stream()),
          "gfx_peq_coeffs_bwd_f32")
    return tuple(out)


@_on_device
def biquad_coeffs(Bs_in, A1_pre, A2_pre, A0=None):
    _require_gpu(Bs_in, A1_pre, A2_pre, A0)
    Bs_in, A1_pre, A2_pre = Bs_in.contiguous(), A1_pre.contiguous(), A2_pre.contiguous()
    A0 = None if A0 is None else A0.contiguous()
    Bs = torch.empty_like(Bs_in)
    As = torch.empty_like(Bs_in)
    check(lib().gfx_biquad_coeffs_f32(_ptr(Bs_in), _ptr(A1_pre), _ptr(A2_pre), _ptr(A0), _ptr(Bs), _ptr(As), A1_pre.numel(), _stream()),
          "gfx_biquad_coeffs_f32")
    return Bs, As


# ----------------------------------------------------------------------------------------- dynamics
KNEES = {"hard": 0, "quadratic": 1, "exponential": 2}


def _rowvec(p, R):
    if p is None:
        return None
    _require_gpu(p)
    p = p.contiguous()
    if p.numel() != R:
        raise ValueError(f"per-row parameter has {p.numel()} elements for {R} rows")
    return p


def _curve(pin, log_threshold, log_ratio, log_knee, P):
    """The pointers of the compressor curve's three per-row parameters (P rows each), in the entries' order."""
    return pin(_rowvec(log_threshold, P)), pin(_rowvec(log_ratio, P)), pin(_rowvec(log_knee, P))


# Default schedule of dynamics_fused: "oneshot" hands the library a workspace, with which the smoothed configuration runs
# as dependency-free 1024-sample tiles for every row whose smoother memory is short (decided per row on the device,
# gfx_dynamics_fused_f32) and as one workgroup per row for the others; "rows" forces one workgroup per row.
MIX_FUSION = True          # dynamics stages take the routing sum that follows them (see dynamics_fused(mix=))
DYN_SCHEDULE = "oneshot"
# the compressor backward without a kept scan rebuilds it inside its tiles (gfx_dynamics_bwd_f32 with a workspace); False: a
# pass over every row writes it out first (the same entry without one, rounds 2-5)
DYN_BWD_RESCAN = True
# rows with a long smoother memory stay on the tile grid (gfx_dynamics_ws_bytes_ex); False: round 4
DYN_LOOKBACK = True


def mix_schedule(dest_sources, n):
    """The schedule of gfx_dynamics_fused_mix_f32 for a routing sum over the n rows of a graph: ``dest_sources[d]`` = the
    rows (strictly increasing) added into destination d, counted from the stage's first row -- 0 .. n-1 are the stage's
    own rows, negative numbers and numbers >= n are finished rows of the buffer before / behind them ("extras").  A
    destination occupies an accumulator from its first to its last source; live ranges are coloured greedily.
    -> (codes (list of n ints), accumulators used, pre, post) with pre / post = [(row, code), ...] for the extras in
    front of / behind the stage's rows; or None when a destination has no source, its rows are not increasing, no
    destination takes any of the stage's rows, or more than four destinations are live at once."""
    if not dest_sources or len(dest_sources) > 254:
        return None
    for rows in dest_sources:
        if not rows or any(b <= a for a, b in zip(rows, rows[1:])):
            return None
    if not any(0 <= r < n for rows in dest_sources for r in rows):
        return None
    pre = sorted({r for rows in dest_sources for r in rows if r < 0})
    post = sorted({r for rows in dest_sources for r in rows if r >= n})
    pos = {r: k for k, r in enumerate(pre)}
    pos.update({j: len(pre) + j for j in range(n)})
    pos.update({r: len(pre) + n + k for k, r in enumerate(post)})
    codes, free_at, slot = [0] * (len(pre) + n + len(post)), [0] * 4, {}
    for d in sorted(range(len(dest_sources)), key=lambda d: pos[dest_sources[d][0]]):
        first, last = pos[dest_sources[d][0]], pos[dest_sources[d][-1]]
        a = next((k for k in range(4) if free_at[k] <= first), None)
        if a is None:
            return None
        free_at[a], slot[d] = last + 1, a
        for r in dest_sources[d]:
            codes[pos[r]] |= 1 << a
        codes[last] |= (d + 1) << (8 + 8 * a)
    return (codes[len(pre) : len(pre) + n], max(slot.values()) + 1, list(zip(pre, codes[: len(pre)])),
            list(zip(post, codes[len(pre) + n :])))


_Mix = namedtuple("_Mix", "out sched n_acc extras n_pre n_post skip_rows")


def _read_mix(mix, B, n, C, L):
    """The ``mix`` dictionary of :func:`dynamics_fused` / :func:`stereo_gain` behind a (B, n, ., L) stage that writes C
    channels -> its values (``n_post``: the extras behind the stage's rows), or None when ``mix["out"]`` is no (B, J, C, L)
    view with a unit last stride or the schedule does not hold n codes."""
    mo, sched, ex = mix["out"], mix["sched"], mix.get("extras")
    if mo.shape != (B, mo.shape[1], C, L) or mo.stride(-1) != 1 or sched.numel() != n:
        return None
    n_pre = mix.get("n_pre", 0)
    return _Mix(mo, sched, mix["n_acc"], ex, n_pre, (0 if ex is None else ex.shape[0]) - n_pre, bool(mix.get("skip_rows")))


def _mix_args(m, n):
    """What the fused-mix entries take of a :func:`_read_mix` result, in their order (a mono sum has no channel stride)."""
    mo = m.out
    return (_ptr(m.sched), n, m.n_acc, _ptr(mo), mo.stride(0), mo.stride(1), mo.stride(2) if mo.shape[2] == 2 else 0,
            _ptr(m.extras), m.n_pre, m.n_post)


@_on_device
def dynamics_fused(x, log_threshold, log_ratio, log_knee, z_alpha, smoother, iir_len, knee, gate, out=None,
                   param_rows=None, schedule=None, u1_out=None, mix=None):
    """``param_rows``: number of parameter rows when shared across the batch (row r uses r % param_rows).
    ``schedule``: "oneshot" (default) or "rows", see above.
    ``u1_out``: optional (R, L) tensor that receives the smoother's un-truncated scan for :func:`dynamics_bwd` (the
    training forward; smoother = 1 only).
    ``mix``: a dict {"sched": int64 device tensor (n,), "n_acc": int, "out": (B, J, C, L) view, optionally "extras": int64
    device tensor (n_pre + n_post, 2) of (row offset from ``out``'s first row, code) and "n_pre"} for a strided
    (B, n, C, L) input (see :func:`mix_schedule`) -- the routing sum that follows is computed by the same kernel
    (gfx_dynamics_fused_mix_f32) and ``mix["done"]`` is set; when the configuration cannot take it, nothing is summed and
    ``mix["done"]`` stays unset (the caller runs the gather-sum stage)."""
    schedule = DYN_SCHEDULE if schedule is None else schedule
    if schedule not in ("oneshot", "rows"):
        raise ValueError(f"dynamics_fused: unknown schedule {schedule!r}")
    _require_gpu(x, out)
    xmap, R, C, L = rowmap(x)
    P = R if param_rows is None else param_rows
    if u1_out is not None:
        _require_gpu(u1_out)
        _expect(u1_out, (R, L), "dynamics_fused: u1_out")
        if not u1_out.is_contiguous() or smoother != 1:
            raise ValueError("dynamics_fused: u1_out must be contiguous and needs the one-pole smoother")
        _apart("dynamics_fused", "u1_out", u1_out, (x,))
    # (mix["out"] is outside the rule: its sources are row numbers held on the device, and reading them back would
    # synchronise; the render's planner keeps the destinations out of the sources -- render/plans.py, tests/test_mix_schedule.py)
    out, ymap = _output(out, (R, C, L), x.device, "dynamics_fused", apart=(x, u1_out))
    pin = _Pin()
    tiled = smoother == 1 and schedule == "oneshot"
    ws = pin.workspace(tiled and (lib().gfx_dynamics_ws_bytes_ex(P, R, L) if DYN_LOOKBACK else lib().gfx_dynamics_ws_bytes(P)),
                       x.device)
    args = (_ptr(x), xmap, _ptr(out), ymap, *_curve(pin, log_threshold, log_ratio, log_knee, P), pin(_rowvec(z_alpha, P)),
            P, R, C, L, smoother, iir_len, KNEES[knee], int(gate), _ptr(u1_out), *ws, _stream())
    kept = 4 * R * L if u1_out is not None else 0
    if mix is not None and tiled and MIX_FUSION and x.ndim == 4 and out.ndim == 4:
        n = x.shape[1]
        m = _read_mix(mix, x.shape[0], n, C, L)
        if m is not None and xmap.inner == n == ymap.inner:
            # the records are keyed by the kernel's own name, as a profile prints it
            with _timed("dyn_fused_kernel", (4 if m.skip_rows else 8) * R * C * L + 4 * m.out.numel() + kept,
                        last="gfx_dynamics_last_kernel") as t:
                # mix["skip_rows"]: nobody but these sums reads the stage's rows (an output-only render): do not store them
                rc = lib().gfx_dynamics_fused_mix_f32(*args[:-1], *_mix_args(m, n), int(m.skip_rows), _stream())
                if rc != 0:
                    t.last = None
            if rc == 0:
                mix["done"] = True
                return out
            if rc != GFX_EINVAL:   # not a configuration of the fused kernel
                check(rc, "gfx_dynamics_fused_mix_f32")
    with _timed("dyn_fused_kernel", 8 * R * C * L + kept, last="gfx_dynamics_last_kernel"):
        check(lib().gfx_dynamics_fused_f32(*args), "gfx_dynamics_fused_f32")
    return out


@_on_device
def dyn_gain_bwd(x, gy, env, log_threshold, log_ratio, log_knee, knee, gate):
    """-> (gain (R,L), denv (R,L), gparams (R,3) = d/d(log_threshold, log_ratio, log_knee)); see the header."""
    _require_gpu(x, gy, env)
    xmap, R, C, L = rowmap(x)
    gmap = _cotangent("dyn_gain_bwd", gy, x, (R, C, L))
    _expect(env, (R, L), "dyn_gain_bwd: env")
    env = env.contiguous()
    gain, denv = torch.empty_like(env), torch.empty_like(env)
    gp = torch.zeros((R, 3), dtype=torch.float32, device=x.device)
    pin = _Pin()
    check(lib().gfx_dyn_gain_bwd_f32(_ptr(x), xmap, _ptr(gy), gmap, _ptr(env), *_curve(pin, log_threshold, log_ratio, log_knee, R),
                                     R, C, L, KNEES[knee], int(gate), _ptr(gain), _ptr(denv), _ptr(gp), _stream()),
          "gfx_dyn_gain_bwd_f32")
    return gain, denv, gp


@_on_device
def dynamics_bwd(x, gy, log_threshold, log_ratio, log_knee, z_alpha, iir_len, knee, gate, out=None, pole=True, u1=None,
                 schedule=None, rescan=None):
    """Fused backward of the smoothed compressor / gate -> (gx (R,C,L), gparams (R,3), dalpha (R) or None).
    ``out``: optional destination for gx ((R,C,L) or a strided (B,n,C,L) view).  ``dalpha`` is the gradient with
    respect to the clamped pole a = min(sigmoid(z_alpha), 1 - 1e-5); the caller applies the chain rule to z_alpha.
    ``u1``: the scan kept by the forward pass (``dynamics_fused(..., u1_out=)``); without it the scan is recomputed --
    inside the backward tiles for rows with a short smoother memory (``rescan``, default DYN_BWD_RESCAN: the scratch the
    other rows' scan goes to is allocated but normally never touched), or by a pass of its own over every row.
    ``schedule`` (with ``u1``): "oneshot" (default, see DYN_SCHEDULE) or "rows"."""
    _require_gpu(x, gy, out)
    xmap, R, C, L = rowmap(x)
    gmap = _cotangent("dynamics_bwd", gy, x, (R, C, L))
    kept = u1 is not None
    if kept:
        _require_gpu(u1)
        _expect(u1, (R, L), "dynamics_bwd: u1")
    gx, gxmap = _output(out, (R, C, L), x.device, "dynamics_bwd", apart=(x, gy, u1))
    gp = torch.empty((R, 3), dtype=torch.float32, device=x.device)
    da = torch.empty(R, dtype=torch.float32, device=x.device) if pole else None
    pin = _Pin()
    # the kept scan (with or without the tiles' workspace), or a scratch the scan is rebuilt into (inside the tiles with a
    # workspace, by a pass of its own over every row without)
    if kept:
        need_ws = (DYN_SCHEDULE if schedule is None else schedule) == "oneshot"   # one-shot tiles for the short-memory rows
    else:
        u1 = torch.empty((R, L), dtype=torch.float32, device=x.device)
        need_ws = bool(DYN_BWD_RESCAN if rescan is None else rescan)
    check(lib().gfx_dynamics_bwd_f32(_ptr(x), xmap, _ptr(gy), gmap, *_curve(pin, log_threshold, log_ratio, log_knee, R),
                                     pin(_rowvec(z_alpha, R)), R, C, L, iir_len, KNEES[knee], int(gate), _ptr(gx), gxmap,
                                     _ptr(gp), pin(u1), 0 if kept else 1, _ptr(da),
                                     *pin.workspace(need_ws and lib().gfx_dynamics_bwd_ws_bytes(R, L), x.device), _stream()),
          "gfx_dynamics_bwd_f32")
    return gx, gp, da


@_on_device
def onepole_dz(g, U, D, coef, N):
    """Row sums sum_n g[n] (c0 U[n] + c2 U[n-N]) + g[n+1] (c1 D[n] + c3 D[n-N]); coef (R,4)."""
    _require_gpu(g, U, D, coef)
    R, L = g.shape
    _expect(U, (R, L), "onepole_dz: U")
    _expect(D, (R, L), "onepole_dz: D")
    _expect(coef, (R, 4), "onepole_dz: coef")
    da = torch.empty(R, dtype=torch.float32, device=g.device)
    pin = _Pin()
    check(lib().gfx_onepole_dz_f32(pin(g), pin(U), pin(D), pin(coef), _ptr(da), R, L, N, _stream()), "gfx_onepole_dz_f32")
    return da


@_on_device
def dyn_dx(x, gy, gain, de):
    _require_gpu(x, gy, gain, de)
    xmap, R, C, L = rowmap(x)
    gmap = _cotangent("dyn_dx", gy, x, (R, C, L))
    _expect(gain, (R, L), "dyn_dx: gain")
    _expect(de, (R, L), "dyn_dx: de")
    gx = torch.empty((R, C, L), dtype=torch.float32, device=x.device)
    pin = _Pin()
    check(lib().gfx_dyn_dx_f32(_ptr(x), xmap, _ptr(gy), gmap, pin(gain), pin(de),
                               _ptr(gx), R, C, L, _stream()), "gfx_dyn_dx_f32")
    return gx


@_on_device
def energy(x):
    _require_gpu(x)
    xmap, R, C, L = rowmap(x)
    e = torch.empty((R, L), dtype=torch.float32, device=x.device)
    check(lib().gfx_energy_f32(_ptr(x), xmap, _ptr(e), R, C, L, _stream()), "gfx_energy_f32")
    return e


@_on_device
def onepole(u, z_alpha, iir_len, Lout=None, relu=True):
    _require_gpu(u, z_alpha)
    u = u.contiguous()
    R, L = u.shape
    Lout = L if Lout is None else Lout
    out = torch.empty((R, Lout), dtype=torch.float32, device=u.device)
    pin = _Pin()
    check(lib().gfx_onepole_f32(_ptr(u), pin(_rowvec(z_alpha, R)), _ptr(out), R, L, Lout, iir_len, int(relu), _stream()), "gfx_onepole_f32")
    return out


@_on_device
def onepole_energy(x, z_alpha, iir_len, Lout=None, relu=True, rowmax=None):
    """onepole(energy(x), ...) in one pass over the signal x ((R, C, L) or a strided (B, n, C, L) view): gfx_onepole_energy_f32.
    ``rowmax``: a dict that receives ``rowmax["words"]``, the bits of max |out| of every row (for odd_alias(rowmax=))."""
    _require_gpu(x, z_alpha)
    xmap, R, C, L = rowmap(x)
    Lout = L if Lout is None else Lout
    out = torch.empty((R, Lout), dtype=torch.float32, device=x.device)
    words = torch.empty(R, dtype=torch.int32, device=x.device) if rowmax is not None else None
    pin = _Pin()
    check(lib().gfx_onepole_energy_f32(_ptr(x), xmap, C, pin(_rowvec(z_alpha, R)), _ptr(out), R, L, Lout, iir_len, int(relu),
                                       _ptr(words), _stream()), "gfx_onepole_energy_f32")
    if rowmax is not None:
        rowmax["words"] = words
    return out


@_on_device
def onepole_fir(z_alpha, iir_len):
    _require_gpu(z_alpha)
    R = z_alpha.numel()
    h = torch.empty((R, iir_len), dtype=torch.float32, device=z_alpha.device)
    pin = _Pin()
    check(lib().gfx_onepole_fir_f32(pin(z_alpha), _ptr(h), R, iir_len, _stream()), "gfx_onepole_fir_f32")
    return h


BALLISTICS_SCHEDULE = "chunks"   # "chunks": rows cut into verified chunks (gfx_ballistics_f32 with a workspace); "rows": whole rows only


@_on_device
def ballistics(u, z_alpha, coefficients=False, schedule=None, flags=None, zi=None, return_state=False):
    """Ballistics.forward (core/envelope.py:84-101) on (R, L) rows: the float32 sequential recursion, bit for bit, whichever
    schedule produces it.  ``coefficients``: ``z_alpha`` holds (at, rt) themselves instead of their logits.
    ``flags``: a list that receives the per-row int32 flags of the chunked schedule (1 = the row was walked whole by the
    last launch: its coefficient is too slow for a chunk, or a chunk boundary failed the bit check) -- diagnostics.
    ``zi`` (R,): y[-1] of every row instead of 1; ``return_state``: -> (y, zf), zf (R,) = y[:, L-1] -- handed to the next
    block as its ``zi``, the blocks are the one-call output in the same bits."""
    schedule = BALLISTICS_SCHEDULE if schedule is None else schedule
    if schedule not in ("chunks", "rows"):
        raise ValueError(f"ballistics: unknown schedule {schedule!r}")
    _require_gpu(u, z_alpha)
    u, z_alpha = u.contiguous(), z_alpha.contiguous()
    R, L = u.shape
    if z_alpha.shape != (R, 2):
        raise ValueError(f"z_alpha must be ({R}, 2), got {tuple(z_alpha.shape)}")
    y = torch.empty_like(u)
    pin = _Pin()
    # zeroed: the single-pass schedules (short rows, very many rows) never write the flags this buffer is returned as
    ws = pin.workspace(schedule == "chunks" and lib().gfx_ballistics_ws_bytes(R), u.device, zero=True)
    zi = _state(zi, (R,), "ballistics", "zi")
    zf = torch.empty(R, dtype=torch.float32, device=u.device) if return_state else None
    with _timed("ballistics_walk_kernel", 8 * R * L):
        check(lib().gfx_ballistics_f32(_ptr(u), _ptr(z_alpha), int(coefficients), _ptr(zi), _ptr(zf), _ptr(y), R, L, *ws,
                                       _stream()), "gfx_ballistics_f32")
    if flags is not None and schedule == "chunks":      # (no rows, no workspace: no flags either)
        flags.append(y.new_empty(0, dtype=torch.int32) if pin.ws is None else pin.ws.view(torch.int32))
    return (y, zf) if return_state else y


@_on_device
def dynamics_ballistics(x, log_threshold, log_ratio, log_knee, z_alpha, knee, gate, out=None, param_rows=None, schedule=None,
                        zi=None, return_state=False):
    """Compressor / NoiseGate with the ballistics energy smoother and no gain smoother in one pass over ``x`` ((R, C, L) or
    a strided (B, n, C, L) view): gfx_dynamics_ballistics_f32.  ``z_alpha``: (param_rows, 2).  ``zi`` (R,), one value per
    SIGNAL row: the envelope entering the block; ``return_state``: -> (out, zf), the envelope leaving it (the kernel never
    stores the envelope itself)."""
    schedule = BALLISTICS_SCHEDULE if schedule is None else schedule
    _require_gpu(x, out, z_alpha)
    xmap, R, C, L = rowmap(x)
    P = R if param_rows is None else param_rows
    z_alpha = z_alpha.contiguous()
    if z_alpha.shape != (P, 2):
        raise ValueError(f"z_alpha must be ({P}, 2), got {tuple(z_alpha.shape)}")
    zi = _state(zi, (R,), "dynamics_ballistics", "zi")
    # the chunked schedule writes every row in its first pass and re-reads x for the rows it has to walk again
    out, ymap = _output(out, (R, C, L), x.device, "dynamics_ballistics", apart=(x, zi))
    zf = torch.empty(R, dtype=torch.float32, device=x.device) if return_state else None
    pin = _Pin()
    with _timed("ballistics_walk_kernel", 8 * R * C * L):
        check(lib().gfx_dynamics_ballistics_f32(_ptr(x), xmap, _ptr(out), ymap, *_curve(pin, log_threshold, log_ratio, log_knee, P),
                                                _ptr(z_alpha), P, R, C, L, KNEES[knee], int(gate), _ptr(zi), _ptr(zf),
                                                *pin.workspace(schedule == "chunks" and lib().gfx_ballistics_ws_bytes(R), x.device),
                                                _stream()), "gfx_dynamics_ballistics_f32")
    return (out, zf) if return_state else out


@_on_device
def ballistics_energy(x, z_alpha, coefficients=False, schedule=None, zi=None, return_state=False):
    """ballistics(mean_c x^2) in one pass over x ((R, C, L) or a strided (B, n, C, L) view) -> (R, L): the envelope of
    Compressor / NoiseGate with energy_smoother="ballistics" (dynamics.py:390, core/envelope.py:84-101).  ``zi`` /
    ``return_state``: as :func:`ballistics`."""
    schedule = BALLISTICS_SCHEDULE if schedule is None else schedule
    _require_gpu(x, z_alpha)
    xmap, R, C, L = rowmap(x)
    z_alpha = z_alpha.contiguous()
    if z_alpha.shape != (R, 2):
        raise ValueError(f"z_alpha must be ({R}, 2), got {tuple(z_alpha.shape)}")
    env = torch.empty((R, L), dtype=torch.float32, device=x.device)
    zi = _state(zi, (R,), "ballistics_energy", "zi")
    zf = torch.empty(R, dtype=torch.float32, device=x.device) if return_state else None
    pin = _Pin()
    with _timed("ballistics_walk_kernel", 4 * R * (C + 1) * L):
        check(lib().gfx_ballistics_energy_f32(_ptr(x), xmap, C, _ptr(z_alpha), int(coefficients), _ptr(zi), _ptr(zf), _ptr(env),
                                              R, L, *pin.workspace(schedule == "chunks" and lib().gfx_ballistics_ws_bytes(R), x.device),
                                              _stream()), "gfx_ballistics_energy_f32")
    return (env, zf) if return_state else env


@_on_device
def ballistics_bwd(x, y, g, z_alpha, schedule="chunks", zi=None):
    """Adjoint of :func:`ballistics`: -> (dL/dx (R,L), dL/dz_alpha (R,2)).  ``schedule``: "chunks" (rows cut into chunks
    with a 2048-sample warm-up, gfx_ballistics_bwd_f32 with a workspace) or "rows" (every row walked whole by one lane).
    ``zi`` (R,): the state the forward entered with; -> (gx, gz, dL/dzi (R,)).  A cotangent of the final state
    is a cotangent of y[:, L-1]: add it to ``g`` there."""
    _require_gpu(x, y, g, z_alpha)
    x, y, g, z_alpha = x.contiguous(), y.contiguous(), g.contiguous(), z_alpha.contiguous()
    R, L = x.shape
    _expect(y, (R, L), "ballistics_bwd: y")
    _expect(g, (R, L), "ballistics_bwd: g")
    _expect(z_alpha, (R, 2), "ballistics_bwd: z_alpha")
    gx, gz = torch.empty_like(x), torch.empty((R, 2), dtype=torch.float32, device=x.device)
    zi = _state(zi, (R,), "ballistics_bwd", "zi")
    gzi = None if zi is None else torch.empty(R, dtype=torch.float32, device=x.device)
    pin = _Pin()
    check(lib().gfx_ballistics_bwd_f32(_ptr(x), _ptr(y), _ptr(g), _ptr(z_alpha), _ptr(zi), _ptr(gx), _ptr(gz), _ptr(gzi), R, L,
                                       *pin.workspace(schedule != "rows" and max(int(lib().gfx_ballistics_bwd_ws_bytes(R, L)), 4),
                                                      x.device), _stream()), "gfx_ballistics_bwd_f32")
    return (gx, gz) if zi is None else (gx, gz, gzi)


@_on_device
def dyn_gain(env, log_threshold, log_ratio, log_knee, knee, gate, log_out):
    _require_gpu(env)
    env = env.contiguous()
    R, L = env.shape
    g = torch.empty_like(env)
    pin = _Pin()
    check(
        lib().gfx_dyn_gain_f32(_ptr(env), _ptr(g), *_curve(pin, log_threshold, log_ratio, log_knee, R), R, L, KNEES[knee],
                               int(gate), int(log_out), _stream()),
        "gfx_dyn_gain_f32",
    )
    return g


@_on_device
def apply_gain(x, g, exp_gain=False, out=None):
    _require_gpu(x, g, out)
    xmap, R, C, L = rowmap(x)
    _expect(g, (R, L), "apply_gain: gain")
    out, ymap = _output(out, (R, C, L), x.device, "apply_gain", apart=(x, g))
    g = g.contiguous()
    check(lib().gfx_apply_gain_f32(_ptr(x), xmap, _ptr(g), _ptr(out), ymap, R, C, L, int(exp_gain), _stream()), "gfx_apply_gain_f32")
    return out


@_on_device
def dyn_gain_apply(x, env, log_threshold, log_ratio, log_knee, knee, gate, out=None, param_rows=None):
    """y = exp(g(log(env + 1e-5)))[:, None, :] * x in one pass (dynamics.py:394-405): ``env`` (R, L) is the smoothed energy,
    ``x`` / ``out`` (R, C, L) tensors or strided (B, n, C, L) views."""
    _require_gpu(x, env, out)
    xmap, R, C, L = rowmap(x)
    _expect(env, (R, L), "dyn_gain_apply: envelope")
    out, ymap = _output(out, (R, C, L), x.device, "dyn_gain_apply", apart=(x, env))
    env = env.contiguous()
    P = R if param_rows is None else param_rows
    pin = _Pin()
    with _timed("dyn_gain_apply_kernel", 4 * R * L * (2 * C + 1)):
        check(lib().gfx_dyn_gain_apply_f32(_ptr(x), xmap, _ptr(env), _ptr(out), ymap, *_curve(pin, log_threshold, log_ratio, log_knee, P),
                                           P, R, C, L, KNEES[knee], int(gate), _stream()), "gfx_dyn_gain_apply_f32")
    return out


@_on_device
def stereo_gain(x, log_gain, out=None, mix=None):
    """``mix``: as in :func:`dynamics_fused` -- the routing sum behind a strided (B, n, C, L) stage, produced by the same
    kernel (gfx_stereo_gain_mix_f32); sets ``mix["done"]`` when it was."""
    _require_gpu(x, log_gain, out)
    xmap, R, C, L = rowmap(x)
    _expect(log_gain, (R, 2), "stereo_gain: log_gain")
    # (mix["out"] is outside the rule, as in dynamics_fused: device-held sources, kept apart by the render's planner)
    out, ymap = _output(out, (R, 2, L), x.device, "stereo_gain", apart=(x,))
    pin = _Pin()
    if mix is not None and MIX_FUSION and x.ndim == 4 and out.ndim == 4:
        n = x.shape[1]
        m = _read_mix(mix, x.shape[0], n, 2, L)
        if m is not None:
            rc = lib().gfx_stereo_gain_mix_f32(_ptr(x), xmap, pin(log_gain), _ptr(out), ymap, R, C, L, *_mix_args(m, n), _stream())
            if rc == 0:
                mix["done"] = True
                return out
            if rc != GFX_EINVAL:
                check(rc, "gfx_stereo_gain_mix_f32")
    check(lib().gfx_stereo_gain_f32(_ptr(x), xmap, pin(log_gain), _ptr(out), ymap, R, C, L, _stream()), "gfx_stereo_gain_f32")
    return out


@_on_device
def biquad_cascade(x, Bs, As, ssm_quirk=False, out=None, zi=None, return_state=False):
    """Exact time-domain cascade of the K biquads in Bs/As (R,Cf,K,3) over x (R,C,L) or a (B,n,C,L) view.

    ``zi``: the filter state entering sample 0, contiguous float32 (R, Cout, K, 2) with Cout = max(C, Cf): per row-channel
    and section (w[-1], w[-2]) of the a0-normalised direct-form-II recursion (None: silence).  With ``zi`` or
    ``return_state`` the result is ``(y, zf)``, zf = (w[L-1], w[L-2]) in the same layout (a new tensor): feed it to the next
    block's call and the blocks' outputs are the one-call output of the whole signal."""
    _require_gpu(x, Bs, As, out)
    xmap, R, Cin, L = rowmap(x)
    Rb, Cf, K, three = Bs.shape
    if Rb != R or three != 3 or As.shape != Bs.shape:
        raise ValueError(f"coefficients {tuple(Bs.shape)} / {tuple(As.shape)} do not match {R} rows")
    Cout = max(Cin, Cf)
    zi = _state(zi, (R, Cout, K, 2), "biquad_cascade", "zi")
    out, ymap = _output(out, (R, Cout, L), x.device, "biquad_cascade", apart=(x, zi))
    Bs, As = Bs.contiguous(), As.contiguous()
    if zi is None and not return_state:
        with _timed("biquad_cascade_kernel", 4 * R * (Cin + Cout) * L):
            check(lib().gfx_biquad_cascade_f32(_ptr(x), xmap, _ptr(out), ymap, _ptr(Bs), _ptr(As), R, Cin, Cf, K, L,
                                               int(ssm_quirk), _stream()), "gfx_biquad_cascade_f32")
        return out
    zf = torch.empty((R, Cout, K, 2), dtype=torch.float32, device=x.device)
    with _timed("biquad_cascade_state_kernel", 4 * R * (Cin + Cout) * L + 16 * R * Cout * K):
        check(lib().gfx_biquad_cascade_state_f32(_ptr(x), xmap, _ptr(out), ymap, _ptr(Bs), _ptr(As), _ptr(zi), _ptr(zf),
                                                 R, Cin, Cf, K, L, int(ssm_quirk), _stream()), "gfx_biquad_cascade_state_f32")
    return out, zf


BIQUAD_GRADS = ("x", "Bs", "As", "zi")


def biquad_cascade_bwd_ws_bytes(R, C_out, K, L):
    """Bytes of workspace one gfx_biquad_cascade_bwd_f32 call needs (no GPU involved): every section's entering state per
    pair of row-channels and 512-sample tile."""
    return lib().gfx_biquad_cascade_bwd_ws_bytes(R, C_out, K, L)


@_on_device
def biquad_cascade_bwd(x, gy, Bs, As, zi=None, gzf=None, want=BIQUAD_GRADS, out=None, ws=None):
    """Backward of :func:`biquad_cascade` (``ssm_quirk=False``) in one call (gfx_biquad_cascade_bwd_f32) -> (gx, gB, gA, gzi),
    None for what ``want`` (any of BIQUAD_GRADS) leaves out.  Nothing of the forward is needed but its arguments.

    ``x``, ``gy``: the forward's input (R,C,L) and dL/dy (R,Cout,L), or strided (B,n,.,L) views; ``zi``: the state the
    forward started from (None: silence); ``gzf``: dL/dzf (R,Cout,K,2) of a stateful forward (None: zero).  ``gx`` is
    ``out`` (any view of x's shape) or a new (R,C,L) tensor, gB / gA (R,Cf,K,3), gzi (R,Cout,K,2).  ``ws``: a uint8
    workspace of at least ``biquad_cascade_bwd_ws_bytes(R, Cout, K, L)`` bytes to reuse.  What the call writes (``out``,
    ``ws``) may share memory with nothing it reads.  Channel broadcasts (1 <-> C) are summed inside the kernel for
    C <= 2; with more channels the broadcast side is passed expanded and the channels of the result are added by torch
    (a (R,C,L) temporary for gx when C_in = 1)."""
    what = "biquad_cascade_bwd"
    _require_gpu(x, gy, Bs, As, zi, gzf, out)
    xmap, R, Cin, L = rowmap(x)
    Rb, Cf, K, three = Bs.shape
    if Rb != R or three != 3 or As.shape != Bs.shape:
        raise ValueError(f"{what}: coefficients {tuple(Bs.shape)} / {tuple(As.shape)} do not match {R} rows")
    Cout = max(Cin, Cf)
    gmap, Rg, Cg, Lg = rowmap(gy)
    if (Rg, Cg, Lg) != (R, Cout, L):
        raise ValueError(f"{what}: gradient {tuple(gy.shape)} does not match rows={R}, channels={Cout}, length={L}")
    unknown = set(want) - set(BIQUAD_GRADS)
    if unknown or not want:
        raise ValueError(f"{what}: want {tuple(want)} must name some of {BIQUAD_GRADS}")
    zi = _state(zi, (R, Cout, K, 2), what, "zi")
    gzf = _state(gzf, (R, Cout, K, 2), what, "gzf")
    reads = (x, gy, Bs, As, zi, gzf)
    gx, gxmap = _signal_grad(what, want, out, (R, Cin, L), xmap, x.device, (*reads, ws))
    # More than two channels with a broadcast side: the kernel sums a broadcast inside a pair of row-channels, which is a
    # row's channels only when there are two.  The broadcast side goes in expanded instead -- the coefficients copied
    # (parameter-sized), x through a row map with a zero channel stride -- and the channels of the result are added here.
    wide_f = Cout > 2 and Cf == 1 and ("Bs" in want or "As" in want)
    wide_x = Cout > 2 and Cin == 1 and gx is not None
    kx, kxmap, kgx, kgxmap, kCin, kCf = x, xmap, gx, gxmap, Cin, Cf
    if wide_f:
        Bs, As, kCf = Bs.expand(R, Cout, K, 3), As.expand(R, Cout, K, 3), Cout
    if wide_x:
        kx = x.expand(*x.shape[:-2], Cout, L)
        kgx = torch.empty((R, Cout, L), dtype=torch.float32, device=x.device)
        kxmap, kgxmap, kCin = rowmap(kx)[0], rowmap(kgx)[0], Cout
    Bs, As = Bs.contiguous(), As.contiguous()
    gB = torch.empty_like(Bs) if "Bs" in want else None
    gA = torch.empty_like(As) if "As" in want else None
    gzi = torch.empty((R, Cout, K, 2), dtype=torch.float32, device=x.device) if "zi" in want else None
    pin = _Pin()
    wsarg = _workspace(what, ws, lib().gfx_biquad_cascade_bwd_ws_bytes(R, Cout, K, L), x.device, pin, reads)
    # x twice (both passes), g once, gx once
    with _timed("biquad_cascade_bwd_kernel", 4 * R * L * (2 * Cin + Cout + (kCin if gx is not None else 0))):
        check(lib().gfx_biquad_cascade_bwd_f32(_ptr(kx), kxmap, _ptr(gy), gmap, _ptr(kgx), kgxmap, _ptr(Bs), _ptr(As), _ptr(zi),
                                               _ptr(gzf), _ptr(gB), _ptr(gA), _ptr(gzi), *wsarg, R, kCin, kCf, K, L, _stream()),
              "gfx_biquad_cascade_bwd_f32")
    if wide_f:
        gB, gA = (None if t is None else t.sum(1, keepdim=True) for t in (gB, gA))
    if wide_x:
        gx.copy_(kgx.view(*gx.shape[:-2], Cout, L).sum(-2, keepdim=True))
    return gx, gB, gA, gzi


@_on_device
def noise_shaping_ir(noise, log_decay, log_gain, log_fade_in, z_fade_in_gain, ir_len, min_decay, max_decay):
    """noise (C,K,>=ir_len) view with unit last stride; parameters (R,C,K) -> ir (R,C,ir_len), un-normalised."""
    _require_gpu(noise, log_decay, log_gain, log_fade_in, z_fade_in_gain)
    R, C, K = log_decay.shape
    if noise.shape[:2] != (C, K) or noise.stride(-1) != 1 or noise.stride(1) != noise.stride(0) // K:
        raise ValueError("noise must be a (C, K, T) view of a contiguous band-split noise buffer")
    pin = _Pin()
    ir = torch.empty((R, C, ir_len), dtype=torch.float32, device=log_decay.device)
    check(
        lib().gfx_noise_shaping_ir_f32(_ptr(noise), noise.stride(1), pin(log_decay), pin(log_gain), pin(log_fade_in),
                                       pin(z_fade_in_gain), _ptr(ir), R, C, K, ir_len, float(min_decay), float(max_decay), _stream()),
        "gfx_noise_shaping_ir_f32",
    )
    return ir


NS_GRADS = ("log_decay", "log_gain", "log_fade_in", "z_fade_in_gain")
NS_BWD_ROWS = 1 << 16      # rows per gfx_noise_shaping_ir_bwd_f32 call: bounds the workspace of a call without one


def noise_shaping_ir_bwd_ws_bytes(R, C, K, ir_len):
    """Bytes of workspace one gfx_noise_shaping_ir_bwd_f32 call over R rows needs (no GPU involved)."""
    return lib().gfx_noise_shaping_ir_bwd_ws_bytes(R, C, K, ir_len)


@_on_device
def noise_shaping_ir_bwd(grad_ir, noise, log_decay, log_gain, log_fade_in, z_fade_in_gain, min_decay, max_decay, ir=None,
                         row_gain=None, want=NS_GRADS, ws=None):
    """Backward of :func:`noise_shaping_ir` (gfx_noise_shaping_ir_bwd_f32) -> {name: (R,C,K) gradient} for the names of
    ``want`` (any of NS_GRADS; a fade parameter that was not given is skipped).

    ``grad_ir``: dL/dh (R,C,ir_len).  With ``ir`` (the forward's output) and ``row_gain`` (R values, 1 / sqrt(mean_c sum_t
    ir^2 + 1e-12)) h = row_gain * ir, the normalised taps; without them h = ir.  ``noise`` must be the (C,K,>=ir_len) view
    the forward was given.  ``ws``: a uint8 workspace of at least ``noise_shaping_ir_bwd_ws_bytes(min(R, NS_BWD_ROWS), C,
    K, ir_len)`` bytes to reuse; it may share memory with none of the inputs."""
    what = "noise_shaping_ir_bwd"
    _require_gpu(grad_ir, noise, log_decay, log_gain, log_fade_in, z_fade_in_gain, ir, row_gain)
    R, C, K = log_decay.shape
    if grad_ir.ndim != 3 or tuple(grad_ir.shape[:2]) != (R, C):
        raise ValueError(f"{what}: gradient {tuple(grad_ir.shape)} does not match the parameters {tuple(log_decay.shape)}")
    ir_len = grad_ir.shape[2]
    if (noise.shape[:2] != (C, K) or noise.stride(-1) != 1 or noise.stride(1) != noise.stride(0) // K
            or noise.shape[2] < ir_len):
        raise ValueError("noise must be a (C, K, T) view of a contiguous band-split noise buffer")
    if (ir is None) != (row_gain is None):
        raise ValueError(f"{what}: ir and row_gain come together (the normalised taps) or not at all")
    if (log_fade_in is None) != (z_fade_in_gain is None):
        raise ValueError(f"{what}: log_fade_in and z_fade_in_gain come together or not at all")
    given = {"log_decay": log_decay, "log_gain": log_gain, "log_fade_in": log_fade_in, "z_fade_in_gain": z_fade_in_gain}
    for name, t in given.items():
        _expect(t, (R, C, K), f"{what}: {name}")
    _expect(ir, (R, C, ir_len), f"{what}: ir")
    _want(what, want, NS_GRADS)
    names = [k for k in NS_GRADS if k in want and given[k] is not None]
    if not names:
        raise ValueError(f"{what}: no gradient asked for ({tuple(want)})")
    if K > 64:
        raise ValueError(f"{what}: at most 64 bands, got {K}")
    if row_gain is not None:
        if row_gain.numel() != R:
            raise ValueError(f"{what}: {row_gain.numel()} gains for {R} rows")
        row_gain = row_gain.reshape(R).contiguous()
    reads = (grad_ir, noise, *given.values(), ir, row_gain)
    grad_ir = grad_ir.contiguous()
    ir = None if ir is None else ir.contiguous()
    given = {k: None if t is None else t.contiguous() for k, t in given.items()}
    grads = {k: torch.empty((R, C, K), dtype=torch.float32, device=grad_ir.device) for k in names}
    cut = lambda t, r0, n: None if t is None else t[r0:r0 + n]  # noqa: E731
    pin = _Pin()
    wsarg = _workspace(what, ws, lib().gfx_noise_shaping_ir_bwd_ws_bytes(min(R, NS_BWD_ROWS), C, K, ir_len), grad_ir.device,
                       pin, reads)
    with _timed("noise_shaping_ir_bwd_kernel", 4 * R * C * ir_len * (1 if ir is None else 2)):
        for r0, n in _row_chunks(R, NS_BWD_ROWS):
            check(
                lib().gfx_noise_shaping_ir_bwd_f32(_ptr(grad_ir[r0:r0 + n]), _ptr(cut(ir, r0, n)), _ptr(cut(row_gain, r0, n)),
                                                   _ptr(noise), noise.stride(1), *(_ptr(cut(t, r0, n)) for t in given.values()),
                                                   *(_ptr(cut(grads.get(k), r0, n)) for k in NS_GRADS), n, C, K, ir_len,
                                                   float(min_decay), float(max_decay), *wsarg, _stream()),
                "gfx_noise_shaping_ir_bwd_f32",
            )
    return grads


# ----------------------------------------------------------------------------------------- waveshapers
WS_TANH, WS_PIECEWISE, WS_POWER, WS_CHEBYSHEV = 0, 1, 2, 3


@_on_device
def row_mean(x):
    """Mean over time of every row-channel: (R,C,L) or (B,n,C,L) view -> (R*C,)."""
    _require_gpu(x)
    xmap, R, C, L = rowmap(x)
    mean = torch.empty(R * C, dtype=torch.float32, device=x.device)
    check(lib().gfx_row_mean_f32(_ptr(x), xmap, _ptr(mean), R, C, L, _stream()), "gfx_row_mean_f32")
    return mean


WS_GRADS = ("x", "log_pre_gain", "log_post_gain", "p0", "p1")


def _waveshaper_args(what, x, R, C, mode, log_pre_gain, log_post_gain, p0, p1, remove_dc, dc):
    """What the waveshaper pair reads besides the signal -> ({name: contiguous (R, n) view or None} in WS_GRADS' order, K =
    number of basis weights of the polynomial modes, dc = the (R * C,) row-channel means to subtract or None)."""
    params = {"log_pre_gain": log_pre_gain, "log_post_gain": log_post_gain, "p0": p0, "p1": p1}
    params = {k: None if t is None else t.contiguous().view(R, -1) for k, t in params.items()}
    K = params["p0"].shape[1] if (params["p0"] is not None and mode in (WS_POWER, WS_CHEBYSHEV)) else 0
    if not remove_dc:
        dc = None
    elif dc is None:
        dc = row_mean(x)
    else:
        _expect(dc, (R * C,), f"{what}: dc")
        dc = dc.contiguous()
    return params, K, dc


def _shape(what, x, mode, log_pre_gain, log_post_gain, p0, p1, use_tanh, inverse_post_gain, remove_dc, out, dc, return_dc,
           oversampling=None):
    """The body of :func:`waveshaper` and, with ``oversampling`` = (factor, h_up, offset_up, h_dn, offset_dn), of
    :func:`oversampled_waveshaper`."""
    _require_gpu(x, log_pre_gain, log_post_gain, p0, p1, out, dc)
    entry, kernel, taps, extra = "gfx_waveshaper_f32", "waveshaper_kernel", (), lambda pin: ()
    if oversampling is not None:
        entry, kernel = "gfx_oversampled_waveshaper_f32", "oversampled_waveshaper_kernel"
        taps, extra = _oversampling_args(what, *oversampling)
    xmap, R, C, L = rowmap(x)
    out, ymap = _output(out, (R, C, L), x.device, what, apart=(x, dc, *taps))
    params, K, dc = _waveshaper_args(what, x, R, C, mode, log_pre_gain, log_post_gain, p0, p1, remove_dc, dc)
    pin = _Pin()
    with _timed(kernel, 8 * R * C * L):
        check(
            getattr(lib(), entry)(_ptr(x), xmap, _ptr(out), ymap, R, C, L, *extra(pin), mode, int(use_tanh),
                                  int(inverse_post_gain), *(_ptr(v) for v in params.values()), K, _ptr(dc), _stream()),
            entry,
        )
    return (out, dc) if return_dc else out


def _shape_bwd(what, x, gy, mode, log_pre_gain, log_post_gain, p0, p1, use_tanh, inverse_post_gain, remove_dc, dc, out, want,
               oversampling=None):
    """The body of :func:`waveshaper_bwd` and, with ``oversampling`` as for :func:`_shape`, of
    :func:`oversampled_waveshaper_bwd`."""
    _require_gpu(x, gy, log_pre_gain, log_post_gain, p0, p1, out, dc)
    entry, sized, kernel = "gfx_waveshaper_bwd_f32", "gfx_waveshaper_bwd_ws_bytes", "waveshaper_bwd_kernel"
    factor, taps, extra = (), (), lambda pin: ()
    if oversampling is not None:
        entry, sized = "gfx_oversampled_waveshaper_bwd_f32", "gfx_oversampled_waveshaper_bwd_ws_bytes"
        kernel, factor = "oversampled_waveshaper_bwd_kernel", oversampling[:1]
        taps, extra = _oversampling_args(what, *oversampling)
    xmap, R, C, L = rowmap(x)
    gmap = _cotangent(what, gy, x, (R, C, L))
    _want(what, want, WS_GRADS)
    gx, gxmap = _signal_grad(what, want, out, (R, C, L), xmap, x.device, (x, gy, dc, *taps))
    params, K, dc = _waveshaper_args(what, x, R, C, mode, log_pre_gain, log_post_gain, p0, p1, remove_dc, dc)
    grads = {k: torch.empty_like(v) for k, v in params.items() if k in want and v is not None}
    pin = _Pin()
    ws = pin.workspace((bool(grads) or (gx is not None and dc is not None))
                       and getattr(lib(), sized)(R, C, L, K, *factor), x.device)
    with _timed(kernel, (8 if gx is None else 12) * R * C * L):
        check(
            getattr(lib(), entry)(_ptr(x), xmap, _ptr(gy), gmap, R, C, L, *extra(pin), mode, int(use_tanh),
                                  int(inverse_post_gain), *(_ptr(v) for v in params.values()), K, _ptr(dc), _ptr(gx), gxmap,
                                  *(_ptr(grads.get(k)) for k in params), *ws, _stream()),
            entry,
        )
    return gx, grads


@_on_device
def waveshaper(x, mode, log_pre_gain=None, log_post_gain=None, p0=None, p1=None, use_tanh=False,
               inverse_post_gain=False, remove_dc=False, out=None, dc=None, return_dc=False):
    """Memoryless distortion of every row (see gfx_waveshaper_f32 in the header for the modes).
    ``dc``: the row-channel means of x when the caller already has them (``remove_dc``); ``return_dc``: -> (out, dc), the
    means this call subtracted (None without ``remove_dc``) -- what waveshaper_bwd needs of them."""
    return _shape("waveshaper", x, mode, log_pre_gain, log_post_gain, p0, p1, use_tanh, inverse_post_gain, remove_dc, out, dc,
                  return_dc)


@_on_device
def waveshaper_bwd(x, gy, mode, log_pre_gain=None, log_post_gain=None, p0=None, p1=None, use_tanh=False,
                   inverse_post_gain=False, remove_dc=False, dc=None, out=None, want=WS_GRADS):
    """Backward of :func:`waveshaper` in one streaming pass (gfx_waveshaper_bwd_f32) -> (gx, grads).

    ``x``, ``gy``: (R,C,L) or strided (B,n,C,L) views; ``want``: which of WS_GRADS to compute (a parameter that was not
    given is skipped).  ``gx`` is None unless "x" is wanted, else ``out`` (any view of the signal's shape, apart from x, gy
    and dc) or a new (R,C,L) tensor.  ``grads``: {name: (R, n) gradient} of the wanted parameters.
    ``dc``: the means the forward subtracted (``waveshaper(..., return_dc=True)``); recomputed when missing."""
    return _shape_bwd("waveshaper_bwd", x, gy, mode, log_pre_gain, log_post_gain, p0, p1, use_tanh, inverse_post_gain,
                      remove_dc, dc, out, want)


# ----------------------------------------------------------------------------------------- oversampled waveshapers
OVERSAMPLE_MAX_FACTOR = 16
OVERSAMPLE_MAX_TAPS = 1024


def oversampled_waveshaper_tile(factor):
    """Base-rate samples of a row-channel that one workgroup of the oversampled kernels produces (os_tile in
    csrc/oversampled.hip): about 4096 / factor, a multiple of 64."""
    _int_in("oversampled_waveshaper_tile", "factor", factor, 1, OVERSAMPLE_MAX_FACTOR)
    return 4096 // factor // 64 * 64


def _oversampling_args(what, factor, h_up, offset_up, h_dn, offset_dn):
    """The factor, the two filters and their offsets, checked before anything is allocated -> (the taps, what the oversampled
    entries take between L and the mode as a function of the launch's ``pin``)."""
    oversampled_waveshaper_tile(factor)
    for name, h, offset_name, offset in (("h_up", h_up, "offset_up", offset_up), ("h_dn", h_dn, "offset_dn", offset_dn)):
        _taps(what, name, h, OVERSAMPLE_MAX_TAPS)
        _int_in(what, offset_name, offset, 0, h.numel() - 1)
    return (h_up, h_dn), lambda pin: (factor, pin(h_up), h_up.numel(), offset_up, pin(h_dn), h_dn.numel(), offset_dn)


@_on_device
def oversampled_waveshaper(x, mode, factor, h_up, offset_up, h_dn, offset_dn, log_pre_gain=None, log_post_gain=None, p0=None,
                           p1=None, use_tanh=False, inverse_post_gain=False, remove_dc=False, out=None, dc=None,
                           return_dc=False):
    """:func:`waveshaper` at ``factor`` times the rate in one fused pass (gfx_oversampled_waveshaper_f32): x minus its mean is
    interpolated by ``h_up`` (u[p] = sum_k xc[k] h_up[p + offset_up - k factor]), shaped, zero outside [0, factor L), and
    decimated by ``h_dn`` (y[m] = sum_p v[p] h_dn[m factor + offset_dn - p]); the high-rate signals never reach memory.
    ``h_up``, ``h_dn``: 1..1024 float32 taps on the GPU each, shared by every row; ``factor`` in 1..16.  Everything else as
    :func:`waveshaper`, except that ``out`` may never share memory with ``x``: tiles read each other's halos.  Equal bits
    from call to call; a row's result does not depend on the other rows."""
    return _shape("oversampled_waveshaper", x, mode, log_pre_gain, log_post_gain, p0, p1, use_tanh, inverse_post_gain,
                  remove_dc, out, dc, return_dc, oversampling=(factor, h_up, offset_up, h_dn, offset_dn))


@_on_device
def oversampled_waveshaper_bwd(x, gy, mode, factor, h_up, offset_up, h_dn, offset_dn, log_pre_gain=None, log_post_gain=None,
                               p0=None, p1=None, use_tanh=False, inverse_post_gain=False, remove_dc=False, dc=None, out=None,
                               want=WS_GRADS):
    """Backward of :func:`oversampled_waveshaper` in one fused pass (gfx_oversampled_waveshaper_bwd_f32) -> (gx, grads), with
    the arguments and results of :func:`waveshaper_bwd`; the taps get no gradient."""
    return _shape_bwd("oversampled_waveshaper_bwd", x, gy, mode, log_pre_gain, log_post_gain, p0, p1, use_tanh,
                      inverse_post_gain, remove_dc, dc, out, want, oversampling=(factor, h_up, offset_up, h_dn, offset_dn))


# ----------------------------------------------------------------------------------------- look-ahead limiter
LIMITER_MAX_TAPS = 1024
LIMITER_MAX_WINDOW = 4096
LIMITER_GRADS = ("x", "log_ceiling")


def limiter_tile(window):
    """Samples of a row that one workgroup of the limiter kernels produces (lim_tile in csrc/limiter.hip) for a window of
    ``window`` = lookahead + 1 + hold samples: 4096 up to a window of 2795, falling to 1024 at 4096 (the backward tile
    holds the peaks of tile + 2 window samples in LDS)."""
    _int_in("limiter_tile", "window", window, 1, LIMITER_MAX_WINDOW)
    return min(4096, max(1024, (155000 - 32 * window) // 16 // 512 * 512))


def _limiter_args(what, x, log_ceiling, h, lookahead, hold, compensate):
    """The configuration of the limiter pair, checked before anything is allocated -> (the signal's row map, R, C, L, the
    (R,) ceilings, sigma, the samples a state carries)."""
    _int_in(what, "lookahead", lookahead, 0, LIMITER_MAX_WINDOW - 1)
    _int_in(what, "hold", hold, 0, LIMITER_MAX_WINDOW - 1 - lookahead)
    _taps(what, "h", h, min(LIMITER_MAX_TAPS, lookahead + 1))
    xmap, R, C, L = rowmap(x)
    if log_ceiling.numel() != R:
        raise ValueError(f"{what}: {log_ceiling.numel()} ceilings for {R} rows")
    return xmap, R, C, L, log_ceiling.reshape(R), lookahead if compensate else 0, lookahead + hold + h.numel() - 1


@_on_device
def limiter(x, log_ceiling, h, lookahead, hold=0, compensate=False, out=None, state=None, return_state=False,
            return_gain=False):
    """Look-ahead peak limiter in one fused pass (gfx_limiter_f32): with T = exp(log_ceiling) per row, D = ``lookahead``,
    M = D + 1 + ``hold`` and the N <= D + 1 smoothing taps ``h`` (float32 on the GPU, shared by every row, non-negative
    and summing to one), p[k] = max_c |x[c,k]|, pk[q] = the largest of p[q-M+1 .. q], m[q] = T / pk[q] where pk[q] > T,
    else 1, s[n] = sum_j h[j] m[n-j], and y[c,n] = x[c,n-D] s[n] -- or, with ``compensate``, y[c,n] = x[c,n] s[n+D], the
    output aligned with the input and x taken as zero beyond its end.  |y| <= T up to rounding.

    ``x`` / ``out``: (R,C,L) tensors or strided (B,n,C,L) views; ``out`` may never share memory with ``x``.  ``state``: the
    last M + N - 2 input samples, contiguous (R, C, M + N - 2), oldest first (None: silence); with ``state`` or
    ``return_state`` the new state comes back too, and blocks cut anywhere give the bits of the one-call output (not with
    ``compensate``, whose output needs samples the next block brings).  ``return_gain``: also the applied gain, (R, L).
    -> y, or (y, [state], [gain]).  Equal bits from call to call; a row's result does not depend on the other rows."""
    what = "limiter"
    _require_gpu(x, log_ceiling, out)
    xmap, R, C, L, log_ceiling, sigma, S = _limiter_args(what, x, log_ceiling, h, lookahead, hold, compensate)
    stateful = state is not None or return_state
    if stateful and compensate:
        raise ValueError(f"{what}: compensate=True needs samples the next block brings; a state goes with compensate=False")
    zi = _state(state, (R, C, S), what, "state")
    out, ymap = _output(out, (R, C, L), x.device, what, apart=(x, zi, h))
    zf = torch.empty((R, C, S), dtype=torch.float32, device=x.device) if stateful else None
    gain = torch.empty((R, L), dtype=torch.float32, device=x.device) if return_gain else None
    pin = _Pin()
    with _timed("limiter_kernel", 8 * R * C * L):
        check(lib().gfx_limiter_f32(_ptr(x), xmap, _ptr(out), ymap, R, C, L, pin(log_ceiling), pin(h), h.numel(), lookahead, hold,
                                    sigma, _ptr(zi), _ptr(zf), _ptr(gain), _stream()), "gfx_limiter_f32")
    extra = (*((zf,) if stateful else ()), *((gain,) if return_gain else ()))
    return (out, *extra) if extra else out


@_on_device
def limiter_bwd(x, gy, log_ceiling, h, lookahead, hold=0, compensate=False, out=None, want=LIMITER_GRADS, ws=None):
    """Backward of :func:`limiter` (a call without a state) in one fused pass (gfx_limiter_bwd_f32) -> (gx, g_log_ceiling),
    None for what ``want`` (any of LIMITER_GRADS) leaves out.  Nothing of the forward is needed but its arguments.

    ``x``, ``gy``: (R,C,L) or strided (B,n,C,L) views; ``gx`` is ``out`` (any view of the signal's shape, apart from x and
    gy) or a new (R,C,L) tensor, g_log_ceiling (R,).  The gradient of a window's maximum goes to its earliest sample, in
    the lowest channel that holds the peak.  ``ws``: a uint8 workspace of at least gfx_limiter_bwd_ws_bytes(R, L,
    lookahead, hold) bytes to reuse, 8-byte aligned.  The taps get no gradient.  Equal bits from call to call."""
    what = "limiter_bwd"
    _require_gpu(x, gy, log_ceiling, out)
    xmap, R, C, L, log_ceiling, sigma, _ = _limiter_args(what, x, log_ceiling, h, lookahead, hold, compensate)
    gmap = _cotangent(what, gy, x, (R, C, L))
    _want(what, want, LIMITER_GRADS, some=True)
    reads = (x, gy, h)
    gx, gxmap = _signal_grad(what, want, out, (R, C, L), xmap, x.device, (*reads, ws))
    gc = torch.empty(R, dtype=torch.float32, device=x.device) if "log_ceiling" in want else None
    pin = _Pin()
    wsarg = (0, 0)
    if gc is not None:
        wsarg = _workspace(what, ws, lib().gfx_limiter_bwd_ws_bytes(R, L, lookahead, hold), x.device, pin, reads, align=8)
    with _timed("limiter_bwd_kernel", (8 if gx is None else 12) * R * C * L):
        check(lib().gfx_limiter_bwd_f32(_ptr(x), xmap, _ptr(gy), gmap, R, C, L, pin(log_ceiling), pin(h), h.numel(), lookahead,
                                        hold, sigma, _ptr(gx), gxmap, _ptr(gc), *wsarg, _stream()), "gfx_limiter_bwd_f32")
    return gx, gc


# ----------------------------------------------------------------------------------------- modulated delay line
MODDELAY_MAX_DELAY = 8192
MODDELAY_MAX_VOICES = 8
MODDELAY_GRADS = ("x", "delay", "depth", "rate", "phase", "gain", "dry")
_MODDELAY_INTERP = {"linear": 0, "cubic": 1}


def moddelay_tile(max_delay, channels):
    """Samples of a row that one workgroup of the modulated-delay kernels produces (MD_TILE in csrc/moddelay.hip): 2048
    for every ``max_delay`` and channel count -- the channels pass through the same LDS one after the other, and the
    largest backward tile (the read positions of 2048 + 8192 + 4 samples) is 60 KiB, two workgroups per CU."""
    _int_in("moddelay_tile", "max_delay", max_delay, 2, MODDELAY_MAX_DELAY)
    _int_in("moddelay_tile", "channels", channels, 1, 2 ** 31 - 1)
    return 2048


def _moddelay_args(what, x, delay, depth, rate, phase, gain, dry, max_delay, interp):
    """The configuration and the parameter shapes of the modulated-delay pair, checked before anything is allocated ->
    (the signal's row map, R, C, L, V, the interpolation's number, the six parameter arrays in the entries' shapes)."""
    _int_in(what, "max_delay", max_delay, 2, MODDELAY_MAX_DELAY)
    if interp not in _MODDELAY_INTERP:
        raise ValueError(f"{what}: interp={interp!r} must be one of {sorted(_MODDELAY_INTERP)}")
    xmap, R, C, L = rowmap(x)
    if delay.ndim != 2 or delay.shape[0] != R or not 1 <= delay.shape[1] <= MODDELAY_MAX_VOICES:
        raise ValueError(f"{what}: delay must be ({R}, V) with V in 1..{MODDELAY_MAX_VOICES}, got {tuple(delay.shape)}")
    V = delay.shape[1]
    for name, p, shape in (("depth", depth, (R, V)), ("rate", rate, (R, V)), ("phase", phase, (R, V, C)),
                           ("gain", gain, (R, V, C))):
        _expect(p, shape, f"{what}: {name}")
    if dry.numel() != R:
        raise ValueError(f"{what}: {dry.numel()} dry gains for {R} rows")
    return xmap, R, C, L, V, _MODDELAY_INTERP[interp], (delay, depth, rate, phase, gain, dry.reshape(R))


def _moddelay_position(pos, R, device, what):
    """The position half of a modulated-delay state: a contiguous int64 (R,) tensor on the signal's device."""
    if not isinstance(pos, torch.Tensor) or pos.device != device or pos.dtype != torch.int64 or tuple(pos.shape) != (R,) \
            or not pos.is_contiguous():
        got = f"{tuple(pos.shape)} {pos.dtype} on {pos.device}" if isinstance(pos, torch.Tensor) else type(pos).__name__
        raise ValueError(f"{what}: the state's position must be a contiguous int64 tensor of shape ({R},) on {device}, got {got}")
    return pos


@_on_device
def moddelay(x, delay, depth, rate, phase, gain, dry, max_delay, interp="cubic", out=None, state=None, return_state=False):
    """Modulated delay line in one fused pass (gfx_moddelay_f32).  Per row r, channel c and voice v, at the absolute
    position p of sample n (p = n, or the state's position + n):

        theta = rate[r,v] p + phase[r,v,c]                             cycles; in double, reduced mod 1
        d     = clamp(delay[r,v] + depth[r,v] sin(2 pi theta), 1, max_delay)   samples; in double
        i = floor(d), f = d - i;   u[v,c,n] = sum_j l_j(f) x[c, n - i - j]
        y[c,n] = dry[r] x[c,n] + sum_v gain[r,v,c] u[v,c,n]

    with the linear (j = 0, 1) or third-order Lagrange (j = -1 .. 2) weights l_j of ``interp``.  ``delay``, ``depth``,
    ``rate``: (R, V) with V <= 8, in samples, samples and cycles per sample; ``phase`` (cycles), ``gain``: (R, V, C);
    ``dry``: (R,) or (R, 1); float32 on the GPU.  The caller's contract, which cannot be checked without reading the
    parameters back: 2 pi rate depth <= 1/2 -- outside it nothing is read or written out of place, and the values (of
    the backward in particular) are unspecified.

    ``x`` / ``out``: (R,C,L) tensors or strided (B,n,C,L) views; ``out`` may never share memory with ``x``.  ``state``:
    the pair (history, position) -- the last max_delay + 2 input samples, contiguous float32 (R, C, max_delay + 2), oldest
    first, and the samples rendered so far, contiguous int64 (R,) on the device (None: silence at position 0); with
    ``state`` or ``return_state`` the new pair comes back too, and blocks cut anywhere give the bits of the one-call
    output.  -> y, or (y, state).  Equal bits from call to call; a row's result does not depend on the other rows."""
    what = "moddelay"
    _require_gpu(x, delay, depth, rate, phase, gain, dry, out)
    xmap, R, C, L, V, mode, params = _moddelay_args(what, x, delay, depth, rate, phase, gain, dry, max_delay, interp)
    S = max_delay + 2
    zi, pos = _pair_state(what, state, (R, C, S), "position", lambda pos: _moddelay_position(pos, R, x.device, what))
    stateful = state is not None or return_state
    out, ymap = _output(out, (R, C, L), x.device, what, apart=(x, zi, pos, *params))
    zf = torch.empty((R, C, S), dtype=torch.float32, device=x.device) if stateful else None
    pos_out = torch.empty(R, dtype=torch.int64, device=x.device) if stateful else None
    pin = _Pin()
    with _timed("moddelay_kernel", 8 * R * C * L):
        check(lib().gfx_moddelay_f32(_ptr(x), xmap, _ptr(out), ymap, R, C, L, V, mode, max_delay, *(pin(p) for p in params),
                                     _ptr(zi), _ptr(pos), _ptr(zf), _ptr(pos_out), _stream()), "gfx_moddelay_f32")
    return (out, (zf, pos_out)) if stateful else out


@_on_device
def moddelay_bwd(x, gy, delay, depth, rate, phase, gain, dry, max_delay, interp="cubic", out=None, want=MODDELAY_GRADS,
                 ws=None):
    """Backward of :func:`moddelay` (a call without a state) in one call (gfx_moddelay_bwd_f32) -> (gx, g_delay, g_depth,
    g_rate, g_phase, g_gain, g_dry), each shaped like its parameter (g_dry (R,)), None for what ``want`` (any of
    MODDELAY_GRADS) leaves out.  Nothing of the forward is needed but its arguments.  The gradients are taken almost
    everywhere: the clamp of the delay passes none where it binds.

    ``x``, ``gy``: (R,C,L) or strided (B,n,C,L) views; ``gx`` is ``out`` (any view of the signal's shape, apart from x and
    gy) or a new (R,C,L) tensor.  ``ws``: a uint8 workspace of at least gfx_moddelay_bwd_ws_bytes(R, C, L, V) bytes to
    reuse, 8-byte aligned (only the parameter gradients need one).  Equal bits from call to call."""
    what = "moddelay_bwd"
    _require_gpu(x, gy, delay, depth, rate, phase, gain, dry, out)
    xmap, R, C, L, V, mode, params = _moddelay_args(what, x, delay, depth, rate, phase, gain, dry, max_delay, interp)
    gmap = _cotangent(what, gy, x, (R, C, L))
    _want(what, want, MODDELAY_GRADS, some=True)
    reads = (x, gy, *params)
    gx, gxmap = _signal_grad(what, want, out, (R, C, L), xmap, x.device, (*reads, ws))
    shapes = {"delay": (R, V), "depth": (R, V), "rate": (R, V), "phase": (R, V, C), "gain": (R, V, C), "dry": (R,)}
    grads = _param_grads(want, shapes, x.device)
    pin = _Pin()
    wsarg = (0, 0)
    if any(g is not None for g in grads):
        wsarg = _workspace(what, ws, lib().gfx_moddelay_bwd_ws_bytes(R, C, L, V), x.device, pin, reads, align=8)
    with _timed("moddelay_bwd_kernel", (8 if gx is None else 12) * R * C * L):
        check(lib().gfx_moddelay_bwd_f32(_ptr(x), xmap, _ptr(gy), gmap, R, C, L, V, mode, max_delay, *(pin(p) for p in params),
                                         _ptr(gx), gxmap, *(_ptr(g) for g in grads), *wsarg, _stream()), "gfx_moddelay_bwd_f32")
    return (gx, *grads)


# ----------------------------------------------------------------------------------------- feedback delay
FBDELAY_MIN_DELAY = 64
FBDELAY_MAX_DELAY = 65536
FBDELAY_CHUNK = 1024           # FB_CHUNK of csrc/fbdelay.hip: the longest run of samples one step of the walk produces
FBDELAY_GRADS = ("x", "delay", "damping", "feedback", "dry", "wet")


def _fbdelay_args(what, x, delay, damping, feedback, dry, wet, max_delay):
    """The configuration and the parameter shapes of the feedback-delay pair, checked before anything is allocated ->
    (the signal's row map, R, C, L, the five parameter arrays in the entries' shapes)."""
    _int_in(what, "max_delay", max_delay, FBDELAY_MIN_DELAY, FBDELAY_MAX_DELAY)
    xmap, R, C, L = rowmap(x)
    if C not in (1, 2):
        raise ValueError(f"{what}: {C} channels, the loop takes 1 or 2")
    for name, p, shape in (("delay", delay, (R, C)), ("damping", damping, (R, C)), ("feedback", feedback, (R, C, C))):
        _expect(p, shape, f"{what}: {name}")
    for name, p in (("dry", dry), ("wet", wet)):
        if p.numel() != R:
            raise ValueError(f"{what}: {p.numel()} {name} gains for {R} rows")
    return xmap, R, C, L, (delay, damping, feedback, dry.reshape(R), wet.reshape(R))


@_on_device
def fbdelay(x, delay, damping, feedback, dry, wet, max_delay, out=None, state=None, return_state=False, tape=False):
    """Feedback delay (echo, ping-pong) on the recursive chunk walk (gfx_fbdelay_f32).  Per row r and channels c, c':

        i_c = floor(delay[r,c]), f_c = delay[r,c] - i_c                 64 <= delay <= max_delay <= 65536, in samples
        s_c[n] = (1 - f_c) w_c[n - i_c] + f_c w_c[n - i_c - 1]
        q_c[n] = (1 - a[r,c]) s_c[n] + a[r,c] q_c[n - 1]                a = damping, 0 <= a < 1
        w_c[n] = x_c[n] + sum_c' F[r,c,c'] q_c'[n]                      F = feedback
        y_c[n] = dry[r] x_c[n] + wet[r] q_c[n]

    ``delay``, ``damping``: (R, C) with C = 1 or 2; ``feedback``: (R, C, C); ``dry``, ``wet``: (R,) or (R, 1); float32 on
    the GPU.  The caller's contract, which cannot be checked without reading the parameters back: every row sum of
    |F| < 1, 0 <= a < 1 and the delay's range -- outside it nothing is read or written out of place, and the values are
    unspecified.

    ``x`` / ``out``: (R,C,L) tensors or strided (B,n,C,L) views; ``out`` may never share memory with ``x``.  ``state``:
    the pair (history, q_last) -- the last max_delay + 1 samples of w, contiguous float32 (R, C, max_delay + 1), oldest
    first, and the loop filter's last value, (R, C) (None: silence); with ``state`` or ``return_state`` the new pair comes
    back too.  The walk restarts at each call: blocks agree with the one call to rounding, and the same sequence of calls
    gives the same bits.  ``tape``: also return the (R,C,L) signals (q, w) that :func:`fbdelay_bwd` reads.
    -> y, or (y, state), with ``tape`` y, [state,] (q, w).  Equal bits from call to call; a row's result does not depend
    on the other rows."""
    what = "fbdelay"
    _require_gpu(x, delay, damping, feedback, dry, wet, out)
    xmap, R, C, L, params = _fbdelay_args(what, x, delay, damping, feedback, dry, wet, max_delay)
    S = max_delay + 1
    zi, q_in = _pair_state(what, state, (R, C, S), "q_last", lambda q: _state(q, (R, C), what, "the state's q_last"))
    stateful = state is not None or return_state
    out, ymap = _output(out, (R, C, L), x.device, what, apart=(x, zi, q_in, *params))
    zf = torch.empty((R, C, S), dtype=torch.float32, device=x.device) if stateful else None
    q_out = torch.empty((R, C), dtype=torch.float32, device=x.device) if stateful else None
    q = torch.empty((R, C, L), dtype=torch.float32, device=x.device) if tape else None
    w = torch.empty((R, C, L), dtype=torch.float32, device=x.device)        # the line: the entry's workspace
    pin = _Pin()
    with _timed("fbdelay_kernel", 12 * R * C * L):
        check(lib().gfx_fbdelay_f32(_ptr(x), xmap, _ptr(out), ymap, R, C, L, max_delay, *(pin(p) for p in params), _ptr(zi),
                                    _ptr(q_in), _ptr(zf), _ptr(q_out), _ptr(q), _ptr(w), 4 * w.numel(), _stream()),
              "gfx_fbdelay_f32")
    res = (out, (zf, q_out)) if stateful else (out,)
    if tape:
        res = (*res, (q, w))
    return res if len(res) > 1 else out


@_on_device
def fbdelay_bwd(x, gy, q, w, delay, damping, feedback, dry, wet, max_delay, out=None, want=FBDELAY_GRADS, ws=None):
    """Backward of :func:`fbdelay` (a call without a state) in one call (gfx_fbdelay_bwd_f32) -> (gx, g_delay, g_damping,
    g_feedback, g_dry, g_wet), each shaped like its parameter (g_dry, g_wet (R,)), None for what ``want`` (any of
    FBDELAY_GRADS) leaves out.  ``q``, ``w``: the contiguous (R,C,L) signals the forward returned with ``tape=True``.

    ``x``, ``gy``: (R,C,L) or strided (B,n,C,L) views; ``gx`` is ``out`` (any view of the signal's shape, apart from x and
    gy) or a new (R,C,L) tensor.  ``ws``: a uint8 workspace of at least gfx_fbdelay_bwd_ws_bytes(R, C, L) bytes to reuse,
    8-byte aligned (the adjoint's line and the tile sums).  Equal bits from call to call."""
    what = "fbdelay_bwd"
    _require_gpu(x, gy, q, w, delay, damping, feedback, dry, wet, out)
    xmap, R, C, L, params = _fbdelay_args(what, x, delay, damping, feedback, dry, wet, max_delay)
    gmap = _cotangent(what, gy, x, (R, C, L))
    q = _state(q, (R, C, L), what, "q")
    w = _state(w, (R, C, L), what, "w")
    if q is None or w is None:
        raise ValueError(f"{what}: q and w, the signals of fbdelay(tape=True), are needed")
    _want(what, want, FBDELAY_GRADS, some=True)
    reads = (x, gy, q, w, *params)
    gx, gxmap = _signal_grad(what, want, out, (R, C, L), xmap, x.device, (*reads, ws))
    shapes = {"delay": (R, C), "damping": (R, C), "feedback": (R, C, C), "dry": (R,), "wet": (R,)}
    grads = _param_grads(want, shapes, x.device)
    pin = _Pin()
    wsarg = _workspace(what, ws, lib().gfx_fbdelay_bwd_ws_bytes(R, C, L), x.device, pin, reads, align=8)
    with _timed("fbdelay_bwd_kernel", 24 * R * C * L):
        check(lib().gfx_fbdelay_bwd_f32(_ptr(x), xmap, _ptr(gy), gmap, _ptr(q), _ptr(w), R, C, L, max_delay,
                                        *(pin(p) for p in params), _ptr(gx), gxmap, *(_ptr(g) for g in grads), *wsarg, _stream()),
              "gfx_fbdelay_bwd_f32")
    return (gx, *grads)


# ----------------------------------------------------------------------------------------- reverb IR
@_on_device
def istft_basis(window):
    _require_gpu(window)
    n_fft = window.numel()
    basis = torch.empty(lib().gfx_istft_basis_bytes(n_fft) // 4, dtype=torch.float32, device=window.device)
    pin = _Pin()
    check(lib().gfx_istft_basis_f32(pin(window), _ptr(basis), n_fft, _stream()), "gfx_istft_basis_f32")
    return basis


STFT_MAX_N_FFT = 2048      # the frame the direct-sum kernel holds in LDS (gfx_stft_f32)


@_on_device
def stft(x, window, hop):
    """torch.stft(x, n_fft, hop, window, center=True, pad_mode="reflect", return_complex=True) for rows x (rows, T) on the
    direct-sum kernel (gfx_stft_f32): -> (rows, n_fft // 2 + 1, 1 + T // hop) complex64."""
    _require_gpu(x)
    if x.ndim != 2:
        raise ValueError(f"stft: rows of samples (rows, T) expected, got {tuple(x.shape)}")
    if not isinstance(window, torch.Tensor) or window.ndim != 1 or window.dtype != torch.float32 or window.device != x.device:
        is_tensor = isinstance(window, torch.Tensor)
        got = f"{tuple(window.shape)} {window.dtype} on {window.device}" if is_tensor else type(window).__name__
        raise ValueError(f"stft: the window must be a one-dimensional float32 tensor on {x.device}, got {got}")
    rows, T = x.shape
    n_fft = window.numel()
    # the limits of gfx_stft_f32 (csrc/stft.hip), which answers a bare GFX_EINVAL for each
    if n_fft < 2 or n_fft > STFT_MAX_N_FFT or n_fft % 2:
        raise ValueError(f"stft: n_fft must be even, from 2 to {STFT_MAX_N_FFT}, got {n_fft} (the window's length)")
    if hop < 1:
        raise ValueError(f"stft: hop must be at least 1, got {hop}")
    if T <= n_fft // 2:
        raise ValueError(f"stft: rows of {T} samples are too short for n_fft = {n_fft}: the reflect padding needs more than "
                         f"n_fft // 2 = {n_fft // 2}")
    x = x.contiguous()
    frames = 1 + T // hop
    out = torch.empty((rows, n_fft // 2 + 1, frames, 2), dtype=torch.float32, device=x.device)
    pin = _Pin()
    for i, n in _row_chunks(rows, GRID_YZ_MAX):
        check(lib().gfx_stft_f32(_ptr(x[i:]), pin(window), _ptr(out[i:]), n, T, n_fft, hop, _stream()), "gfx_stft_f32")
    return torch.view_as_complex(out)


ISTFT_SCHEDULES = {"auto": 0, "gemm": 1, "fft": 2}   # GFX_ISTFT_* (include/grafx_amd.h)


def _reverb_noise(what, noise_stft, R):
    """The noise of the reverb pair: one spectrum shared by all R rows, or (R,2,K,T) fresh noise per row.  -> cut(r0, n) =
    (pointer, number of spectra) for rows r0 .. r0 + n of the float32 (...,2,K,T,2) view of the complex64 buffer."""
    rows = noise_stft.shape[0] if noise_stft.ndim == 4 else 1
    if rows not in (1, R):
        raise ValueError(f"{what}: {rows} noise spectra for {R} rows")
    nz = torch.view_as_real(noise_stft.contiguous())
    return lambda r0, n: (_ptr(nz), 1) if rows == 1 else (_ptr(nz[r0:r0 + n]), n)


@_on_device
def stft_reverb_ir(noise_stft, init_lm, delta_lm, gain_env, window, basis, ir_len, hop, ms_to_lr, schedule="auto"):
    """-> (ir (R,2,ir_len) un-normalised, row_gain (R) = 1/sqrt(mean_c sum_t ir^2 + 1e-12)).  `schedule`: how the frames
    are transformed -- "gemm" (matrix cores, any even n_fft), "fft" (n_fft 384 / hop 192 only), "auto"."""
    _require_gpu(init_lm, delta_lm, gain_env, window, basis)
    R = init_lm.shape[0]
    n_fft = window.numel()
    T = noise_stft.shape[-1]
    noise = _reverb_noise("stft_reverb_ir", noise_stft, R)
    ir = torch.empty((R, 2, ir_len), dtype=torch.float32, device=init_lm.device)
    row_gain = torch.empty((R,), dtype=torch.float32, device=init_lm.device)
    sched = ISTFT_SCHEDULES[schedule]
    init_lm, delta_lm = init_lm.contiguous(), delta_lm.contiguous()
    gain_env = None if gain_env is None else gain_env.contiguous()
    for r0, n in _row_chunks(R, GRID_ROWS_I16_MAX):
        pin = _Pin()
        ws = pin.workspace(lib().gfx_stft_reverb_workspace_bytes(n, ir_len, n_fft, hop, T, sched), init_lm.device)
        check(
            lib().gfx_stft_reverb_ir_f32(*noise(r0, n), pin(init_lm[r0:r0 + n]), pin(delta_lm[r0:r0 + n]),
                                         pin(None if gain_env is None else gain_env[r0:r0 + n]), pin(window), pin(basis),
                                         _ptr(ir[r0:r0 + n]), _ptr(row_gain[r0:r0 + n]), n, ir_len, n_fft, hop, T,
                                         int(ms_to_lr), *ws, sched, _stream()),
            "gfx_stft_reverb_ir_f32",
        )
    return ir, row_gain


def stft_reverb_ir_bwd_ws_bytes(R, ir_len):
    """Bytes of workspace one gfx_stft_reverb_ir_bwd_f32 call over R rows needs (no GPU involved)."""
    return lib().gfx_stft_reverb_ir_bwd_ws_bytes(R, ir_len)


@_on_device
def stft_reverb_ir_bwd(grad_ir, noise_stft, init_lm, delta_lm, gain_env, window, basis, hop, ms_to_lr, ir=None,
                       row_gain=None, want_gain_env=True, ws=None):
    """Backward of :func:`stft_reverb_ir` with the "fft" schedule (n_fft 384 / hop 192 only; gfx_stft_reverb_ir_bwd_f32)
    -> (g_init (R,2,193), g_delta (R,2,193), g_gain_env (R,2,T) or None).

    ``grad_ir``: dL/dh (R,2,ir_len).  With ``ir`` and ``row_gain`` (the forward's outputs) h = row_gain * ir, the
    normalised taps; without them h = ir.  The other arguments are the forward's; ``noise_stft`` per row must be the
    noise the forward used.  ``g_gain_env`` is computed when ``gain_env`` is given and ``want_gain_env`` is set.
    ``ws``: a uint8 workspace of at least ``stft_reverb_ir_bwd_ws_bytes(min(R, 32767), ir_len)`` bytes to reuse, apart from
    everything the call reads."""
    _require_gpu(grad_ir, init_lm, delta_lm, gain_env, window, basis, ir, row_gain)
    R, _, ir_len = grad_ir.shape
    n_fft = window.numel()
    T = noise_stft.shape[-1]
    if (ir is None) != (row_gain is None):
        raise ValueError("stft_reverb_ir_bwd: ir and row_gain come together (the normalised taps) or not at all")
    if init_lm.shape[0] != R or (ir is not None and tuple(ir.shape) != tuple(grad_ir.shape)):
        raise ValueError(f"stft_reverb_ir_bwd: gradient {tuple(grad_ir.shape)} does not match the {init_lm.shape[0]} rows")
    noise = _reverb_noise("stft_reverb_ir_bwd", noise_stft, R)
    grad_ir, init_lm, delta_lm = grad_ir.contiguous(), init_lm.contiguous(), delta_lm.contiguous()
    gain_env = None if gain_env is None else gain_env.contiguous()
    ir = None if ir is None else ir.contiguous()
    row_gain = None if row_gain is None else row_gain.contiguous()
    g_init, g_delta = torch.empty_like(init_lm), torch.empty_like(delta_lm)
    g_env = torch.empty_like(gain_env) if (gain_env is not None and want_gain_env) else None
    held = _Pin()                                # (the workspace serves every chunk of rows)
    wsarg = _workspace("stft_reverb_ir_bwd", ws, lib().gfx_stft_reverb_ir_bwd_ws_bytes(min(R, GRID_ROWS_I16_MAX), ir_len),
                       grad_ir.device, held, (grad_ir, noise_stft, init_lm, delta_lm, gain_env, window, basis, ir, row_gain,
                                              g_init, g_delta, g_env))
    cut = lambda t, r0, n: None if t is None else t[r0:r0 + n]  # noqa: E731
    for r0, n in _row_chunks(R, GRID_ROWS_I16_MAX):
        pin = _Pin()
        check(
            lib().gfx_stft_reverb_ir_bwd_f32(_ptr(grad_ir[r0:r0 + n]), _ptr(cut(ir, r0, n)), _ptr(cut(row_gain, r0, n)),
                                             *noise(r0, n), pin(init_lm[r0:r0 + n]),
                                             pin(delta_lm[r0:r0 + n]), pin(cut(gain_env, r0, n)), pin(window), pin(basis),
                                             _ptr(g_init[r0:r0 + n]), _ptr(g_delta[r0:r0 + n]), _ptr(cut(g_env, r0, n)), n,
                                             ir_len, n_fft, hop, T, int(ms_to_lr), *wsarg, _stream()),
            "gfx_stft_reverb_ir_bwd_f32",
        )
    return g_init, g_delta, g_env


# ----------------------------------------------------------------------------------------- STFT loss
def stft_loss_ws_bytes(R, L, n_fft, hop):
    """Bytes of workspace one gfx_stft_loss_sums_f32 / gfx_stft_loss_bwd_f32 call needs (no GPU involved): 16 per row and
    run of 16384 / n_fft frames; 0 for a resolution outside the native range (n_fft a power of two in [128, 2048],
    1 <= hop <= n_fft, L > n_fft / 2)."""
    return lib().gfx_stft_loss_ws_bytes(R, L, n_fft, hop)


def _loss_rows(t, what, name, view_only=False):
    """A (..., L) signal of the STFT loss as a (B, C, L) view and the RowMap of its B * C single rows (row r at
    (r / C) * stride(0) + (r % C) * stride(1)): a (B, C, L) slice of a larger buffer is addressed in place.  Leading
    dimensions that do not fold into two strides are copied -- or refused, for a tensor the call writes (``view_only``)."""
    if t.ndim < 2:
        raise ValueError(f"{what}: {name} must be (..., L) with at least one leading dimension, got {tuple(t.shape)}")
    if t.stride(-1) != 1:
        if view_only:
            raise ValueError(f"{what}: the last dimension of {name} must be contiguous")
        t = t.contiguous()
    if t.ndim == 2:
        t3 = t.unsqueeze(1)
    elif t.ndim == 3:
        t3 = t
    elif view_only:
        try:
            t3 = t.view(-1, *t.shape[-2:])
        except RuntimeError:
            raise ValueError(f"{what}: the leading dimensions of {name} {tuple(t.shape)} (strides {tuple(t.stride())}) do not "
                             f"fold into one") from None
    else:
        t3 = t.reshape(-1, *t.shape[-2:])
    return t3, RowMap(max(t3.shape[1], 1), t3.stride(0), t3.stride(1), 0)


def _loss_args(what, pred, target, window, hop):
    _require_gpu(pred, target, window)
    if pred.shape != target.shape:
        raise ValueError(f"{what}: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ in shape")
    p3, pmap = _loss_rows(pred, what, "pred")
    t3, tmap = _loss_rows(target, what, "target")
    B, C, L = p3.shape
    n_fft = window.numel()
    nbytes = lib().gfx_stft_loss_ws_bytes(B * C, L, n_fft, hop)
    if not nbytes:
        raise ValueError(f"{what}: n_fft={n_fft} (the window's length), hop={hop}, L={L} with {B * C} rows is outside the "
                         f"native range: n_fft a power of two in [128, 2048], 1 <= hop <= n_fft, L > n_fft / 2")
    return p3, pmap, t3, tmap, B * C, L, n_fft, nbytes


def _loss_sums(what, pred, target, window, hop, eps, ws, bank=None):
    """The body of :func:`stft_loss_sums` and, with ``bank`` = (fb, bands), of :func:`stft_band_loss_sums`."""
    p3, pmap, t3, tmap, R, L, n_fft, nbytes = _loss_args(what, pred, target, window, hop)
    entry, kernel, banked, bank_args = "gfx_stft_loss_sums_f32", "stft_loss_sums_kernel", (), ()
    if bank is not None:
        fb, bands, n_bins = _band_args(what, *bank, n_fft)
        entry, kernel, banked = "gfx_stft_band_loss_sums_f32", "stft_band_loss_sums_kernel", (fb, *bands)
        bank_args = (_ptr(fb), _ptr(bands[0]), _ptr(bands[1]), n_bins)
    sums = torch.empty((R, 4), dtype=torch.float32, device=pred.device)
    pin = _Pin()
    wsarg = _workspace(what, ws, nbytes, pred.device, pin, (p3, t3, window, *banked), align=16)
    with _timed(kernel, 4 * R * L * 2):
        check(getattr(lib(), entry)(_ptr(p3), pmap, _ptr(t3), tmap, pin(window), *bank_args, _ptr(sums), R, L, n_fft, hop, eps,
                                    *wsarg, _stream()), entry)
    return sums


def _loss_bwd(what, pred, target, window, hop, coef, eps, out, accumulate, ws, bank=None):
    """The body of :func:`stft_loss_bwd` and, with ``bank`` = (fb, bands), of :func:`stft_band_loss_bwd`."""
    _require_gpu(coef, out)
    p3, pmap, t3, tmap, R, L, n_fft, nbytes = _loss_args(what, pred, target, window, hop)
    entry, kernel, banked, bank_args = "gfx_stft_loss_bwd_f32", "stft_loss_bwd_kernel", (), ()
    if bank is not None:
        fb, bands, n_bins = _band_args(what, *bank, n_fft)
        entry, kernel, banked = "gfx_stft_band_loss_bwd_f32", "stft_band_loss_bwd_kernel", (fb, *bands)
        bank_args = (*(_ptr(b) for b in banked), n_bins)
    _expect(coef, (R, 3), what + ": coef")
    if accumulate and out is None:
        raise ValueError(f"{what}: accumulate adds to a given out")
    reads = (p3, t3, window, coef, *banked)
    if out is not None:
        if out.shape != pred.shape:
            raise ValueError(f"{what}: out {tuple(out.shape)} does not match pred {tuple(pred.shape)}")
        o3, gmap = _loss_rows(out, what, "out", view_only=True)
        _output(o3, tuple(p3.shape), pred.device, what, apart=(*reads, ws))
    else:
        out = torch.empty(pred.shape, dtype=torch.float32, device=pred.device)
        o3, gmap = _loss_rows(out, what, "out", view_only=True)
    pin = _Pin()
    wsarg = _workspace(what, ws, nbytes, pred.device, pin, reads, align=16)
    with _timed(kernel, 4 * R * L * (4 if accumulate else 3)):
        check(getattr(lib(), entry)(_ptr(p3), pmap, _ptr(t3), tmap, pin(window), *bank_args, pin(coef), _ptr(o3), gmap, R, L,
                                    n_fft, hop, eps, int(bool(accumulate)), *wsarg, _stream()), entry)
    return out


@_on_device
def stft_loss_sums(pred, target, window, hop, eps=1e-8, ws=None):
    """The four sums of one resolution of an STFT magnitude loss per row (gfx_stft_loss_sums_f32) -> (R, 4) float32:
    A = sum (|T|-|P|)^2, B = sum |T|^2, E = sum ||T|-|P||, D = sum |log|T| - log|P|| over the bins and frames of
    P = torch.stft(pred, n_fft, hop, window=window, center=True, pad_mode="reflect") and T likewise, magnitudes floored at
    sqrt(eps).  ``pred`` / ``target``: (..., L) of one shape, R = the product of the leading dimensions; a (B, C, L) slice
    of a larger buffer is read in place.  ``window``: n_fft floats, n_fft a power of two in [128, 2048].  ``ws``: a uint8
    workspace of at least ``stft_loss_ws_bytes(R, L, n_fft, hop)`` bytes to reuse, 16-byte aligned, apart from everything
    the call reads.  Nothing of a spectrogram's size is allocated; equal bits from call to call."""
    return _loss_sums("stft_loss_sums", pred, target, window, hop, eps, ws)


@_on_device
def stft_loss_bwd(pred, target, window, hop, coef, eps=1e-8, out=None, accumulate=False, ws=None):
    """Gradient with respect to ``pred`` of sum_r (cA A + cE E + cD D)[r], the sums of :func:`stft_loss_sums`, with
    ``coef`` (R, 3) = (cA, cE, cD) per row (gfx_stft_loss_bwd_f32) -> a tensor of pred's shape.  The frames are
    recomputed from ``pred`` and ``target``; every gradient sample is stored once.  ``out``: the destination (pred's shape;
    any view whose leading dimensions fold into two strides), required with ``accumulate``, which adds to what it holds
    -- the resolutions of one loss sum into one tensor.  It may share memory with nothing the call reads.  ``ws``: as for
    :func:`stft_loss_sums`."""
    return _loss_bwd("stft_loss_bwd", pred, target, window, hop, coef, eps, out, accumulate, ws)


def _band_args(what, fb, bands, n_fft):
    """The filterbank of a banded STFT loss call, checked: ``fb`` (n_bins, n_fft / 2 + 1) float32 and ``bands`` =
    (row_lo, row_hi, col_lo, col_hi), int32 on the GPU (losses.filterbank_bands) -> (fb, the four arrays, n_bins), all
    contiguous.  What the arrays hold is not read here (that would synchronise): it is the caller's, as the header says."""
    _require_gpu(fb)
    bins = n_fft // 2 + 1
    if fb.ndim != 2 or fb.shape[1] != bins or not 1 <= fb.shape[0] <= bins:
        raise ValueError(f"{what}: the filterbank must be (n_bins, n_fft / 2 + 1 = {bins}) with 1 <= n_bins <= {bins}, got "
                         f"{tuple(fb.shape)}")
    if fb.requires_grad:
        raise ValueError(f"{what}: the filterbank gets no gradient (detach it)")
    if len(bands) != 4:
        raise ValueError(f"{what}: bands are (row_lo, row_hi, col_lo, col_hi), got {len(bands)} entries")
    for name, b, n in zip(("row_lo", "row_hi", "col_lo", "col_hi"), bands, (fb.shape[0], fb.shape[0], bins, bins)):
        if not isinstance(b, torch.Tensor) or not b.is_cuda or b.dtype != torch.int32 or tuple(b.shape) != (n,):
            raise ValueError(f"{what}: {name} must be {n} int32 on the GPU")
    return fb.contiguous(), tuple(b.contiguous() for b in bands), fb.shape[0]


@_on_device
def stft_band_loss_sums(pred, target, window, hop, fb, bands, eps=1e-8, ws=None):
    """:func:`stft_loss_sums` on a filterbank scale (gfx_stft_band_loss_sums_f32) -> (R, 4) float32: with
    Pm = fb @ |P| and Tm = fb @ |T| per frame (magnitudes floored at sqrt(eps) per bin),  A = sum (Tm-Pm)^2, B = sum Tm^2,
    E = sum |Tm-Pm|, D = sum |log Tm - log Pm| over the n_bins bands of all frames.  ``fb``: (n_bins, n_fft / 2 + 1)
    non-negative weights, staircase banded; ``bands``: what ``losses.filterbank_bands(fb)`` returned, on the GPU.  The
    rest as for :func:`stft_loss_sums`, the workspace included."""
    return _loss_sums("stft_band_loss_sums", pred, target, window, hop, eps, ws, bank=(fb, bands))


@_on_device
def stft_band_loss_bwd(pred, target, window, hop, fb, bands, coef, eps=1e-8, out=None, accumulate=False, ws=None):
    """:func:`stft_loss_bwd` for the sums of :func:`stft_band_loss_sums` (gfx_stft_band_loss_bwd_f32): the gradient with
    respect to ``pred`` of sum_r (cA A + cE E + cD D)[r] -> a tensor of pred's shape.  ``fb`` and ``bands`` as in the
    forward (the filterbank gets no gradient), everything else as for :func:`stft_loss_bwd`."""
    return _loss_bwd("stft_band_loss_bwd", pred, target, window, hop, coef, eps, out, accumulate, ws, bank=(fb, bands))


# ----------------------------------------------------------------------------------------- loudness
def kweight_energy_ws_bytes(R, C, L):
    """Bytes of workspace one gfx_kweight_energy_f32 / gfx_kweight_energy_bwd_f32 call needs (no GPU involved): 64 per
    row-channel and 1024-sample tile; 0 for a zero or negative argument."""
    return lib().gfx_kweight_energy_ws_bytes(R, C, L)


def _kweight_args(what, x, coef, hop):
    """What the two K-weighting entries share, checked: the signal's row map, the ten coefficients as a host array, the
    number of sub-blocks and the workspace's size."""
    xmap, R, C, L = rowmap(x)
    if isinstance(coef, torch.Tensor) and coef.is_cuda:
        raise ValueError(f"{what}: coef is read on the host at the call: a (2, 5) float64 CPU tensor or sequence")
    coef = torch.as_tensor(coef, dtype=torch.float64)
    _expect(coef, (2, 5), what + ": coef")
    if not torch.isfinite(coef).all():
        raise ValueError(f"{what}: coef holds a value that is not finite")
    _int_in(what, "hop", hop, 1, L)
    nbytes = lib().gfx_kweight_energy_ws_bytes(R, C, L)
    return xmap, R, C, L, (ctypes.c_double * 10)(*coef.reshape(-1).tolist()), L // hop, nbytes


@_on_device
def kweight_energy(x, coef, hop, ws=None):
    """Sub-block energies of x (R,C,L), or a strided (B,n,C,L) view, behind the two-biquad cascade ``coef``
    (gfx_kweight_energy_f32) -> (R, C, n_sub) float64, n_sub = L // hop: the sums of squares of the filtered signal over
    consecutive runs of ``hop`` samples; the samples from n_sub * hop on belong to none.  ``coef``: (2, 5) float64 on the
    CPU (or a sequence), (b0, b1, b2, a1, a2) per section, a0-normalised, the same for every row -- the K-weighting of
    loudness.k_weighting.  The recursion and the sums run in double.  ``ws``: a uint8 workspace of at least
    ``kweight_energy_ws_bytes(R, C, L)`` bytes to reuse.  Equal bits from call to call."""
    what = "kweight_energy"
    _require_gpu(x)
    xmap, R, C, L, c10, n_sub, nbytes = _kweight_args(what, x, coef, hop)
    energy = torch.empty((R, C, n_sub), dtype=torch.float64, device=x.device)
    pin = _Pin()
    wsarg = _workspace(what, ws, nbytes, x.device, pin, (x,), align=16)
    with _timed("kweight_energy_kernel", 4 * R * C * L * 2):     # x twice: the tiles' end states, then the energies
        check(lib().gfx_kweight_energy_f32(_ptr(x), xmap, c10, _ptr(energy), R, C, L, hop, *wsarg, _stream()),
              "gfx_kweight_energy_f32")
    return energy


@_on_device
def kweight_energy_bwd(x, coef, genergy, hop, out=None, accumulate=False, ws=None):
    """Gradient with respect to ``x`` of sum(genergy * kweight_energy(x, coef, hop)) (gfx_kweight_energy_bwd_f32) -> a
    float32 tensor of x's shape.  ``genergy``: (R, C, n_sub) float64 on the GPU.  The filtered signal is rebuilt from
    ``x``; every gradient sample is stored once, the samples from n_sub * hop on get 0.  ``out``: the destination (x's
    rows, channels and length; any strided (B,n,C,L) view), required with ``accumulate``, which adds to what it holds.
    What the call writes (``out``, ``ws``) may share memory with nothing it reads.  ``ws``: as for :func:`kweight_energy`."""
    what = "kweight_energy_bwd"
    _require_gpu(x, out)
    if not isinstance(genergy, torch.Tensor) or not genergy.is_cuda or genergy.dtype != torch.float64:
        raise TypeError(f"{what}: genergy must be a float64 tensor on the GPU")
    if accumulate and out is None:
        raise ValueError(f"{what}: accumulate adds to a given out")
    reads = (x, genergy)
    xmap, R, C, L, c10, n_sub, nbytes = _kweight_args(what, x, coef, hop)
    _expect(genergy, (R, C, n_sub), what + ": genergy")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    _, gmap = _output(out, (R, C, L), x.device, what, apart=(*reads, ws))
    pin = _Pin()
    wsarg = _workspace(what, ws, nbytes, x.device, pin, reads, align=16)
    # x three times (end states, the adjoint's end states, the adjoint), gx once
    with _timed("kweight_energy_bwd_kernel", 4 * R * C * L * (5 if accumulate else 4)):
        check(lib().gfx_kweight_energy_bwd_f32(_ptr(x), xmap, c10, pin(genergy), _ptr(out), gmap, R, C, L, hop,
                                               int(bool(accumulate)), *wsarg, _stream()), "gfx_kweight_energy_bwd_f32")
    return out


# ----------------------------------------------------------------------------------------- polyphase FIR
UPFIRDN_TILE = 1024          # GFX_UPFIRDN_TILE of include/grafx_amd.h: consecutive outputs of a row-channel per workgroup
UPFIRDN_MAX_RATIO = 1024     # up and down
UPFIRDN_MAX_TAPS = 16384


def upfirdn_absmax_ws_bytes(R, C, M):
    """Bytes of workspace one gfx_upfirdn_absmax_f32 call needs (no GPU involved): 16 per row-channel and tile of
    UPFIRDN_TILE outputs; 0 for a zero or negative argument."""
    return lib().gfx_upfirdn_absmax_ws_bytes(R, C, M)


def _upfirdn_args(what, x, h, up, down, offset, n_out):
    """What the two polyphase entries share, checked before anything is allocated: the signal's row map, the taps, the
    ratio, the offset and the number of outputs -> (xmap, R, C, L, N, M)."""
    _taps(what, "h", h, UPFIRDN_MAX_TAPS)
    N = h.numel()
    _int_in(what, "up", up, 1, UPFIRDN_MAX_RATIO)
    _int_in(what, "down", down, 1, UPFIRDN_MAX_RATIO)
    _int_in(what, "offset", offset, 0, N - 1)
    xmap, R, C, L = rowmap(x)
    if min(R, C, L) < 1:
        raise ValueError(f"{what}: x {tuple(x.shape)} holds no sample")
    M = -(-(L * up + N - 1 - offset) // down) if n_out is None else n_out
    if isinstance(M, bool) or not isinstance(M, int) or M < 1:
        raise ValueError(f"{what}: n_out={n_out!r} must be a positive integer")
    return xmap, R, C, L, N, M


@_on_device
def upfirdn(x, h, up, down, offset=0, n_out=None, out=None, accumulate=False):
    """y[r,c,m] = sum_k x[r,c,k] h[m down + offset - k up], m < n_out (gfx_upfirdn_f32): x (R,C,L), or a strided (B,n,C,L)
    view read in place, zero outside [0, L); ``h``: N <= 16384 float32 taps on the GPU, shared by every row, zero outside
    [0, N); ``up``, ``down`` in 1..1024; ``offset`` in 0..N-1.  -> (R, C, n_out) float32, or ``out``: a (R, C, n_out) tensor
    or strided (B, n, C, n_out) view, written in place (``accumulate``: added to; requires ``out``).  ``n_out`` defaults to
    ceil((L up + N - 1 - offset) / down), every output with a non-empty tap window; outputs beyond them are 0.0.  The adjoint
    with respect to x is ``upfirdn(g, h.flip(0), down, up, N - 1 - offset, n_out=L)``.  ``out`` may share memory with
    neither ``x`` nor ``h``.  Equal bits from call to call; a row's result does not depend on the other rows."""
    what = "upfirdn"
    _require_gpu(x, out)
    xmap, R, C, L, N, M = _upfirdn_args(what, x, h, up, down, offset, n_out)
    if accumulate and out is None:
        raise ValueError(f"{what}: accumulate adds to a given out")
    out, ymap = _output(out, (R, C, M), x.device, what, apart=(x, h))
    pin = _Pin()
    with _timed("upfirdn_kernel", 4 * R * C * (L + M)):
        check(lib().gfx_upfirdn_f32(_ptr(x), xmap, pin(h), N, up, down, offset, _ptr(out), ymap, R, C, L, M,
                                    int(bool(accumulate)), _stream()), "gfx_upfirdn_f32")
    return out


@_on_device
def upfirdn_absmax(x, h, up, down, offset=0, n_out=None, ws=None):
    """(peak, index) of :func:`upfirdn`'s output without writing it (gfx_upfirdn_absmax_f32): peak (R, C) float32, the
    largest |y[r,c,m]| over m < n_out, and index (R, C) int64, the lowest m that attains it (0.0 and 0 for an all-zero
    row).  ``ws``: a uint8 workspace of at least ``upfirdn_absmax_ws_bytes(R, C, n_out)`` bytes to reuse, 16-byte aligned,
    apart from ``x`` and ``h``.  Equal bits from call to call."""
    what = "upfirdn_absmax"
    _require_gpu(x)
    xmap, R, C, L, N, M = _upfirdn_args(what, x, h, up, down, offset, n_out)
    peak = torch.empty((R, C), dtype=torch.float32, device=x.device)
    index = torch.empty((R, C), dtype=torch.int64, device=x.device)
    pin = _Pin()
    wsarg = _workspace(what, ws, lib().gfx_upfirdn_absmax_ws_bytes(R, C, M), x.device, pin, (x, h), align=16)
    with _timed("upfirdn_absmax_kernel", 4 * R * C * L):
        check(lib().gfx_upfirdn_absmax_f32(_ptr(x), xmap, pin(h), N, up, down, offset, _ptr(peak), _ptr(index), R, C, L, M,
                                           *wsarg, _stream()), "gfx_upfirdn_absmax_f32")
    return peak, index


# ----------------------------------------------------------------------------------------- routing
@_on_device
def gather_sum(buf, src_idx, seg_ptr, out):
    """out[b,j] = sum of buf[b, src_idx[e]] over e in [seg_ptr[j], seg_ptr[j+1]); buf/out are (B,V,C,L) views."""
    # Outside the aliasing rule: ``out`` is usually a node range of ``buf`` itself, and which rows are read is in src_idx,
    # on the device -- reading it back would synchronise.  The render's planner keeps the destinations out of the sources
    # (render/plans.py, tests/test_mix_schedule.py).
    _require_gpu(buf, out)
    if buf.stride(-1) != 1 or out.stride(-1) != 1:
        raise ValueError("last dimension must be contiguous")
    B, _, C, L = buf.shape
    J = out.shape[1]
    if (out.shape[0], out.shape[2], out.shape[3]) != (B, C, L) or seg_ptr.numel() != J + 1:
        raise ValueError(f"gather_sum: output {tuple(out.shape)} / {seg_ptr.numel() - 1} segments do not match the "
                         f"buffer {tuple(buf.shape)}")
    if J * C > GRID_YZ_MAX:
        raise ValueError(f"gather_sum: {J} destinations x {C} channels ride on one grid dimension, at most {GRID_YZ_MAX}")
    with _timed("gather_sum_kernel", 4 * B * C * L * (src_idx.numel() + J)):
        for b0, nb in _row_chunks(B, GRID_YZ_MAX):     # the batch rides on a grid dimension: slices keep the views' strides
            check(
                lib().gfx_gather_sum_f32(_ptr(buf[b0:]), buf.stride(0), buf.stride(1), buf.stride(2), _ptr(src_idx),
                                         _ptr(seg_ptr), _ptr(out[b0:]), out.stride(0), out.stride(1), out.stride(2), nb, J, C, L,
                                         _stream()),
                "gfx_gather_sum_f32",
            )
    return out


@_on_device
def gather_sum_fanout(buf, unique_src, dest_mask, out):
    """Fan-out form of :func:`gather_sum`: source rows read once, up to 32 destinations (bit mask per source)."""
    # outside the aliasing rule, as gather_sum: the source rows are named on the device, the planner keeps them apart
    _require_gpu(buf, out)
    B, _, C, L = buf.shape
    J = out.shape[1]
    if (out.shape[0], out.shape[2], out.shape[3]) != (B, C, L) or dest_mask.numel() != unique_src.numel():
        raise ValueError(f"gather_sum_fanout: output {tuple(out.shape)} does not match the buffer {tuple(buf.shape)}")
    with _timed("gather_sum_kernel", 4 * B * C * L * (unique_src.numel() + J)):
        # the batch rides on a grid dimension; what the kernel refuses (alignment, J, C) it refuses for every slice alike,
        # so a refusal can only come from the first one, before anything is written
        for b0, nb in _row_chunks(B, GRID_YZ_MAX):
            code = lib().gfx_gather_sum_fanout_f32(_ptr(buf[b0:]), buf.stride(0), buf.stride(1), buf.stride(2), _ptr(unique_src),
                                                   _ptr(dest_mask), unique_src.numel(), _ptr(out[b0:]), out.stride(0),
                                                   out.stride(1), out.stride(2), nb, J, C, L, _stream())
            if code != 0:
                if b0 == 0:
                    return False
                check(code, "gfx_gather_sum_fanout_f32")
    return True
