"""What every wrapper of :mod:`grafx_amd.ops` goes through before its launch: the device and stream plumbing, the
per-launch timing hook, and the checks of the tensors whose pointers are passed.  The kernels trust their sizes, and a
RowMap carries strides only, so a destination, a carried state or a workspace is checked or made here, once, and
nowhere else: :func:`_output`, :func:`_state` and :func:`_workspace`, all on the aliasing rule of :func:`_apart`.  The
small checks more than one wrapper needs are here too: :func:`_expect` (a shape), :func:`_int_in` (an integer in a range),
:func:`_taps` (shared filter taps) and :func:`_pair_state` (a state of two parts).  So is the frame of a backward entry:
:func:`_want` (the gradients asked of it), :func:`_cotangent` (the shape of dL/dy), :func:`_signal_grad` (where the signal
gradient goes, and what it must be apart from) and :func:`_param_grads` (the wanted parameter gradients)."""
import contextvars
import functools

import torch

from ._lib import RowMap, lib


# Per-launch timing hook: `with ops.profiling() as prof:` collects (start_event, end_event, algorithmic_bytes) per kernel
# launch issued from the current context (bench.py's live roofline measurement).  A ContextVar, not a module global:
# another thread rendering at the same time neither pays for the events nor pollutes the record.
_PROFILE = contextvars.ContextVar("grafx_amd_profile", default=None)


class profiling:
    def __enter__(self):
        self.record = {}
        self.token = _PROFILE.set(self.record)
        return self.record

    def __exit__(self, *exc):
        _PROFILE.reset(self.token)
        return False


class _timed:
    """``last``: name of the library's ``gfx_*_last_kernel`` entry when the record is keyed by the kernel that ran, as a
    profile prints it (asked for only under a profile, and only when the block ended without an error; a block that
    launched nothing of its own sets ``t.last = None``)."""

    def __init__(self, name, nbytes, last=None):
        self.name, self.nbytes, self.last = name, nbytes, last

    def __enter__(self):
        self.rec = _PROFILE.get()
        if self.rec is not None:
            self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.rec is not None:
            self.b.record()
            if self.last is not None and exc[0] is None:
                self.name = getattr(lib(), self.last)().decode()
            self.rec.setdefault(self.name, []).append((self.a, self.b, self.nbytes))


def _require_gpu(*tensors):
    for t in tensors:
        if t is None:
            continue
        if not t.is_cuda:
            raise RuntimeError(
                "grafx_amd processors run on the MI355X only (got a CPU tensor); there is no CPU fallback. "
                "Move signals and parameters to the GPU, or use the reference/oracle on CPU."
            )
        if t.dtype != torch.float32:
            raise TypeError(f"grafx_amd kernels compute in float32, got {t.dtype}")


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return 0 if t is None else t.data_ptr()


class _Pin:
    """Pointer factory for ONE launch: ``pin(t)`` returns the device address of a contiguous version of ``t`` and
    keeps that (possibly temporary) tensor referenced until the wrapper returns, i.e. until the launch is enqueued.
    Taking ``data_ptr()`` of an unnamed ``.contiguous()`` result frees the temporary before the launch; the next
    same-size temporary then reuses the block and two arguments silently alias (round-1 advisor finding)."""

    def __init__(self):
        self.keep = []
        self.ws = None

    def __call__(self, t):
        if t is None:
            return 0
        t = t.contiguous()
        self.keep.append(t)
        return t.data_ptr()

    def workspace(self, nbytes, device, zero=False):
        """The (pointer, byte count) pair of the launch's workspace: ``nbytes`` fresh bytes, kept as ``pin.ws`` until the
        wrapper returns, or (0, 0) for no workspace (``nbytes`` 0 or False).  ``zero``: zero-filled."""
        if not nbytes:
            return 0, 0
        self.ws = (torch.zeros if zero else torch.empty)(nbytes, dtype=torch.uint8, device=device)
        return self.ws.data_ptr(), nbytes


def _on_device(fn):
    """Run a wrapper with the tensors' device current: the stream handed to the library (``_stream()``) and the
    library's per-device tables (``hipGetDevice`` in csrc/common.hip) both follow the *current* device, so tensors on
    cuda:1 under a current device cuda:0 would be launched on the wrong device.  All tensor arguments must share
    one device."""

    @functools.wraps(fn)
    def run(*args, **kwargs):
        dev = None
        for a in (*args, *kwargs.values()):
            if isinstance(a, torch.Tensor) and a.is_cuda:
                if dev is None:
                    dev = a.device
                elif a.device != dev:
                    raise ValueError(f"{fn.__name__}: tensors on different devices ({dev} and {a.device})")
        if dev is None or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)

    return run


def _expect(t, shape, what):
    """The kernels trust their sizes: every secondary tensor's shape is checked here, before its pointer is passed."""
    if t is not None and tuple(t.shape) != tuple(shape):
        raise ValueError(f"{what}: expected shape {tuple(shape)}, got {tuple(t.shape)}")


def rowmap(t):
    """RowMap for a (R, C, L) tensor or a (B, n, C, L) view whose last dim is contiguous.

    Lets kernels address slices of render_grafx's signal buffer in place.
    Returns (RowMap, R, C, L).
    """
    if t.stride(-1) != 1:
        raise ValueError("last dimension must be contiguous")
    if t.ndim == 3:
        R, C, L = t.shape
        return RowMap(max(R, 1), 0, t.stride(0), t.stride(1)), R, C, L
    if t.ndim == 4:
        B, n, C, L = t.shape
        return RowMap(max(n, 1), t.stride(0), t.stride(1), t.stride(2)), B * n, C, L
    raise ValueError(f"expected a 3-D or 4-D signal tensor, got {t.ndim}-D")


# Nodes the exact search of _overlap may visit before it answers True.  Views cut from one contiguous buffer visit at most
# two per level of the buffer's strides; only interleaved as_strided views come near the limit.
_OVERLAP_NODES = 256


def _overlap(a, b):
    """Whether two strided views share an element.  Never False when they do.  Exact whenever the search below ends within
    _OVERLAP_NODES nodes -- always for views cut from one contiguous buffer by slicing, indexing and permuting, whatever
    their extents: two node ranges of the render's (B, V, C, L) buffer interleave in memory without touching.  Integer
    arithmetic on addresses, shapes and strides only.

    An element of ``a`` at index i and one of ``b`` at index j coincide when address_a - address_b = sum_s (j_s - i_s) * s
    over the strides s of either view, with j_s - i_s anywhere in -(na_s - 1) .. nb_s - 1.  The strides are taken largest
    first, and a difference is tried only while what remains is within reach of the smaller strides."""
    if a.numel() == 0 or b.numel() == 0:
        return False
    low, reach, found = [a.data_ptr(), b.data_ptr()], [0, 0], []
    for k, t in enumerate((a, b)):
        for n, st in zip(t.shape, t.stride()):
            if n > 1 and st != 0:     # (a dimension of one element or of stride 0 adds no element)
                if st < 0:            # torch makes no such view today; one that did is still answered soundly
                    low[k] += (n - 1) * st * t.element_size()
                    st = -st
                reach[k] += (n - 1) * st
                found.append((st, k, n - 1))
    (pa, pb), ea, eb = low, a.element_size(), b.element_size()
    if pa + (reach[0] + 1) * ea <= pb or pb + (reach[1] + 1) * eb <= pa:
        return False                  # the bounding ranges are apart (views of two allocations always are)
    if ea != eb or (pa - pb) % ea:
        return True                   # elements of different width or on different grids: the bounding ranges are the answer
    steps = {}                        # stride -> [na - 1, nb - 1], summed over the dimensions that have it
    for st, k, m in found:
        steps.setdefault(st, [0, 0])[k] += m
    dims = sorted(steps.items(), reverse=True)
    below = [(0, 0)]                  # below[i]: lowest and highest sum the dimensions from i on can add
    for st, (na, nb) in reversed(dims):
        below.append((below[-1][0] - na * st, below[-1][1] + nb * st))
    below.reverse()
    todo, left = [((pa - pb) // ea, 0)], _OVERLAP_NODES
    while todo:
        delta, i = todo.pop()
        left -= 1
        if i == len(dims) or left < 0:           # (the last dimension leaves nothing but 0 below it)
            return True
        st, (na, nb) = dims[i]
        lo, hi = below[i + 1]
        todo += [(delta - d * st, i + 1) for d in range(max(-na, -((hi - delta) // st)), min(nb, (delta - lo) // st) + 1)]
    return False


def _self_overlap(t):
    """Whether two indices of a view may name one element: a stride of 0 on a dimension of more than one element
    (``expand``), or strides that are not nested (``as_strided``) -- no stride, smallest first, beyond the reach of the ones
    before it.  Never False when the view overlaps itself; a view cut from a contiguous buffer by slicing, indexing and
    permuting is nested and answered False."""
    if t.numel() == 0:
        return False
    reach = 0
    for st, n in sorted((abs(st), n) for n, st in zip(t.shape, t.stride()) if n > 1):
        if st <= reach:
            return True
        reach += (n - 1) * st
    return False


def _apart(what, name, t, apart):
    """The aliasing rule for one tensor ``t`` a call writes (None: nothing to check): it shares no element with itself nor
    with any tensor of ``apart`` -- what the call reads and whatever else it writes (None entries are skipped).  Every kernel
    takes its pointers ``__restrict__``, and most read a neighbourhood of what they store: a shared element is a wrong
    answer that depends on timing.  Called before anything is allocated or launched for the call."""
    if t is None:
        return
    if _self_overlap(t):
        raise ValueError(f"{what}: rows of {name} share memory with each other (strides {tuple(t.stride())} for shape "
                         f"{tuple(t.shape)})")
    if any(o is not None and _overlap(o, t) for o in apart):
        raise ValueError(f"{what}: {name} must not share memory with a tensor the call reads or another one it writes")


def _output(out, shape, device, what, longer=False, apart=()):
    """The destination of an entry that writes (R, C, L) = ``shape`` -> (out, its RowMap): a new float32 tensor when
    ``out`` is None, else the caller's (R, C, L) tensor or strided (B, n, C, L) view -- the same rows and channels, unit
    last stride, and the same length (``longer``: at least that length).  ``apart``: the tensors ``out`` must share no
    element with (:func:`_apart`); ``out`` may not overlap itself either.  A RowMap carries strides only: the library cannot
    see a short destination, so it is refused here, before any pointer is taken."""
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=device)
        return out, rowmap(out)[0]
    omap, R, C, L = rowmap(out)
    if (R, C) != tuple(shape[:2]) or (L < shape[2] if longer else L != shape[2]):
        raise ValueError(f"{what}: out {tuple(out.shape)} does not match rows={shape[0]}, channels={shape[1]}, "
                         f"length{'>=' if longer else '='}{shape[2]}")
    _apart(what, "out", out, apart)
    return out, omap


def _state(z, shape, what, name):
    """A carried state (``zi`` / ``zf``) of a stateful entry: None, or a contiguous float32 GPU tensor of exactly
    ``shape`` -- the kernels read and write it in place through plain pointers."""
    if z is None:
        return None
    if not isinstance(z, torch.Tensor) or not z.is_cuda or z.dtype != torch.float32 or tuple(z.shape) != tuple(shape) \
            or not z.is_contiguous():
        got = f"{tuple(z.shape)} {z.dtype} on {z.device}" if isinstance(z, torch.Tensor) else type(z).__name__
        raise ValueError(f"{what}: {name} must be a contiguous float32 GPU tensor of shape {tuple(shape)}, got {got}")
    return z


def _workspace(what, ws, nbytes, device, pin, apart, align=1):
    """The (pointer, byte count) pair of a launch's workspace.  Without ``ws``: what ``pin.workspace(nbytes, device)``
    makes.  A caller's ``ws`` is held to the aliasing rule against ``apart`` (:func:`_apart`: what the call reads and
    whatever else it writes), then to its form: contiguous uint8 on ``device``, at least ``nbytes`` of them, at an address
    that is a multiple of ``align`` -- the library answers a bare error code for a short or misaligned workspace, and
    takes a pointer to host memory as it comes.  Called where the workspace is made, the last thing before the launch: a
    refused ``ws`` has cost the call's own allocations, and none of its kernels has run."""
    if ws is None:
        return pin.workspace(nbytes, device)
    _apart(what, "ws", ws, apart)
    if ws.device != device or ws.dtype != torch.uint8 or not ws.is_contiguous() or ws.numel() < nbytes or ws.data_ptr() % align:
        aligned = f", {align}-byte aligned" if align > 1 else ""
        raise ValueError(f"{what}: the workspace must be {nbytes} contiguous uint8 on {device}{aligned}")
    return ws.data_ptr(), ws.numel()


def _int_in(what, name, v, lo, hi):
    """An integer argument that reaches the library as it is: an int (no bool, no float that happens to be whole) in
    ``lo`` .. ``hi``."""
    if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
        raise ValueError(f"{what}: {name}={v!r} must be an integer in {lo}..{hi}")


def _taps(what, name, h, max_taps):
    """Filter taps every row shares: a one-dimensional float32 tensor on the GPU of 1 .. ``max_taps`` values."""
    if not isinstance(h, torch.Tensor) or not h.is_cuda or h.dtype != torch.float32:
        raise TypeError(f"{what}: {name} must be a float32 tensor on the GPU")
    if h.ndim != 1 or not 1 <= h.numel() <= max_taps:
        raise ValueError(f"{what}: {name} must hold 1..{max_taps} taps in one dimension, got {tuple(h.shape)}")


def _want(what, want, known, some=False):
    """The gradients a backward entry is asked for are some of the ones it knows (``some``: and at least one)."""
    unknown = set(want) - set(known)
    if unknown:
        raise ValueError(f"{what}: unknown gradients {sorted(unknown)} (known: {known})")
    if some and not want:
        raise ValueError(f"{what}: no gradient asked for")


def _cotangent(what, gy, x, shape):
    """The cotangent ``gy`` of a backward entry has the (R, C, L) = ``shape`` of the signal ``x`` -> its RowMap."""
    gmap, *got = rowmap(gy)
    if tuple(got) != tuple(shape):
        raise ValueError(f"{what}: gradient {tuple(gy.shape)} does not match the input {tuple(x.shape)}")
    return gmap


def _signal_grad(what, want, out, shape, xmap, device, apart):
    """Where a backward entry writes the signal gradient -> (gx, its RowMap).  Without "x" in ``want`` the entry writes no
    signal gradient (and takes any row map): (None, ``xmap``, the input's).  Else ``out`` or a new tensor, as
    :func:`_output` makes it.  A given ``out`` is checked whether or not it is used; ``apart``: everything the call reads
    and its ``ws``."""
    if "x" not in want and out is None:
        return None, xmap
    dest = _output(out, shape, device, what, apart=apart)
    return dest if "x" in want else (None, xmap)


def _param_grads(want, shapes, device):
    """The parameter gradients of a backward entry, in the order of ``shapes`` = {name: shape}: a new float32 tensor for a
    name in ``want``, None for the others (the entry takes a null pointer for a gradient nobody asked for)."""
    return [torch.empty(shape, dtype=torch.float32, device=device) if name in want else None for name, shape in shapes.items()]


def _pair_state(what, state, shape, second, read_second):
    """The two parts of a stateful entry's ``state`` = (history, ``second``) -> (history, second part), both None without
    a state.  The history is a :func:`_state` of ``shape``; ``read_second`` checks the other part and returns it."""
    if state is None:
        return None, None
    if not isinstance(state, (tuple, list)) or len(state) != 2:
        raise ValueError(f"{what}: state must be the pair (history, {second})")
    zi, other = _state(state[0], shape, what, "the state's history"), read_second(state[1])
    if zi is None or other is None:
        raise ValueError(f"{what}: state must be the pair (history, {second})")
    return zi, other


def _row_chunks(rows, limit):
    """(first row, count) of the launches that take ``rows`` rows ``limit`` at a time (rows ride on a grid dimension)."""
    return ((i, min(limit, rows - i)) for i in range(0, rows, limit))
