"""In-place signal-buffer I/O protocol between render_grafx and the HIP processors.

``render_into(x4, out4, **params)`` receives strided (B, n, C, L) views of the render loop's
signal buffer (input slice, destination slice) and per-row parameters flattened batch-major
(B*n, ...), exactly the rows ``forward`` would get.  Processors whose kernels address rows
through a gfx_rowmap_t read and write the buffer directly; the default falls back to
``forward`` on a flattened copy.

``prepare(**params[, _shared_rows]) -> Prepared | None`` (optional): the parameter-only part of ``render_into``
(filter design, impulse-response synthesis, spectra).  The render loop runs it ahead of time on a side stream,
under the signal kernels of the earlier stages, and hands the result back as ``render_into(..., _prepared=...)``.

``stream_block(x4, out4, carry, **params) -> carry`` (every processor class): one block of a streamed render.  It writes
the block's output into ``out4`` like ``render_into`` and returns what the next block's call needs in ``carry`` -- whatever
the processor's own keywords call it (``state=``, ``history=``), None for a memoryless processor and for the first block.
``stream_check()`` raises the processor's own ValueError when its configuration cannot be rendered in blocks; the render
asks every stage before it launches the first.
``stream_silence(carry) -> carry`` takes a carry this processor returned and gives back, in new tensors of the same
shapes, the carry that means "nothing came before": what a first block's None stands for, materialised, so that a stream
can start on the kernels every later block runs (render.silent_state, render.CapturedStream)."""
import torch
import torch.nn.functional as F

from ...autograd import needs_grad


class Prepared:
    """What ``prepare`` returns: device tensors (so the render can order their lifetime across streams) + scalars."""

    def __init__(self, *tensors, **scalars):
        self.tensors = tensors
        self.__dict__.update(scalars)


def write_rows(out4, y):
    """A processor's (R, C, L) / (B, n, C, L) result (or ``(result, by-products)``) into the (B, n, C, L) destination view."""
    y = y[0] if isinstance(y, tuple) else y
    if y.data_ptr() != out4.data_ptr():
        out4.copy_(y.reshape(out4.shape))
    return out4


def map_carry(fn, carry):
    """``fn`` on every tensor leaf of a carry (None, a tensor, or a tuple / list of carries) -> a carry of the same form."""
    if carry is None:
        return None
    if isinstance(carry, torch.Tensor):
        return fn(carry)
    return type(carry)(map_carry(fn, c) for c in carry)


def carry_leaves(carry):
    """The tensor leaves of a carry, in order."""
    if carry is None:
        return []
    if isinstance(carry, torch.Tensor):
        return [carry]
    return [leaf for c in carry for leaf in carry_leaves(c)]


def child_stream(proc, owner):
    """The wrapped processor of a container, which must speak the block protocol itself."""
    if not hasattr(proc, "stream_block"):
        raise ValueError(f"{type(owner).__name__}: the wrapped {type(proc).__name__} has no stream_block()")
    return proc


class StreamIO:
    """The block protocol of a processor without memory: the block is rendered like any signal, nothing is carried."""

    def stream_check(self):
        """Raises ValueError, with the reason, when this configuration cannot be rendered in blocks."""

    def stream_block(self, x4, out4, carry, _shared_rows=None, **params):
        self.stream_check()
        if hasattr(self, "render_into"):
            extra = {} if _shared_rows is None else {"_shared_rows": _shared_rows}
            self.render_into(x4, out4, **extra, **params)
        else:
            if _shared_rows is not None:
                params = {k: expand_shared(v, shared_reps(x4, _shared_rows)) for k, v in params.items()}
            write_rows(out4, self.forward(x4.reshape(-1, *x4.shape[2:]), **params))
        return None

    def stream_silence(self, carry):
        """Histories and filter states start from zero (a processor whose None means something else overrides this)."""
        return map_carry(torch.zeros_like, carry)


class BufferIO(StreamIO):
    def render_into(self, x4, out4, **params):
        y = self.forward(x4.reshape(-1, *x4.shape[2:]), **params)
        out4.copy_(y.view(out4.shape))
        return out4


class FusedIO(BufferIO):
    """A module on one fused op whose ``forward`` takes the strided views themselves and a destination ``_out``: the op
    writes the buffer in place.  Under grad the autograd node makes its own output, and the rows are written from it."""

    def render_into(self, x4, out4, **params):
        if needs_grad(x4, *params.values()):
            return write_rows(out4, self.forward(x4, **params))
        return self.forward(x4, _out=out4, **params)


class FusedStateIO(FusedIO):
    """A FusedIO module with memory in every configuration: the carry is the state of ``forward(state=)``."""

    def stream_block(self, x4, out4, carry, **params):
        return self.forward(x4, _out=out4, state=carry, return_state=True, **params)[1]


def history_after(x, S):
    """The input history a first block leaves: the last ``S`` samples of ``x`` behind zeros -> contiguous (R, C, S), off
    the tape."""
    C, L = x.shape[-2:]
    xr = x.detach().reshape(-1, C, L)
    return F.pad(xr[..., max(0, L - S):], (max(0, S - L), 0)).contiguous()


def refuse_state_under_grad(name, state):
    """The fused ops' backward entries start from silence: a block that enters with a state cannot be trained through."""
    if state is not None:
        raise ValueError(f"{name}: a block that enters with a state has no native backward; train on whole signals")


def shared_reps(x, shared_rows):
    """How many times `shared_rows` parameter rows repeat over the rows of x ((R,C,L) or a (B,n,C,L) view)."""
    rows = x.shape[0] * x.shape[1] if x.ndim == 4 else x.shape[0]
    if rows % shared_rows != 0:
        raise ValueError(f"{rows} signal rows cannot share {shared_rows} parameter rows")
    return rows // shared_rows


def expand_shared(t, reps):
    """(n, ...) per-node parameter -> (reps*n, ...) batch-major rows (what upstream's expand + flatten produces)."""
    return None if t is None else t.repeat(reps, *([1] * (t.ndim - 1)))
