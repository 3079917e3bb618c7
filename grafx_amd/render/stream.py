"""Streaming: the in-place buffer render one block at a time, with what every processor carries from block to block."""
import torch

from .backward import _wants_grad
from .forward import _buffer_io_reason
from .plans import _gather_plan
from .stage import StageArguments, stage_input


class RenderState:
    """What a render of one block leaves for the render of the next (``render_grafx(..., state=, return_state=True)``).

    Opaque to the caller.  It holds one carry per render STEP -- keyed by the step's index in ``render_data.iter_list``, in
    whatever form that step's processor hands it back (``stream_block``) -- so a node type whose nodes are spread over
    several steps keeps one carry per step and nothing is sliced or re-assembled between blocks.  It also records what it
    was made for (batch size -- None for an unbatched 3-D render --, channels, device, every step's node type and row
    count) and ``samples``, the number of samples rendered so far.  A render never changes the state it is given: it
    returns a new one."""

    __slots__ = ("batch", "channels", "device", "steps", "carries", "samples")

    def __init__(self, batch, channels, device, steps, carries=None, samples=0):
        self.batch, self.channels, self.device = batch, channels, torch.device(device)
        self.steps = tuple((str(t), int(n)) for t, n in steps)
        self.carries = dict(carries or {})
        self.samples = int(samples)
        if any(not 1 <= i <= len(self.steps) for i in self.carries):
            raise ValueError(f"RenderState: a carry for a step outside 1..{len(self.steps)}")

    @staticmethod
    def steps_of(render_data):
        """(node type, rows written) of every render step after the sources."""
        steps = []
        for step in render_data.iter_list[1 : render_data.max_order + 1]:
            d0, d1 = step.dest_write.idx
            steps.append((step.node_type, d1 - d0))
        return tuple(steps)

    def mismatch(self, batch, channels, device, steps):
        """Why this state does not belong to a render of that shape (None: it does)."""
        if self.batch != batch:
            say = lambda b: "an unbatched render" if b is None else f"batch size {b}"   # noqa: E731
            return f"the state was made for {say(self.batch)}, this render has {say(batch)}"
        if self.channels != channels:
            return f"the state was made for {self.channels} channels, this render has {channels}"
        if self.device != torch.device(device):
            return f"the state lives on device {self.device}, this render runs on {torch.device(device)}"
        steps = tuple((str(t), int(n)) for t, n in steps)
        if len(self.steps) != len(steps):
            return f"the state was made for a render of {len(self.steps)} steps, this render_data has {len(steps)}"
        for i, (mine, theirs) in enumerate(zip(self.steps, steps), 1):
            if mine != theirs:
                return (f"render step {i} of the state is {mine[1]} rows of node type {mine[0]!r}, this render_data has "
                        f"{theirs[1]} rows of {theirs[0]!r} there")
        return None

    def advanced(self, carries, samples):
        """The state after one more block of ``samples`` samples that left ``carries``."""
        return RenderState(self.batch, self.channels, self.device, self.steps, carries, self.samples + samples)

    def __repr__(self):
        return (f"RenderState(batch={self.batch}, channels={self.channels}, device={str(self.device)!r}, "
                f"steps={len(self.steps)}, samples={self.samples})")


def _stream_admit(processors, input_signals, per_type_parameters, render_data, common_parameters, state):
    """Everything a streamed render refuses, asked before the first launch (so a refusal leaves no half-written buffer and
    no half-advanced state) -> the state to render from (a fresh one for None)."""
    if input_signals.ndim not in (3, 4):
        raise Exception(f"input_signal has shape of {input_signals.shape} ({input_signals.ndim} ndims), which is not 3 or 4 dims.")
    reason = _buffer_io_reason(processors, input_signals, render_data, method="stream_block")
    if reason is not None:
        raise ValueError(f"render_grafx: a render with a state runs on the in-place buffer path, which this one cannot take "
                         f"because {reason}")
    if _wants_grad(input_signals, per_type_parameters, common_parameters):
        raise NotImplementedError("render_grafx: a render with a state does not carry gradients (a parameter or the input "
                                  "requires grad); back-propagation through a streamed graph is not implemented -- render "
                                  "under torch.no_grad(), or without state / return_state")
    squeeze = input_signals.ndim == 3
    B, C = (None if squeeze else input_signals.shape[0]), input_signals.shape[-2]
    steps = RenderState.steps_of(render_data)
    if state is None:
        state = RenderState(B, C, input_signals.device, steps)
    elif not isinstance(state, RenderState):
        raise ValueError(f"render_grafx: state must be a RenderState from an earlier block, got {type(state).__name__}")
    else:
        why = state.mismatch(B, C, input_signals.device, steps)
        if why is not None:
            raise ValueError(f"render_grafx: {why}")
    for i in range(1, render_data.max_order + 1):
        node_type = render_data.iter_list[i].node_type
        if node_type in processors:
            try:
                processors[node_type].stream_check()
            except ValueError as err:
                raise ValueError(f"render_grafx: node type {node_type!r} cannot be rendered in blocks: {err}") from None
    return state



def _design_stream(processors, input_signals, per_type_parameters, render_data, common_parameters):
    """The parameter-only work of a streamed render, apart from its blocks: {step: Prepared} for every step whose processor
    offers ``prepare()`` and returns a Prepared for these parameters -- what ``_render_stream(prepared=)`` takes."""
    squeeze = input_signals.ndim == 3
    stage_arguments = StageArguments(processors, render_data, per_type_parameters, common_parameters, squeeze,
                                     1 if squeeze else input_signals.shape[0])
    prepared = {}
    for i in range(1, render_data.max_order + 1):
        proc = processors[render_data.iter_list[i].node_type] if render_data.iter_list[i].node_type in processors else None
        if hasattr(proc, "prepare"):
            extra, params, common_i = stage_arguments(i)
            design = proc.prepare(**extra, **params, **common_i)
            if design is not None:
                prepared[i] = design
    return prepared


def _render_stream(processors, input_signals, per_type_parameters, render_data, common_parameters, state,
                   keep_signal_buffer, prepared=None):
    """One block of a streamed render: the in-place buffer render with every stage called through ``stream_block``.
    No mix fusion, no tee and no side streams (none of them takes a carry): a routing sum is its own gather-sum, every
    stage designs its filters right before it runs -- except the steps of ``prepared`` ({step: Prepared}, _design_stream),
    which take their design from there."""
    from .. import ops

    state = _stream_admit(processors, input_signals, per_type_parameters, render_data, common_parameters, state)
    squeeze = input_signals.ndim == 3
    x = input_signals.unsqueeze(0) if squeeze else input_signals
    B, n_src, C, L = x.shape
    dev = x.device
    stage_arguments = StageArguments(processors, render_data, per_type_parameters, common_parameters, squeeze, B)

    buf = torch.empty(B, render_data.num_nodes, C, L, device=dev)
    sources_in_buf = False

    def need_sources():
        nonlocal sources_in_buf
        if not sources_in_buf:
            buf[:, :n_src].copy_(x)
            sources_in_buf = True

    if keep_signal_buffer:    # (an output-only render copies the sources only when a stage reads them from the buffer)
        need_sources()
    carries = {}
    out_view = None
    for i in range(1, render_data.max_order + 1):
        step = render_data.iter_list[i]
        d0, d1 = step.dest_write.idx
        out_view = buf.narrow(1, d0, d1 - d0)
        plan = _gather_plan(step, dev)
        node_type = step.node_type
        routing = node_type not in processors  # in / out / mix: the (summed) input is the output
        where, x_view = stage_input(ops, step, plan, x, buf, n_src, out_view if routing else None, need_sources)
        if routing:
            if where != "gather":
                out_view.copy_(x_view)
            continue
        extra, params, common_i = stage_arguments(i)
        if prepared is not None and i in prepared:
            extra["_prepared"] = prepared[i]
        carries[i] = processors[node_type].stream_block(x_view, out_view, state.carries.get(i), **extra, **params, **common_i)
    kept = (buf[0] if squeeze else buf) if keep_signal_buffer else None
    return (out_view[0] if squeeze else out_view), [], kept, state.advanced(carries, L)


def silent_state(processors, input_signals, per_type_parameters, render_data, common_parameters=None):
    """The :class:`RenderState` that means "nothing came before", materialised: every carry a render of blocks shaped like
    ``input_signals`` hands on, filled with what its processor calls silence (``stream_silence``: zero histories and filter
    states, envelopes at 1).  A render from it computes what a render from ``state=None`` computes, on the kernels every
    later block runs (a None carry takes the stateless ones) -- which is what lets one fixed kernel list serve the whole
    stream (CapturedStream).  Learns the carries' shapes from one eager block rendered from ``state=None``, and so makes
    the refusals of ``render_grafx(state=)``; ``.samples`` is 0."""
    state = _render_stream(processors, input_signals, per_type_parameters, render_data, common_parameters, None, False)[3]
    carries = {}
    for i, carry in state.carries.items():
        proc = processors[render_data.iter_list[i].node_type]
        if not hasattr(proc, "stream_silence"):
            raise ValueError(f"silent_state: processor type {render_data.iter_list[i].node_type!r} ({type(proc).__name__}) "
                             "has no stream_silence()")
        carries[i] = proc.stream_silence(carry)
    return RenderState(state.batch, state.channels, state.device, state.steps, carries, 0)
