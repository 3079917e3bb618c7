"""A whole render as ONE HIP graph (inference / serving).

``render_grafx`` is a Python loop that launches ~45 kernels on up to three streams.  At serving sizes (one or a few
graphs per call) the GPU finishes each of them in microseconds and the call is bound by the host: interpreter, ctypes
and launch overhead.  Capturing the loop once and replaying it removes all of that; the kernels, their order, the
side-stream overlap and the results are exactly those of the eager call (bit-identical).

    fast = CapturedRender(processors, example_input, parameters, render_data)
    y, _, buf = fast(new_input)              # or fast(new_input, new_parameters)

Inputs are copied into the static tensors the graph was captured on; the outputs are static too (valid until the next
call).  Shapes, devices and the render data are fixed at capture time.  No autograd.

A streamed render -- ``render_grafx(state=, return_state=True)``, one block after the other -- replays the same way:

    stream = CapturedStream(processors, example_block, parameters, render_data)
    for block in blocks:
        y, _, buf = stream(block)            # bit-identical to the eager blocks from silent_state(...)

see :class:`CapturedStream`.
"""
import torch

from ..processors.core._buffer_io import carry_leaves, map_carry
from .graph import render_grafx
from .stream import RenderState, _design_stream, _render_stream, _stream_admit, silent_state


def _clone_tree(tree):
    if isinstance(tree, torch.Tensor):
        return tree.detach().clone()
    if hasattr(tree, "items"):
        return {k: _clone_tree(v) for k, v in tree.items()}
    return tree


def _copy_tree(dst, src):
    if isinstance(dst, torch.Tensor):
        dst.copy_(src)
    elif hasattr(dst, "items"):
        for k in dst:
            _copy_tree(dst[k], src[k])


class CapturedRender:
    def __init__(self, processors, input_signals, per_type_parameters, render_data, common_parameters=None, warmup=2):
        if not input_signals.is_cuda:
            raise ValueError("CapturedRender needs the HIP path (CUDA/HIP input tensors)")
        self.input_signals = input_signals.detach().clone()
        self.parameters = _clone_tree(per_type_parameters)
        self.common_parameters = None if common_parameters is None else _clone_tree(common_parameters)
        args = (processors, self.input_signals, self.parameters, render_data, self.common_parameters)
        current = torch.cuda.current_stream(input_signals.device)
        stream = torch.cuda.Stream(device=input_signals.device)
        stream.wait_stream(current)
        with torch.cuda.stream(stream), torch.no_grad():
            for _ in range(warmup):  # code objects, per-device tables, allocator pools: everything lazy happens here
                render_grafx(*args, parameters_grad=False)
        current.wait_stream(stream)
        torch.cuda.synchronize(input_signals.device)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph), torch.no_grad():
            self.outputs = render_grafx(*args, parameters_grad=False)

    def __call__(self, input_signals=None, per_type_parameters=None, common_parameters=None):
        if input_signals is not None:
            self.input_signals.copy_(input_signals)
        if per_type_parameters is not None:
            _copy_tree(self.parameters, per_type_parameters)
        if common_parameters is not None:
            _copy_tree(self.common_parameters, common_parameters)
        self.graph.replay()
        return self.outputs


class CapturedStream:
    """A streamed render, block by block, as a captured HIP graph: every call renders the next block of the stream.

    The eager streamed render is a Python loop of ~45 launches per block that allocates its buffer and carries anew and
    designs every filter on every block; at serving sizes it is bound by the host.  Here the block length, batch, channels
    and render data are fixed at construction, inputs and parameters are copied into static tensors, and the state lives
    in static carry tensors that start from ``state`` (a RenderState of an eager stream) or from silence, materialised
    (``silent_state``: a captured graph is one fixed kernel list, so the first block runs the kernels of every later one).
    Two graphs, each a linear chain captured on one stream:

    * the *design graph*: the parameter-only work of every step whose processor hands back a ``Prepared`` from
      ``prepare()`` (the "fsm" equaliser's coefficients, taps and spectra; the reverb's impulse response and spectra).  It
      runs at construction and in :meth:`update_parameters`, never per block; ``designed`` lists those steps.
    * the *block graph*: one ``_render_stream`` block reading the static carries, with the designs above handed in and
      everything else designed inline, followed by a copy of every carry the block produced back into the static ones
      (the stateful kernels do not take overlapping zi / zf: the hand-over is a copy).

    Bit-identical to the eager blocks rendered from ``silent_state(...)`` (the same kernels on the same arguments).
    Everything ``render_grafx(state=)`` refuses is refused here with the same message, before anything is captured.

        y, _, buf = stream(block)            # valid until the next call; buf is None with keep_signal_buffer=False
        stream.update_parameters(p)          # takes effect at the next block; histories and envelopes carry on
        stream.reset()                       # back to silence
        s = stream.state()                   # a RenderState of clones: an eager render_grafx(state=s) continues the stream
        stream.load_state(s)                 # ... and back (copied in; s is not changed)"""

    def __init__(self, processors, example_block, per_type_parameters, render_data, common_parameters=None,
                 keep_signal_buffer=True, state=None, warmup=2):
        if not example_block.is_cuda:
            raise ValueError("CapturedStream needs the HIP path (CUDA/HIP input tensors)")
        # asked of the caller's own tensors (the static clones below never require grad)
        _stream_admit(processors, example_block, per_type_parameters, render_data, common_parameters, state)
        self.input_signals = example_block.detach().clone()
        self.parameters = _clone_tree(per_type_parameters)
        self.common_parameters = None if common_parameters is None else _clone_tree(common_parameters)
        args = (processors, self.input_signals, self.parameters, render_data, self.common_parameters)
        self._args = args
        self.samples = 0
        device = example_block.device
        current = torch.cuda.current_stream(device)
        self._stream = torch.cuda.Stream(device=device)      # both graphs are captured on this one stream
        self._stream.wait_stream(current)
        with torch.cuda.stream(self._stream), torch.no_grad():
            self._silence = silent_state(*args)              # (its eager block also builds the cached routing plans)
            self._like = self._silence                       # batch, channels, device, steps of this stream
            self._carries = {i: map_carry(torch.clone, c) for i, c in self._silence.carries.items()}
            if state is not None:
                self.load_state(state)
            # from the materialised state, so that the warm-up launches the kernels of the capture: code objects,
            # per-device tables, allocator pools, the routing plans of this keep_signal_buffer -- everything lazy
            for _ in range(max(1, warmup)):
                designs = _design_stream(*args)
                _render_stream(*args, self._state_in(), keep_signal_buffer, prepared=designs)
        current.wait_stream(self._stream)
        torch.cuda.synchronize(device)
        self.designed = tuple(sorted(designs))
        self.design_graph, self._prepared = None, {}
        if self.designed:
            self.design_graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(self.design_graph, stream=self._stream), torch.no_grad():
                self._prepared = _design_stream(*args)       # its tensors stay with the object: the block graph reads them
            self.design_graph.replay()
        self.block_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.block_graph, stream=self._stream), torch.no_grad():
            y, intermediates, buf, after = _render_stream(*args, self._state_in(), keep_signal_buffer, prepared=self._prepared)
            for i, carry in after.carries.items():
                for dst, src in zip(carry_leaves(self._carries[i]), carry_leaves(carry), strict=True):
                    dst.copy_(src)
        self.outputs = (y, intermediates, buf)

    def _state_in(self):
        return self._like.advanced(self._carries, 0)

    def __call__(self, block):
        if tuple(block.shape) != tuple(self.input_signals.shape):
            raise ValueError(f"CapturedStream: captured for blocks of shape {tuple(self.input_signals.shape)}, got "
                             f"{tuple(block.shape)} (the block length, batch and channels are fixed at construction)")
        self.input_signals.copy_(block)
        self.block_graph.replay()
        self.samples += block.shape[-1]
        return self.outputs

    def update_parameters(self, per_type_parameters=None, common_parameters=None):
        """New parameters from the next block on (None: as they are), and the hoisted designs redone for them."""
        if per_type_parameters is not None:
            _copy_tree(self.parameters, per_type_parameters)
        if common_parameters is not None:
            _copy_tree(self.common_parameters, common_parameters)
        if self.design_graph is not None:
            self.design_graph.replay()

    def reset(self):
        """Back to silence: the next block is the first of a new stream."""
        self._load(self._silence.carries)
        self.samples = 0

    def state(self):
        """The stream so far as a RenderState of its own tensors (clones)."""
        return self._like.advanced({i: map_carry(torch.clone, c) for i, c in self._carries.items()}, self.samples)

    def load_state(self, state):
        """Continue from ``state``, a RenderState of a stream of this shape (eager or captured); it is copied, never changed."""
        if not isinstance(state, RenderState):
            raise ValueError(f"CapturedStream: state must be a RenderState, got {type(state).__name__}")
        why = state.mismatch(self._like.batch, self._like.channels, self._like.device, self._like.steps)
        if why is not None:
            raise ValueError(f"CapturedStream: {why}")
        # (a step without a carry in ``state`` -- a RenderState nothing has been rendered from -- starts from silence)
        carries = {i: self._silence.carries[i] if state.carries.get(i) is None else state.carries[i] for i in self._carries}
        for i, mine in self._carries.items():
            want, got = [tuple(t.shape) for t in carry_leaves(mine)], [tuple(t.shape) for t in carry_leaves(carries[i])]
            if want != got:
                raise ValueError(f"CapturedStream: the carry of render step {i} has leaves of shape {got}, this stream's "
                                 f"has {want}")
        self._load(carries)
        self.samples = state.samples

    def _load(self, carries):
        for i, mine in self._carries.items():
            for dst, src in zip(carry_leaves(mine), carry_leaves(carries[i])):
                dst.copy_(src)
