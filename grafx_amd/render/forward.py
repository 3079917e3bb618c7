"""The in-place buffer render (inference, and the forward of the training render): every stage reads and writes the
(B, V, C, L) signal buffer where it is, routing sums run as one gather-sum kernel or inside the kernel of the stage in
front of them, and the parameter-only work of the later stages runs on a side stream underneath the first ones."""
import warnings

import torch

from ..data.configs import UTILITY_TYPES
from .plans import _gather_plan, _mix_schedule, _reads_rows
from .stage import StageArguments, stage_input

# Training forward: keep the dynamics stages' smoother scan (R x L floats per stage) for their backward.  Rounds 2-5 kept it
# (the alternative was a pass of its own over every row); since round 6 the backward tiles rebuild the scan from the
# samples they read anyway (gfx_dynamics_bwd_f32 with a scratch u1), which takes 4 bytes per sample out of the forward AND the
# backward kernel and 4.8 GB at 256 graphs out of the step's peak: off by default (True: round 5's path).
KEEP_SMOOTHER_SCAN = False
# Where the parameter-only work of the later stages (filter design, the reverb's impulse response and spectra) runs:
#   "under_first"   on a side stream underneath the first processor stage's signal kernel (the convolution of the first
#                   equaliser stage in a console: compute-bound, the side kernels take CUs from it);
#   "under_second"  underneath the second processor stage (the compressors in a console: memory-bound, idle ALUs);
#   "inline"        no side stream: every stage designs its own filters on the main stream right before it runs.
# Measured on the headline graph: profiles/r4/prepare_stream_ab.md.
PREPARE_MODE = "under_first"


class GenericRenderPathWarning(UserWarning):
    """A render of CUDA signals that does not take the in-place buffer path (see _buffer_io_reason)."""


def _buffer_io_reason(processors, input_signals, render_data, method="render_into"):
    """None when the render can take the in-place buffer path (gradients are handled by _BufferRenderFn around it), else
    what keeps it off: the render then runs upstream's loop (render/graph.py:104-175 of the reference: copies on read,
    torch routing, one processor call per stage -- the processors themselves still run their HIP kernels).
    ``method``: what every processor must offer (the streamed render asks for ``stream_block``)."""
    if not input_signals.is_cuda:
        return "the signals are not on a GPU"
    if render_data.method == "one-by-one":
        return "the schedule is 'one-by-one' (no type batching)"
    if not render_data.siso_only:
        return "the graph holds multi-input / multi-output processors (render/prepare.py:109-192 of the reference)"
    for step in render_data.iter_list[1:]:
        if step.node_type in processors:
            if not hasattr(processors[step.node_type], method):
                return f"processor type {step.node_type!r} ({type(processors[step.node_type]).__name__}) has no {method}()"
        elif step.node_type not in UTILITY_TYPES:
            return f"node type {step.node_type!r} has no processor"
        if step.dest_write.method != "slice" or len(step.source_reads) != 1 or step.source_reads[0].method == "none":
            return f"stage {step.node_type!r} does not read one input and write a contiguous range of rows"
        if _gather_plan(step, input_signals.device) is False:
            return f"stage {step.node_type!r} aggregates through an unsorted scatter"
    return None


def _buffer_io_ok(processors, input_signals, render_data):
    """Structural conditions of the in-place buffer path."""
    reason = _buffer_io_reason(processors, input_signals, render_data)
    if reason is not None and input_signals.is_cuda:
        # not silent: a CUDA render off the fast path says so (once per reason and call site)
        warnings.warn(f"render_grafx: taking the generic loop instead of the in-place buffer render because {reason}",
                      GenericRenderPathWarning, stacklevel=3)
    return reason is None


_AUX_STREAMS = {}


def _aux_stream(device, name):
    """The render's side stream `name` ("copy" of the sources into the buffer, "prepare" of the later stages), made once."""
    key = (device.type, device.index, name)
    if key not in _AUX_STREAMS:
        _AUX_STREAMS[key] = torch.cuda.Stream(device=device)
    return _AUX_STREAMS[key]


def _tee_range(render_data, processors, n_src, device):
    """Source rows [a, b) that the first stage reads as a plain slice through a tee-capable processor, or None."""
    if render_data.max_order < 1:
        return None
    step = render_data.iter_list[1]
    read = step.source_reads[0]
    proc = processors[step.node_type] if step.node_type in processors else None
    if proc is None or not getattr(proc, "accepts_tee", False):
        return None
    if read.method != "slice" or read.idx[1] > n_src or _gather_plan(step, device) is not None:
        return None
    return tuple(read.idx)


def _complement(rng, n):
    if rng is None:
        return [(0, n)]
    a, b = rng
    return [(lo, hi) for lo, hi in ((0, a), (b, n)) if hi > lo]


def _mix_safe_types():
    """Exact processor classes whose render_into(..., _mix=) writes exactly the stage's output rows and their sums (a user
    subclass may post-process them: it gets the two stages one after the other)."""
    from .. import processors as P

    return (P.Compressor, P.NoiseGate, P.StereoGain)


def _mix_candidate(processors, render_data, i, done, device):
    """The routing-sum stage that stage i may produce itself, and the stages to run before stage i for that:
    the stage right behind it -- or the one behind ONE processor stage that does not read stage i's rows (the
    console: the bus compressors, then the reverb, then the master sum of both), which then runs first."""
    steps, last = render_data.iter_list, render_data.max_order
    step = steps[i]
    proc = processors[step.node_type]
    if not (getattr(proc, "accepts_mix", False) and type(proc) in _mix_safe_types()):
        return None, []
    first = []
    j = i + 1
    if j <= last and steps[j].node_type in processors and j not in done:
        if _reads_rows(steps[j], *step.dest_write.idx):
            return None, []
        first, j = [j], j + 1
    if j > last or steps[j].node_type in processors:
        return None, []
    sched = _mix_schedule(step, steps[j], device)
    if sched is None:
        return None, []
    if first:
        f0, f1 = steps[first[0]].dest_write.idx
        if not any(f0 <= r < f1 for r in sched["extra_rows"]):
            return None, []      # the sum does not need the stage in between: keep the schedule's order
    rows_ready = lambda r: r < step.dest_write.idx[0] or any(  # noqa: E731
        steps[f].dest_write.idx[0] <= r < steps[f].dest_write.idx[1] for f in first)
    if not all(rows_ready(r) for r in sched["extra_rows"]):
        return None, []
    return j, first


def _prepare_later_stages(processors, render_data, stage_arguments, after, main):
    """Parameter-only work of the stages after `after` (filter design, impulse responses, spectra) on a side
    stream, under the signal kernels of the earlier stages; -> {order: (Prepared, event)}."""
    steps = render_data.iter_list
    todo = [j for j in range(after + 1, render_data.max_order + 1)
            if hasattr(processors[steps[j].node_type] if steps[j].node_type in processors else None, "prepare")]
    if not todo:
        return {}
    # parameter views (and, where a processor needs them, the batch-expanded copies) are made on the main stream
    args = {j: stage_arguments(j) for j in todo}
    prep = _aux_stream(main.device, "prepare")
    prep.wait_stream(main)  # the parameters may have been produced on the caller's stream
    ready = {}
    with torch.cuda.stream(prep):
        for j in todo:
            extra_j, params_j, common_j = args[j]
            state = processors[steps[j].node_type].prepare(**extra_j, **params_j, **common_j)
            if state is None:
                continue
            for tns in state.tensors:  # allocated on the side stream, read on the main one
                tns.record_stream(main)
            event = torch.cuda.Event()
            event.record(prep)
            ready[j] = (state, event)
    return ready


def _render_buffer_io(processors, input_signals, per_type_parameters, render_data, common_parameters, aux=None,
                      keep_signal_buffer=True):
    """render_grafx for HIP processors: every stage reads and writes the (B, V, C, L) signal buffer in place
    (no clone / index_select / reshape copies), routing sums run as one gather-sum kernel.
    ``keep_signal_buffer=False`` (an output-only render; the third return value is None): rows that nothing reads are
    not written -- the sources are not copied into the buffer unless a stage reads them from there, and a stage whose
    rows only feed the routing sum fused into its kernel does not store them.
    ``aux``: a dict (training path) in which processors with ``accepts_aux`` keep per-stage by-products of the forward
    pass that their backward needs (key: the stage's order); the stage-wise backward hands it back to them."""
    from .. import ops
    from .backward import _tape_safe_types

    squeeze = input_signals.ndim == 3
    x = input_signals.unsqueeze(0) if squeeze else input_signals
    B, n_src, C, L = x.shape
    stage_arguments = StageArguments(processors, render_data, per_type_parameters, common_parameters, squeeze, B)

    buf = torch.empty(B, render_data.num_nodes, C, L, device=x.device)
    # The sources must end up in the buffer's first slots (the buffer is returned with every node's signal),
    # but nothing has to wait for that copy: stages that read source rows read them from `x` itself, and the
    # copy runs on a side stream underneath the first (compute-bound) stages.
    # ... and a stage whose processor can "tee" (write its input through to a second destination from the
    # registers that hold it anyway) makes the copy of the rows it reads free.
    lean = not keep_signal_buffer
    teed = None if lean else _tee_range(render_data, processors, n_src, x.device)
    main = torch.cuda.current_stream(x.device)
    rest = [] if lean else _complement(teed, n_src)
    sources_in_buf = not lean          # lean: copied on demand (need_sources), on the main stream
    side = _aux_stream(x.device, "copy") if rest else None
    if side is not None:
        side.wait_stream(main)
        with torch.cuda.stream(side):
            for a, b in rest:
                buf[:, a:b].copy_(x[:, a:b], non_blocking=True)
        # No record_stream() on x / buf: the main stream joins the side stream before this function returns, so
        # everything the caller (or the allocator, on reuse) does with them afterwards is ordered behind the copy.
        # record_stream would instead make the caching allocator hold the 30 GB buffer back until it has *observed*
        # the side stream's event; with the host running a few steps ahead it then cannot recycle the buffer and
        # falls back to a fresh hipMalloc per step (seen as intermittent 150-800 ms steps).
    copied = False  # has the main stream joined the copy yet?
    prepared = None
    launched = 0  # processor stages launched so far
    done = set()  # stages already produced out of schedule order (see below)

    def need_sources():
        """A stage is about to read source rows from the buffer: join the side stream's copy (lean: make it now)."""
        nonlocal copied, sources_in_buf
        if side is not None and not copied:
            main.wait_stream(side)
            copied = True
        if not sources_in_buf:
            buf[:, :n_src].copy_(x)
            sources_in_buf = True

    def run_stage(i, mix_with=None):
        """Stage i; `mix_with`: the routing-sum stage the processor is offered to produce too -> did it?"""
        nonlocal prepared, launched
        step = render_data.iter_list[i]
        d0, d1 = step.dest_write.idx
        out_v = buf.narrow(1, d0, d1 - d0)
        plan = _gather_plan(step, x.device)
        node_type = step.node_type
        routing = node_type not in processors  # in / out / mix: the (summed) input is the output
        where, x_view = stage_input(ops, step, plan, x, buf, n_src, out_v if routing else None, need_sources)
        if routing:
            if where != "gather":
                out_v.copy_(x_view)
            return False
        proc = processors[node_type]
        extra, params, common_i = stage_arguments(i)
        if teed is not None and i == 1:
            a, b = teed
            extra["tee"] = buf.narrow(1, a, b - a)
        if prepared is not None and i in prepared:
            state, event = prepared[i]
            main.wait_event(event)
            extra["_prepared"] = state
        if (aux is not None and plan is None and KEEP_SMOOTHER_SCAN and getattr(proc, "accepts_aux", False)
                and type(proc) in _tape_safe_types()):
            # only for the exact library types whose backward consumes it (see `trusted` in the backward); a gathered
            # input is a temporary: the backward re-gathers it, same values
            extra["_aux"] = (aux, i)
        mix = None
        if mix_with is not None:
            nxt = render_data.iter_list[mix_with]
            sched = _mix_schedule(step, nxt, x.device)
            if any(r < n_src for r in sched["extra_rows"]):
                # the sum also takes SOURCE rows, which the kernel reads from `buf`: they are filled by the side stream's
                # copy, and the skipped mix stage is the one that would have joined it (a stage reading `x` directly has not)
                need_sources()
            e0, e1 = nxt.dest_write.idx
            mix = extra["_mix"] = {"sched": sched["sched"], "n_acc": sched["n_acc"], "extras": sched["extras"],
                                   "n_pre": sched["n_pre"], "out": buf.narrow(1, e0, e1 - e0)}
            # output-only render: rows that only the fused sum reads (not the last stage's, not read by any later stage
            # other than the sum itself) are not stored
            if lean and i != render_data.max_order and not any(
                    _reads_rows(render_data.iter_list[k], d0, d1) for k in range(i + 1, render_data.max_order + 1)
                    if k != mix_with and k not in done):
                mix["skip_rows"] = True
        proc.render_into(x_view, out_v, **extra, **params, **common_i)
        launched += 1
        if prepared is None and PREPARE_MODE != "inline" and launched == (2 if PREPARE_MODE == "under_second" else 1):
            # this stage is on its way: now design the later ones underneath it
            prepared = _prepare_later_stages(processors, render_data, stage_arguments, i, main)
        return mix is not None and bool(mix.get("done"))

    out_view = None
    for i in range(1, render_data.max_order + 1):
        d0, d1 = render_data.iter_list[i].dest_write.idx
        out_view = buf.narrow(1, d0, d1 - d0)  # (the last stage's rows are the output)
        if i in done:
            continue
        j, first = (_mix_candidate(processors, render_data, i, done, x.device)
                    if render_data.iter_list[i].node_type in processors else (None, []))
        if j is not None and first and not (ops.MIX_FUSION and L % 4 == 0):
            j, first = None, []      # (the fused kernel would decline: do not reorder for nothing)
        for f in first:
            run_stage(f)
            done.add(f)
        if run_stage(i, mix_with=j):
            done.add(j)
        # (declined: the stage in between has run early and the sum runs at its own place -- still a valid order)
    if side is not None and not copied:
        main.wait_stream(side)  # the returned buffer is complete on the caller's stream
    return (out_view[0] if squeeze else out_view), [], (None if lean else buf[0] if squeeze else buf)
