"""Training: the in-place buffer render as one autograd node with a stage-wise backward."""
import contextlib

import torch

from .forward import _render_buffer_io
from .plans import _block_fan, _gather_plan, _plan_max_row, _transposed_plan
from .stage import StageArguments, stage_input

# The adjoint of a routing sum whose sources feed the same destinations in blocks (console: eight strips -> their bus + the
# send) stays in block form -- k rows per graph instead of k * m -- when the stage that wrote those rows can read it so
# (see plans._block_fan, autograd.grad_source).  False: always expand (round 5's path: gather_sum_fanout writes every row).
BLOCK_FAN_ADJOINT = True


def _any_requires_grad(p):
    if isinstance(p, torch.Tensor):
        return p.requires_grad
    return any(_any_requires_grad(v) for v in p.values()) if hasattr(p, "values") else False


def _wants_grad(input_signals, per_type_parameters, common_parameters):
    return torch.is_grad_enabled() and (input_signals.requires_grad or _any_requires_grad(per_type_parameters)
                                        or (common_parameters is not None and _any_requires_grad(common_parameters)))


def _tape_safe_types():
    """Exact processor classes whose output is linear in their one native autograd node (see the stage-wise backward)."""
    from .. import processors as P

    return (P.ParametricEqualizer, P.Compressor, P.NoiseGate, P.STFTMaskedNoiseReverb, P.BiquadFilter,
            P.TanhDistortion, P.PiecewiseTanhDistortion, P.PowerDistortion, P.ChebyshevDistortion)


def _flatten_tree(tree, leaves):
    """Nested dict of tensors -> spec with leaf indices (tensors appended to `leaves`)."""
    if isinstance(tree, torch.Tensor):
        leaves.append(tree)
        return len(leaves) - 1
    if hasattr(tree, "items"):
        return {k: _flatten_tree(v, leaves) for k, v in tree.items()}
    return ("const", tree)


def _unflatten_tree(spec, leaves):
    if isinstance(spec, int):
        return leaves[spec]
    if isinstance(spec, dict):
        return {k: _unflatten_tree(v, leaves) for k, v in spec.items()}
    return spec[1]


def _leaf_indices(spec, acc):
    if isinstance(spec, int):
        acc.add(spec)
    elif hasattr(spec, "items"):
        for v in spec.values():
            _leaf_indices(v, acc)
    return acc


class RowGradients:
    """Gradient of every node's signal -- the rows of a (B, V, C, L) buffer -- accumulated while the backward walks the
    schedule in reverse.

    Held per PART: ``edges`` cuts the rows into the sources and every stage's output rows, one part each, allocated when
    something first contributes to it and dropped as soon as its stage has been back-propagated (one buffer-sized tensor
    before round 6: 28 GiB at the headline batch, 16 GiB of it never used).  Never zero-filled as a whole: ``written``
    tracks which rows hold a value, the first contribution to a row is a copy, later ones add.
    Rows may also exist only in block form: ``virtual[(a, b)] = (rows (B, k, C, L), m)``, row a + i standing for distinct
    row i // m (plans._block_fan).  A stage that reads its output gradient through a row map takes them as they are
    (autograd.grad_source); anything else gets them written out first (materialise)."""

    def __init__(self, edges, B, V, C, L, dtype, device):
        self.edges, self.shape, self.options = edges, (B, C, L), {"dtype": dtype, "device": device}
        self.parts = {}
        self.written = [False] * V
        self.virtual = {}

    def _empty(self, rows):
        B, C, L = self.shape
        return torch.empty(B, rows, C, L, **self.options)

    def part_view(self, a, b):
        """Rows [a, b) when they lie inside one part (allocated on demand), else None."""
        for pa, pb in self.edges:
            if pa <= a and b <= pb:
                t = self.parts.get((pa, pb))
                if t is None:
                    t = self.parts[(pa, pb)] = self._empty(pb - pa)
                return t.narrow(1, a - pa, b - a)
        return None

    def span_view(self, a, b):
        """Rows [a, b) as ONE tensor: inside a part, or over whole parts none of which exists yet; else None."""
        v = self.part_view(a, b) if len(self.pieces(a, b)) == 1 else None
        if v is None:
            cover = [e for e in self.edges if e[0] < b and a < e[1]]
            if cover[0][0] == a and cover[-1][1] == b and not any(e in self.parts for e in cover):
                v = self._empty(b - a)
                for pa, pb in cover:       # (the parts are views of it: it lives until the last of them is dropped)
                    self.parts[(pa, pb)] = v.narrow(1, pa - a, pb - pa)
        return v

    def pieces(self, a, b):
        """[a, b) cut at the part boundaries."""
        cuts = [(max(a, pa), min(b, pb)) for pa, pb in self.edges if pa < b and a < pb]
        if not cuts or cuts[0][0] != a or cuts[-1][1] != b or any(x[1] != y[0] for x, y in zip(cuts, cuts[1:])):
            raise RuntimeError(f"render backward: rows [{a}, {b}) are not covered by the schedule's write ranges")
        return cuts

    def any_written(self, a, b):
        return any(self.written[a:b])

    def fill(self, g):
        """Every row = the caller's gradient of the whole buffer."""
        for pa, pb in self.edges:
            self.part_view(pa, pb).copy_(g.narrow(1, pa, pb - pa))
        self.written = [True] * len(self.written)

    def drop_part(self, a, b):
        """The stage that wrote rows [a, b) has been back-propagated: nobody reads their gradient again."""
        self.parts.pop((a, b), None)

    def set_blocks(self, a, rows, m):
        """Rows [a, a + k * m) now exist only in block form: k distinct rows per graph, each standing for m rows."""
        n = rows.shape[1] * m
        self.virtual[(a, a + n)] = (rows, m)
        self.written[a : a + n] = [True] * n

    def blocks(self, a, b):
        """(rows, m) when exactly rows [a, b) are in block form, else None."""
        return self.virtual.get((a, b))

    def drop_blocks(self, a, b):
        del self.virtual[(a, b)]

    def blocks_overlap(self, a, b):
        return any(r[0] < b and a < r[1] for r in self.virtual)

    def materialise(self, a, b):
        """Write out every block-form range that overlaps [a, b)."""
        B, C, L = self.shape
        for va, vb in [r for r in self.virtual if r[0] < b and a < r[1]]:
            rows, m = self.virtual.pop((va, vb))
            self.part_view(va, vb).view(B, rows.shape[1], m, C, L).copy_(rows.unsqueeze(2))

    def accumulate(self, a, b, g):
        """rows [a, b) += g  (g: (B, b-a, C, L))"""
        self.materialise(a, b)
        written = self.written
        for pa, pb in self.pieces(a, b):
            i = pa
            while i < pb:
                j = i
                while j < pb and written[j] == written[i]:
                    j += 1
                dst, src = self.part_view(i, j), g.narrow(1, i - a, j - i)
                if src.data_ptr() == dst.data_ptr():
                    pass  # the stage wrote its input gradient straight into these rows (autograd.GRAD_SINK)
                elif written[i]:
                    dst.add_(src)
                else:
                    dst.copy_(src)
                written[i:j] = [True] * (j - i)
                i = j

    def settled(self, a, b):
        """Rows [a, b) as they stand; rows nothing contributed to are zero."""
        self.materialise(a, b)
        for i in range(a, b):
            if not self.written[i]:
                self.part_view(i, i + 1).zero_()
                self.written[i] = True
        whole = self.part_view(a, b)
        return whole if whole is not None else torch.cat([self.part_view(x, y) for x, y in self.pieces(a, b)], 1)


def _reads_block_form(proc, L):
    """Can this processor's backward read its output gradient in block form?  (Exact library types only: _stage_backward.)"""
    return type(proc) in _tape_safe_types() and hasattr(proc, "reads_grad_source") and bool(proc.reads_grad_source(L))


def _stage_backward(ctx, i, buf, leaves, live, rows, leaf_grads):
    """Back-propagate processor stage i alone: re-evaluate it on its (detached) input rows with a local tape, feed the tape
    the stage's rows of ``rows``, add the parameter gradients onto ``leaf_grads`` -> the stage's input gradient (B, n, C, L),
    or None when nobody wants it.  The tape goes when this returns: two stages' temporaries never overlap at the peak."""
    from .. import autograd as diff
    from .. import ops

    processors, render_data, p_spec, c_spec = ctx.meta
    B, _, C, L = buf.shape
    step = render_data.iter_list[i]
    d0, d1 = step.dest_write.idx
    plan = _gather_plan(step, buf.device)
    a, b = step.source_reads[0].idx if plan is None else (None, None)
    proc = processors[step.node_type]
    # Every shortcut below assumes that the processor's output is a LINEAR function of the one native autograd node that
    # consumes the stage's input view: true for the library's own classes, not for a user subclass that post-processes
    # super().forward(); so they are enabled for the exact types only (type(), not isinstance()).
    trusted = type(proc) in _tape_safe_types()
    # block-form rows stay as they are for a stage that reads its output gradient through a row map
    blocks = rows.blocks(d0, d1)
    if blocks is not None and not _reads_block_form(proc, L):
        blocks = None
    g_out = None if blocks is not None else rows.settled(d0, d1)
    x_in = stage_input(ops, step, plan, buf, buf, ctx.n_src)[1]  # (the sources are in the saved buffer)
    with torch.enable_grad():
        if not getattr(proc, "accepts_strided_rows", False):
            x_in = x_in.reshape(-1, C, L)  # the (R, C, L) rows of the upstream contract (a copy)
        # a stage fed by the sources alone needs no input gradient unless the caller asked for g_x
        want_gx = ctx.needs_input_grad[1] or (b > ctx.n_src if plan is None else _plan_max_row(step, plan) >= ctx.n_src)
        x_in = x_in.detach().requires_grad_(want_gx)  # else: (B, n, C, L) view of the buffer, no copy
        local = [t.detach().requires_grad_(t.requires_grad) for t in leaves]
        # (shared rows: the processor's front-end runs once per node and its gradient is summed over the batch inside the
        # convolution's backward)
        extra, params, common_i = StageArguments(
            processors, render_data, _unflatten_tree(p_spec, local),
            None if c_spec is None else _unflatten_tree(c_spec, local), ctx.squeeze, B)(i)
        if trusted and i in ctx.aux and getattr(proc, "accepts_aux", False):
            extra["_aux"] = (ctx.aux, i)   # what the forward render kept for this stage
        with diff.tape_only(trusted):  # only the stage's tape is wanted here, not its output values
            y = proc(x_in, **extra, **params, **common_i)
        y = y[0] if isinstance(y, tuple) else y
        wrt = ([x_in] if want_gx else []) + [local[j] for j in live]
        source = contextlib.nullcontext()
        if blocks is not None:
            # the stage's one native node reads the k distinct rows per graph through its row map; the engine
            # carries a placeholder of the output's shape (one element, zero strides)
            block_rows, m = blocks
            grad_out = diff.tape_placeholder(y.shape, buf.device)
            source = diff.grad_source(x_in, block_rows.view(B * block_rows.shape[1], 1, C, L).expand(-1, m, -1, -1))
        else:
            grad_out = g_out if y.shape == g_out.shape else g_out.reshape(y.shape)
        with source:
            sink_rows = None
            if (trusted and want_gx and plan is None and x_in.ndim == 4 and not rows.any_written(a, b)
                    and not rows.blocks_overlap(a, b)):
                sink_rows = rows.span_view(a, b)
            if sink_rows is not None:
                # first (usually only) contribution to these rows: let the stage write it in place
                with diff.grad_sink(x_in, sink_rows) as sink:
                    grads = torch.autograd.grad(y, wrt, grad_outputs=grad_out, allow_unused=True)
                if sink.writes > 1:
                    raise RuntimeError(f"{type(proc).__name__}: {sink.writes} autograd nodes wrote the stage's input "
                                       "gradient in place (expected one)")
            else:
                grads = torch.autograd.grad(y, wrt, grad_outputs=grad_out, allow_unused=True)
        if blocks is not None:
            if source.reads != 1:
                raise RuntimeError(f"{type(proc).__name__}: the stage's block-form output gradient was read by "
                                   f"{source.reads} autograd nodes (expected one)")
            rows.drop_blocks(d0, d1)
    for j, g in zip(live, grads[1:] if want_gx else grads):
        if g is not None:
            leaf_grads[j] = g if leaf_grads[j] is None else leaf_grads[j] + g
    return grads[0].reshape(B, -1, C, L) if want_gx else None


def _gather_adjoint(ctx, i, plan, g_in, rows):
    """Adjoint of stage i's gather-sum: every source row collects the gradients of the slots it fed (transposed plan)."""
    from .. import ops

    processors, render_data = ctx.meta[:2]
    B, _, C, L = g_in.shape
    dev = g_in.device
    step = render_data.iter_list[i]
    fanb = _block_fan(step, plan, dev) if BLOCK_FAN_ADJOINT else None
    if fanb is not None:
        u0, k, m, bidx, bptr = fanb
        # ... provided the stage that wrote exactly these rows can read the block form (else: no point)
        reader = next((render_data.iter_list[j] for j in range(i - 1, 0, -1)
                       if tuple(render_data.iter_list[j].dest_write.idx) == (u0, u0 + k * m)), None)
        if (reader is not None and reader.node_type in processors and _reads_block_form(processors[reader.node_type], L)
                and not rows.any_written(u0, u0 + k * m) and not rows.blocks_overlap(u0, u0 + k * m)):
            # k distinct gradient rows per graph instead of k * m expanded ones: written out only if their reader
            # cannot take them in this form (materialise)
            g_in = g_in if g_in.stride(-1) == 1 else g_in.contiguous()
            rows.set_blocks(u0, ops.gather_sum(g_in, bidx, bptr, torch.empty(B, k, C, L, device=dev)), m)
            return
    uniq, dst_idx, ptr, contiguous, fan = _transposed_plan(step, plan, dev)
    g_src = None
    if contiguous and not rows.any_written(uniq[0], uniq[0] + len(uniq)):
        g_src = rows.span_view(uniq[0], uniq[0] + len(uniq))  # first contribution: gather straight into the rows
    if g_src is None:
        g_src = torch.empty(B, len(uniq), C, L, device=dev)
    g_in = g_in if g_in.stride(-1) == 1 else g_in.contiguous()
    if fan is None or not ops.gather_sum_fanout(g_in, fan[0], fan[1], g_src):
        g_src = ops.gather_sum(g_in, dst_idx, ptr, g_src)
    if contiguous:
        rows.accumulate(uniq[0], uniq[0] + len(uniq), g_src)
    else:
        for k, u in enumerate(uniq):
            rows.accumulate(u, u + 1, g_src.narrow(1, k, 1))


class _BufferRenderFn(torch.autograd.Function):
    """render_grafx as ONE autograd node.

    Forward is the in-place buffer render (the inference path, run without a tape).  The signal buffer it returns
    holds every node's output, i.e. every activation the backward needs, so the backward walks the schedule in
    reverse and, per stage, re-evaluates that stage alone on its (detached) input rows with a local tape,
    back-propagates the stage's slice of the buffer gradient through it, and adds the input gradient onto the
    rows the stage read.  Compared with taping the upstream loop (clone-on-read + in-place slice writes into
    one (B, V, C, L) tensor) this never copies or zero-fills the whole buffer gradient per stage — at the console
    graph that was most of the step — and keeps peak memory at two buffers plus one stage's tape."""

    @staticmethod
    def forward(ctx, meta, input_signals, *leaves):
        processors, render_data, p_spec, c_spec = meta
        params = _unflatten_tree(p_spec, leaves)
        common = None if c_spec is None else _unflatten_tree(c_spec, leaves)
        ctx.aux = {}
        with torch.no_grad():
            _, _, buf = _render_buffer_io(processors, input_signals, params, render_data, common, aux=ctx.aux)
        ctx.meta = meta
        # the backward re-traces the stages on the autograd engine's worker thread, which does not see the caller's
        # context-local set_exact_convolution(): carry the setting the forward ran under
        from ..processors.core.convolution import exact_convolution

        ctx.exact = exact_convolution()
        ctx.squeeze = input_signals.ndim == 3
        ctx.n_src = input_signals.shape[0 if ctx.squeeze else 1]
        ctx.save_for_backward(buf, *leaves)
        # The output rows are returned as an output of their own (a small copy) next to the full buffer: a loss that
        # only looks at the output then sends back a small gradient instead of a zero-filled buffer-sized one.
        d0, d1 = render_data.iter_list[render_data.max_order].dest_write.idx
        ctx.out_rows = (d0, d1)
        ctx.set_materialize_grads(False)
        return buf.narrow(0 if ctx.squeeze else 1, d0, d1 - d0).clone(), buf

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out_rows, g_buf):
        from ..processors.core.convolution import exact_convolution_scope

        with exact_convolution_scope(ctx.exact):
            return _BufferRenderFn._backward(ctx, g_out_rows, g_buf)

    @staticmethod
    def _backward(ctx, g_out_rows, g_buf):
        processors, render_data, p_spec, c_spec = ctx.meta
        buf, *leaves = ctx.saved_tensors
        squeeze = ctx.squeeze
        if squeeze:
            buf = buf.unsqueeze(0)
            g_out_rows = None if g_out_rows is None else g_out_rows.unsqueeze(0)
            g_buf = None if g_buf is None else g_buf.unsqueeze(0)
        steps = render_data.iter_list[1 : render_data.max_order + 1]
        rows = RowGradients(sorted({(0, ctx.n_src)} | {tuple(step.dest_write.idx) for step in steps}),
                            *buf.shape, buf.dtype, buf.device)
        if g_buf is not None:
            rows.fill(g_buf)
        if g_out_rows is not None:
            rows.accumulate(*ctx.out_rows, g_out_rows)
        leaf_grads = [None] * len(leaves)
        live = [i for i, t in enumerate(leaves) if t.requires_grad]

        for i in range(render_data.max_order, 0, -1):
            step = render_data.iter_list[i]
            d0, d1 = step.dest_write.idx
            if not rows.any_written(d0, d1):
                continue  # nothing downstream depends on this stage
            if step.node_type in processors:
                g_in = _stage_backward(ctx, i, buf, leaves, live, rows, leaf_grads)
            else:  # in / out / mix: the (summed) input is the output
                g_in = rows.settled(d0, d1)
            # add the stage's input gradient onto the rows it read
            plan = _gather_plan(step, buf.device)
            if g_in is not None and plan is None:
                rows.accumulate(*step.source_reads[0].idx, g_in)
            elif g_in is not None:
                _gather_adjoint(ctx, i, plan, g_in, rows)
            rows.drop_part(d0, d1)  # this stage has been back-propagated: nobody reads its output gradient again
        # parameters of stages nothing downstream depends on: upstream's taped loop hands back zeros for them (their
        # rows are part of the returned buffer), not None -- optimisers treat the two differently
        # (parameters of a type that has no node in the graph never entered upstream's tape: those stay None)
        scheduled = {step.node_type for step in steps} & set(processors)
        taped = set()
        for node_type in scheduled:
            if hasattr(p_spec, "items") and node_type in p_spec:
                _leaf_indices(p_spec[node_type], taped)
        if scheduled and c_spec is not None:
            _leaf_indices(c_spec, taped)
        for j in live:
            if leaf_grads[j] is None and j in taped:
                leaf_grads[j] = torch.zeros_like(leaves[j])
        g_x = None
        if ctx.needs_input_grad[1]:
            g_x = rows.settled(0, ctx.n_src)
            g_x = (g_x[0] if squeeze else g_x).contiguous()
        return (None, g_x, *leaf_grads)


def _render_buffer_io_with_grad(processors, input_signals, per_type_parameters, render_data, common_parameters):
    leaves = []
    p_spec = _flatten_tree(per_type_parameters, leaves)
    c_spec = None if common_parameters is None else _flatten_tree(common_parameters, leaves)
    out, buf = _BufferRenderFn.apply((processors, render_data, p_spec, c_spec), input_signals, *leaves)
    return out, [], buf
