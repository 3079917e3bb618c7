"""The two things every walker of the in-place buffer render (forward, stage-wise backward, streamed block) asks per
stage: the keyword arguments of the stage's processor, and where its input rows come from."""
import torch

from .core import expand_tensor_or_tensor_dict, flatten_batch_and_node, read_tensor_or_tensor_dict
from .plans import _gather, _touches_inputs


class StageArguments:
    """``StageArguments(...)(i)`` -> ``(extra, params, common_i)``: what render step i's processor is called with.

    Unbatched render (``squeeze``): the step's rows of its type's parameters.  Batched render: upstream expands every
    per-node parameter B times (render/graph.py:68-75 of the reference); a processor with ``accepts_shared_params`` gets
    the un-expanded rows instead and ``extra["_shared_rows"]`` (it builds its filters once per node and lets every batch
    row read them) -- unless there are common parameters, which are per batch row.  Expansion is a copy kernel per leaf:
    done when the first stage of a node type asks for it and kept for that type's later stages; a type whose stages all
    take shared rows is never expanded.  Common parameters are expanded once, here."""

    def __init__(self, processors, render_data, per_type_parameters, common_parameters, squeeze, B):
        self.processors, self.steps, self.tree, self.squeeze, self.B = (
            processors, render_data.iter_list, per_type_parameters, squeeze, B)
        self.shared = not squeeze and common_parameters is None
        if common_parameters is not None and not squeeze:
            common_parameters = expand_tensor_or_tensor_dict(common_parameters, expand=B, dim=0)
        self.common = common_parameters
        self.expanded = {}  # node type -> its batch-expanded subtree

    def __call__(self, i):
        step = self.steps[i]
        node_type = step.node_type
        extra = {}
        if self.squeeze:
            params = read_tensor_or_tensor_dict(self.tree[node_type], step.parameter_read, dim=0)
        elif self.shared and getattr(self.processors[node_type], "accepts_shared_params", False):
            params = read_tensor_or_tensor_dict(self.tree[node_type], step.parameter_read, dim=0)
            extra["_shared_rows"] = step.dest_write.idx[1] - step.dest_write.idx[0]
        else:
            if node_type not in self.expanded:
                self.expanded[node_type] = expand_tensor_or_tensor_dict(self.tree[node_type], expand=self.B, dim=0)
            params = read_tensor_or_tensor_dict(self.expanded[node_type], step.parameter_read, dim=1,
                                                postprocess=flatten_batch_and_node)
        common_i = {}
        if self.common is not None:
            common_i = read_tensor_or_tensor_dict(self.common, step.dest_write, dim=0 if self.squeeze else 1,
                                                  postprocess=None if self.squeeze else flatten_batch_and_node)
        return extra, params, common_i


def stage_input(ops, step, plan, x, buf, n_src, out=None, need_sources=None):
    """Input rows of a stage -> ``(where, rows)``: ``"x"`` and a view of the sources ``x`` when the read is a plain slice of
    source rows (nothing waits for their copy into the buffer), ``"buf"`` and a view of the signal buffer for any other
    plain slice, ``"gather"`` and the gather-sum of the plan's buffer rows, written into ``out`` (a routing stage's own
    rows) or a fresh temporary.  ``need_sources()`` is the walker's: called before source rows are read from the buffer."""
    read = step.source_reads[0]
    if plan is None:
        a, b = read.idx
        if b <= n_src:
            return "x", x.narrow(1, a, b - a)
    if need_sources is not None and _touches_inputs(read, n_src):
        need_sources()
    if plan is None:
        return "buf", buf.narrow(1, a, b - a)
    if out is None:
        B, _, C, L = buf.shape
        out = torch.empty(B, plan[2], C, L, device=buf.device)
    return "gather", _gather(ops, buf, plan, out)
