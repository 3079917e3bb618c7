"""Host logic of the in-place buffer renders, on CPU tensors: the backward's row gradients against a dense model
(render/backward.py: RowGradients), a stage's arguments against the expression of the upstream loop (render/stage.py:
StageArguments), the transposed gather plan as the adjoint of the plan (render/plans.py)."""
from types import SimpleNamespace

import pytest
import torch

B, V, C, L = 2, 8, 1, 3
EDGES = [(0, 3), (3, 5), (5, 8)]


def _rows():
    from grafx_amd.render.backward import RowGradients

    return RowGradients(EDGES, B, V, C, L, torch.float32, torch.device("cpu"))


def _ints(n, seed):
    """Integer-valued float32 rows: sums of them are exact, every comparison below is torch.equal."""
    return torch.randint(-4, 5, (B, n, C, L), generator=torch.Generator().manual_seed(seed)).float()


def test_row_gradients_accumulate_like_a_dense_buffer():
    rows, dense = _rows(), torch.zeros(B, V, C, L)
    for a, b, seed in [(0, 2, 1), (0, 2, 2),      # inside one part, twice: a copy, then an add
                       (1, 3, 3),                 # rows 1 (written) and 2 (not yet) of one part in one call
                       (2, 5, 4)]:                # across two parts in one call
        g = _ints(b - a, seed)
        rows.accumulate(a, b, g)
        dense[:, a:b] += g
        assert rows.any_written(a, b)
    assert not rows.any_written(5, 8)
    assert torch.equal(rows.settled(5, 8), torch.zeros(B, 3, C, L))    # never contributed to: zeros
    assert rows.any_written(5, 8)
    assert torch.equal(rows.settled(0, 3), dense[:, 0:3])
    assert torch.equal(rows.settled(0, 8), dense)                        # over all parts: concatenated
    with pytest.raises(RuntimeError, match="not covered by the schedule's write ranges"):
        rows.accumulate(6, 10, _ints(4, 5))
    with pytest.raises(RuntimeError, match="not covered by the schedule's write ranges"):
        rows.span_view(6, 10)


def test_row_gradients_span_view_backs_parts_that_do_not_exist_yet():
    rows, dense = _rows(), torch.zeros(B, V, C, L)
    span = rows.span_view(3, 8)                    # two parts, neither exists: one tensor behind both
    assert span.shape == (B, 5, C, L) and not rows.any_written(3, 8)
    g = _ints(5, 6)
    span.copy_(g)                                  # (a stage writes its input gradient straight into it ...)
    rows.accumulate(3, 8, span)                    # ... and hands the same storage in: not added onto itself
    dense[:, 3:8] += g
    assert rows.any_written(3, 4) and rows.any_written(7, 8)
    assert torch.equal(rows.settled(3, 8), dense[:, 3:8])
    assert rows.part_view(3, 5).data_ptr() == span.data_ptr()
    g = _ints(5, 7)
    rows.accumulate(3, 8, g)                       # a second contribution adds
    dense[:, 3:8] += g
    assert torch.equal(rows.settled(0, 8), dense)

    rows = _rows()
    rows.accumulate(3, 5, _ints(2, 8))
    assert rows.span_view(3, 8) is None            # one of the parts exists
    assert rows.span_view(3, 5) is not None and rows.span_view(4, 5).shape == (B, 1, C, L)     # inside one part: a view
    assert rows.span_view(0, 3) is not None        # a whole part that does not exist yet

    rows.drop_part(3, 5)                           # its stage is done
    span = rows.span_view(3, 8)                    # ... so the rows can be backed afresh
    assert span is not None and rows.parts[(3, 5)].data_ptr() == span.data_ptr()


def test_row_gradients_block_form_rows_are_written_out_before_anything_adds_to_them():
    rows, dense = _rows(), torch.zeros(B, V, C, L)
    distinct = _ints(1, 9)                         # k = 1 distinct row per graph, standing for m = 2 rows
    rows.set_blocks(3, distinct, 2)
    dense[:, 3:5] += distinct
    assert rows.blocks(3, 5)[1] == 2 and rows.blocks(3, 5)[0] is distinct and rows.blocks(3, 4) is None
    assert rows.any_written(3, 5) and (3, 5) not in rows.parts
    assert rows.blocks_overlap(4, 6) and not rows.blocks_overlap(5, 8) and not rows.blocks_overlap(0, 3)
    g = _ints(2, 10)
    rows.accumulate(4, 6, g)                       # overlaps the block-form rows: they are materialised first
    dense[:, 4:6] += g
    assert rows.blocks(3, 5) is None and not rows.blocks_overlap(3, 5)
    assert torch.equal(rows.settled(3, 8), dense[:, 3:8])

    rows = _rows()
    rows.set_blocks(3, distinct, 2)
    assert torch.equal(rows.settled(3, 5), distinct.expand(B, 2, C, L))      # ... and before anybody reads them as rows
    rows = _rows()
    rows.set_blocks(3, distinct, 2)
    rows.drop_blocks(3, 5)                         # read in block form by their stage
    assert rows.blocks(3, 5) is None


# ---- stage arguments ------------------------------------------------------------------------------------------------
def _access(idx):
    return SimpleNamespace(method="index" if isinstance(idx, torch.Tensor) else "slice", idx=idx)


def _schedule():
    def step(node_type, read, dest):
        return SimpleNamespace(node_type=node_type, parameter_read=_access(read), dest_write=_access(dest))

    return SimpleNamespace(iter_list=[None, step("eq", (0, 2), (0, 2)), step("eq", torch.tensor([3, 1]), (2, 4)),
                                      step("comp", (1, 4), (4, 7))])


def _tree():
    gen = torch.Generator().manual_seed(0)
    return {"eq": {"gain": torch.randn(4, 3, generator=gen), "band": {"q": torch.randn(4, 2, generator=gen)}},
            "comp": {"threshold": torch.randn(5, 1, generator=gen)}}


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    return a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)


def _upstream(tree, access, node_type, batch):
    """What the generic loop of render/graph.py computes (node_type None: the common parameters)."""
    from grafx_amd.render.core import expand_tensor_or_tensor_dict, flatten_batch_and_node, read_tensor_or_tensor_dict

    if batch is None:
        return read_tensor_or_tensor_dict(tree if node_type is None else tree[node_type], access, dim=0)
    tree = expand_tensor_or_tensor_dict(tree, batch, 0)
    return read_tensor_or_tensor_dict(tree if node_type is None else tree[node_type], access, dim=1,
                                      postprocess=flatten_batch_and_node)


@pytest.mark.parametrize("batch", [None, 3])
@pytest.mark.parametrize("with_common", [False, True])
def test_stage_arguments_are_the_upstream_reads(batch, with_common):
    from grafx_amd.render.stage import StageArguments

    rd, tree = _schedule(), _tree()
    common = {"level": torch.arange(14.0).view(7, 2)} if with_common else None
    procs = {"eq": SimpleNamespace(), "comp": SimpleNamespace()}
    arguments = StageArguments(procs, rd, tree, common, batch is None, 1 if batch is None else batch)
    for i in (1, 2, 3):
        step = rd.iter_list[i]
        extra, params, common_i = arguments(i)
        assert extra == {}
        assert _same(params, _upstream(tree, step.parameter_read, step.node_type, batch))
        assert _same(common_i, _upstream(common, step.dest_write, None, batch) if with_common else {})
    if batch is not None:
        assert params["threshold"].shape == (3 * 3, 1)


def test_stage_arguments_leave_shared_rows_unexpanded_and_expand_a_type_once(monkeypatch):
    from grafx_amd.render import stage
    from grafx_amd.render.core import read_tensor_or_tensor_dict

    rd, tree = _schedule(), _tree()
    expanded = []
    real = stage.expand_tensor_or_tensor_dict
    monkeypatch.setattr(stage, "expand_tensor_or_tensor_dict", lambda x, **kw: expanded.append(x) or real(x, **kw))
    # "comp" takes shared rows, "eq" does not: two steps of "eq" expand its subtree once, "comp"'s is never expanded
    procs = {"eq": SimpleNamespace(), "comp": SimpleNamespace(accepts_shared_params=True)}
    arguments = stage.StageArguments(procs, rd, tree, None, False, 3)
    for i in (1, 2, 3, 2):
        step = rd.iter_list[i]
        extra, params, common_i = arguments(i)
        assert common_i == {}
        if step.node_type == "comp":
            assert extra == {"_shared_rows": 3}
            assert _same(params, read_tensor_or_tensor_dict(tree["comp"], step.parameter_read, dim=0))
            assert params["threshold"].shape == (3, 1)
        else:
            assert extra == {} and _same(params, _upstream(tree, step.parameter_read, "eq", 3))
    assert len(expanded) == 1 and expanded[0] is tree["eq"]
    # common parameters are per batch row: nobody takes shared rows then, and they are expanded once, up front
    expanded.clear()
    common = {"level": torch.arange(14.0).view(7, 2)}
    arguments = stage.StageArguments(procs, rd, tree, common, False, 3)
    assert len(expanded) == 1 and expanded[0] is common
    extra, params, common_i = arguments(3)
    assert extra == {} and _same(params, _upstream(tree, rd.iter_list[3].parameter_read, "comp", 3))
    assert [x is tree["comp"] for x in expanded] == [False, True]
    # an unbatched render expands nothing
    expanded.clear()
    stage.StageArguments(procs, rd, tree, common, True, 1)(1)
    assert expanded == []


# ---- gather plans ---------------------------------------------------------------------------------------------------
def test_transposed_plan_is_the_adjoint_of_the_gather_plan():
    from grafx_amd.render.plans import _gather_plan, _transposed_plan

    dev = torch.device("cpu")
    step = SimpleNamespace(source_reads=[_access(torch.tensor([0, 1, 1, 2]))],
                           aggregations=[SimpleNamespace(method="scatter", idx=torch.tensor([0, 0, 1, 1]))])
    plan = _gather_plan(step, dev)
    src, seg, n_out, fan = plan
    assert src.tolist() == [0, 1, 1, 2] and seg.tolist() == [0, 2, 4] and n_out == 2
    assert _gather_plan(step, dev) is plan                       # built once per step and device
    src, seg = src.tolist(), seg.tolist()
    dense = torch.zeros(n_out, 3, dtype=torch.long)              # slot j sums the rows r with dense[j, r] == 1
    for j in range(n_out):
        for e in range(seg[j], seg[j + 1]):
            dense[j, src[e]] += 1
    assert dense.tolist() == [[1, 1, 0], [0, 1, 1]]

    uniq, dst, ptr, contiguous, fan_T = _transposed_plan(step, plan, dev)
    assert uniq == [0, 1, 2] and contiguous
    dst, ptr = dst.tolist(), ptr.tolist()
    transposed = torch.zeros(len(uniq), n_out, dtype=torch.long)  # source row uniq[k] collects the slots it fed
    for k in range(len(uniq)):
        for e in range(ptr[k], ptr[k + 1]):
            transposed[k, dst[e]] += 1
    assert torch.equal(transposed, dense[:, uniq].t())

    # the two fan-out forms (read every row once, add it to the slots of its bit mask) describe the same matrix
    rows, masks = fan                                            # forward: per distinct source row, a mask over slots
    forward = torch.zeros_like(dense)
    for r, mask in zip(rows.tolist(), masks.tolist()):
        for j in range(n_out):
            forward[j, r] = (mask >> j) & 1
    assert torch.equal(forward, dense)
    slots, masks = fan_T                                         # adjoint: per slot, a mask over the distinct source rows
    adjoint = torch.zeros_like(dense)
    for j, mask in zip(slots.tolist(), masks.tolist()):
        for k, r in enumerate(uniq):
            adjoint[j, r] = (mask >> k) & 1
    assert torch.equal(adjoint, dense)
