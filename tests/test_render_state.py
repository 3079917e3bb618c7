"""RenderState's own bookkeeping (grafx_amd.render.RenderState), with CPU tensors standing in for the carries: no
processor is launched."""
import pytest
import torch

from grafx_amd.render import RenderState

STEPS = (("eq", 8), ("compressor", 8), ("mix", 3), ("reverb", 1), ("out", 1))


def test_construction_and_advancing():
    s = RenderState(2, 2, "cpu", STEPS)
    assert s.samples == 0 and s.carries == {} and s.batch == 2 and s.channels == 2 and s.steps == STEPS
    hist, env = torch.zeros(16, 2, 255), (torch.ones(2, 8, 1),)
    t = s.advanced({1: hist, 2: env, 3: None}, 1536)
    u = t.advanced({1: hist + 1, 2: env, 3: None}, 1)
    assert (s.samples, t.samples, u.samples) == (0, 1536, 1537)
    assert s.carries == {} and t.carries[1] is hist and t.carries[2] is env and t.carries[3] is None
    assert u.steps == STEPS and "samples=1537" in repr(u)
    with pytest.raises(ValueError, match="outside 1..5"):
        RenderState(2, 2, "cpu", STEPS, {6: hist})
    with pytest.raises(ValueError, match="outside 1..5"):
        s.advanced({0: hist}, 1)


def test_steps_of_a_render_data():
    from grafx_amd.data import GRAFX, NodeConfigs, convert_to_tensor
    from grafx_amd.render import prepare_render, reorder_for_fast_render

    G = GRAFX(config=NodeConfigs(["eq", "compressor"]))
    G.add_serial_chain(["in", "eq", "compressor", "eq", "out"])
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam"))
    assert RenderState.steps_of(rd) == (("eq", 1), ("compressor", 1), ("eq", 1), ("out", 1))


@pytest.mark.parametrize("offered, message", [
    ((3, 2, "cpu", STEPS), "made for batch size 2, this render has batch size 3"),
    ((None, 2, "cpu", STEPS), "made for batch size 2, this render has an unbatched render"),
    ((2, 1, "cpu", STEPS), "made for 2 channels, this render has 1"),
    ((2, 2, "meta", STEPS), "lives on device cpu, this render runs on meta"),
    ((2, 2, "cpu", STEPS[:4]), "a render of 5 steps, this render_data has 4"),
    ((2, 2, "cpu", STEPS[:1] + (("compressor", 4),) + STEPS[2:]), "render step 2 of the state is 8 rows of node type "
                                                                  "'compressor', this render_data has 4 rows"),
    ((2, 2, "cpu", STEPS[:3] + (("delay", 1),) + STEPS[4:]), "render step 4 of the state is 1 rows of node type 'reverb', "
                                                             "this render_data has 1 rows of 'delay'"),
])
def test_mismatch_says_which(offered, message):
    s = RenderState(2, 2, "cpu", STEPS)
    assert s.mismatch(2, 2, "cpu", STEPS) is None
    assert message in s.mismatch(*offered)
