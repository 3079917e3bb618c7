"""The materialised silent state of the block protocol (``stream_silence``) on hand-made CPU carries -- no processor is
launched --, and the refusals of ``silent_state`` / ``CapturedStream`` that need no GPU."""
import pytest
import torch


def test_public_names():
    from grafx_amd.processors.core._buffer_io import StreamIO
    from grafx_amd.render import CapturedStream, silent_state
    from grafx_amd.render.capture import CapturedStream as from_capture

    assert callable(silent_state) and CapturedStream is from_capture
    assert callable(StreamIO.stream_silence)


def _unchanged(carry, kept):
    from grafx_amd.processors.core._buffer_io import carry_leaves

    return all(torch.equal(a, b) for a, b in zip(carry_leaves(carry), carry_leaves(kept), strict=True))


def test_silence_of_a_fir_history_and_a_recursive_state_is_zero():
    from grafx_amd.processors import BiquadFilter, FIRFilter, ParametricEqualizer

    g = torch.Generator().manual_seed(0)
    for proc, shape in ((ParametricEqualizer(num_filters=4, flashfftconv=False, fsm_fir_len=256), (4, 2, 255)),
                        (FIRFilter(fir_len=63, flashfftconv=False), (4, 1, 62)),
                        (ParametricEqualizer(num_filters=4, backend="lfilter"), (2, 2, 2, 4, 2)),
                        (BiquadFilter(num_filters=2, backend="lfilter"), (2, 2, 2, 2, 2))):
        carry = torch.randn(*shape, generator=g)
        kept = carry.clone()
        silent = proc.stream_silence(carry)
        assert silent is not carry and silent.shape == carry.shape and silent.dtype == carry.dtype
        assert torch.equal(silent, torch.zeros(shape)) and torch.equal(carry, kept)
        assert proc.stream_silence(None) is None


def test_silence_of_the_ballistics_smoothers_is_one():
    from grafx_amd.processors import BallisticsEnvelopeFollower, Compressor, NoiseGate
    from grafx_amd.processors.core.envelope import Ballistics

    g = torch.Generator().manual_seed(1)
    for proc, shape in ((Compressor(energy_smoother="ballistics", iir_len=255, flashfftconv=False), (2, 3, 1)),
                        (NoiseGate(energy_smoother="ballistics", gain_smoother="ballistics", iir_len=255, flashfftconv=False),
                         (2, 3, 2)),
                        (Ballistics(), (6,)), (BallisticsEnvelopeFollower(), (6,))):
        carry = torch.rand(*shape, generator=g)
        kept = carry.clone()
        silent = proc.stream_silence(carry)
        assert silent is not carry and torch.equal(silent, torch.ones(shape)) and torch.equal(carry, kept)
        assert proc.stream_silence(None) is None
    # a compressor without a smoother is memoryless: its carry is None and stays None
    assert Compressor(energy_smoother=None, flashfftconv=False).stream_silence(None) is None


def test_a_container_maps_its_childrens_carries_leaf_by_leaf():
    from grafx_amd.processors import Compressor, DryWet, ParametricEqualizer, SerialChain, StereoGain

    eq = ParametricEqualizer(num_filters=4, flashfftconv=False, fsm_fir_len=256)
    comp = Compressor(energy_smoother="ballistics", iir_len=255, flashfftconv=False)
    chain = SerialChain({"strip": SerialChain({"eq": eq, "comp": comp}), "gain": StereoGain(), "wet": DryWet(comp)})
    g = torch.Generator().manual_seed(2)
    carry = ((torch.randn(2, 2, 255, generator=g), torch.rand(2, 1, 1, generator=g)), None, (torch.rand(2, 1, 1, generator=g),))
    kept = ((carry[0][0].clone(), carry[0][1].clone()), None, (carry[2][0].clone(),))
    silent = chain.stream_silence(carry)
    assert isinstance(silent, tuple) and len(silent) == 3 and isinstance(silent[0], tuple) and len(silent[0]) == 2
    assert torch.equal(silent[0][0], torch.zeros(2, 2, 255))        # the equaliser's history
    assert torch.equal(silent[0][1], torch.ones(2, 1, 1))           # the compressor's envelope
    assert silent[1] is None                                        # a memoryless child
    assert isinstance(silent[2], tuple) and torch.equal(silent[2][0], torch.ones(2, 1, 1))
    assert _unchanged(carry, kept)
    assert chain.stream_silence(None) is None


def _chain():
    from grafx_amd.data import GRAFX, NodeConfigs, convert_to_tensor
    from grafx_amd.processors import Compressor
    from grafx_amd.render import prepare_render, reorder_for_fast_render

    G = GRAFX(config=NodeConfigs(["compressor"]))
    G.add_serial_chain(["in", "compressor", "out"])
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam"))
    procs = {"compressor": Compressor(energy_smoother="ballistics", iir_len=255, flashfftconv=False)}
    params = {"compressor": {k: torch.zeros(1, n) for k, n in (("log_threshold", 1), ("log_ratio", 1), ("log_knee", 1),
                                                                   ("z_alpha_pre", 2))}}
    return procs, torch.zeros(2, 1, 2, 64), params, rd


def test_cpu_signals_are_refused():
    from grafx_amd.render import CapturedStream, silent_state

    with pytest.raises(ValueError, match="not on a GPU"):
        silent_state(*_chain())
    with pytest.raises(ValueError, match="HIP path"):
        CapturedStream(*_chain())
