"""The impulse-response backward's C entries without a GPU: the header and _lib.SIGNATURES both carry them (tests/test_abi.py
holds the two to each other type by type), and the workspace query returns the size the header documents."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entries_are_declared_and_bound():
    from grafx_amd import _lib

    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    for name in ("gfx_stft_reverb_ir_bwd_ws_bytes", "gfx_stft_reverb_ir_bwd_f32"):
        assert name + "(" in header and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


def test_workspace_query_returns_the_documented_size():
    from grafx_amd import ops

    # R * (ceil(2 ir_len / 4096) + ceil(num_frames / 16) * 4 * 193) floats, num_frames = 1 + ir_len / 192
    R, ir_len = 2, 60000
    frames = 1 + ir_len // 192
    want = R * (-(-2 * ir_len // 4096) + -(-frames // 16) * 4 * 193) * 4
    assert want == 123760
    assert ops.stft_reverb_ir_bwd_ws_bytes(R, ir_len) == want
    assert ops.stft_reverb_ir_bwd_ws_bytes(1, 193) == (1 + 1 * 4 * 193) * 4
    assert ops.stft_reverb_ir_bwd_ws_bytes(0, ir_len) == 0 and ops.stft_reverb_ir_bwd_ws_bytes(R, 0) == 0
