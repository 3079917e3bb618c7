"""The noise-shaping impulse-response backward's C entries without a GPU: the header and _lib.SIGNATURES both carry them
(tests/test_abi.py holds the two to each other type by type), and the workspace query returns the size the header documents."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_entries_are_declared_and_bound():
    from grafx_amd import _lib

    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    for name in ("gfx_noise_shaping_ir_bwd_ws_bytes", "gfx_noise_shaping_ir_bwd_f32"):
        assert name + "(" in header and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)


def test_workspace_query_returns_the_documented_size():
    from grafx_amd import ops

    # R * C * ceil(ir_len / 2048) * (8 K + 1) floats
    R, C, K, ir_len = 2, 2, 12, 60000
    want = R * C * -(-ir_len // 2048) * (8 * K + 1) * 4
    assert want == 46560
    assert ops.noise_shaping_ir_bwd_ws_bytes(R, C, K, ir_len) == want
    assert ops.noise_shaping_ir_bwd_ws_bytes(1, 1, 1, 1) == 9 * 4
    assert ops.noise_shaping_ir_bwd_ws_bytes(1, 1, 1, 2048) == 9 * 4 and ops.noise_shaping_ir_bwd_ws_bytes(1, 1, 1, 2049) == 18 * 4


def test_entry_refuses_inconsistent_arguments_before_any_launch():
    """Every check of the entry comes before its first launch, so the refusals need no GPU: the pointers below are never
    followed.  (The consistent call is made on the GPU, tests/test_gpu_noise_shaping_ir_bwd.py.)"""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, K, T = 2, 2, 3, 100
    need = lib.gfx_noise_shaping_ir_bwd_ws_bytes(R, C, K, T)
    p = 0x1000      # stands for any non-null device pointer
    good = dict(grad_ir=p, ir=p, row_gain=p, noise=p, noise_stride=T, log_decay=p, log_gain=p, log_fade_in=p,
                z_fade_in_gain=p, g_log_decay=p, g_log_gain=p, g_log_fade_in=p, g_z_fade_in_gain=p, R=R, C=C, K=K, ir_len=T,
                min_decay=-0.2, max_decay=-0.005, ws=p, ws_bytes=need, stream=None)
    bad = {
        "a workspace one byte short": dict(ws_bytes=need - 1),
        "no workspace": dict(ws=None),
        "no gradient": dict(grad_ir=None),
        "the taps without their gains": dict(row_gain=None),
        "the gains without their taps": dict(ir=None),
        "half a fade pair": dict(z_fade_in_gain=None, g_z_fade_in_gain=None),
        "a fade gradient without the fade pair": dict(log_fade_in=None, z_fade_in_gain=None, g_z_fade_in_gain=None),
        "no output": dict(g_log_decay=None, g_log_gain=None, g_log_fade_in=None, g_z_fade_in_gain=None),
        "65 bands": dict(K=65, ws_bytes=1 << 20),
        "a noise stride below the length": dict(noise_stride=T - 1),
        "no rows": dict(R=0),
        "an empty response": dict(ir_len=0),
    }
    for what, change in bad.items():
        assert lib.gfx_noise_shaping_ir_bwd_f32(*{**good, **change}.values()) == -1, what   # GFX_EINVAL


def test_workspace_query_returns_zero_for_a_zero_argument():
    from grafx_amd import ops

    for zero in range(4):
        args = [2, 2, 12, 60000]
        args[zero] = 0
        assert ops.noise_shaping_ir_bwd_ws_bytes(*args) == 0
