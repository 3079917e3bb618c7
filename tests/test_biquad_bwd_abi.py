"""The biquad cascade backward's C entries without a GPU: the header and _lib.SIGNATURES both carry them (tests/test_abi.py
holds the two to each other type by type), the workspace query returns the size the header documents, and the entry refuses
bad arguments before any launch."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def documented(R, C_out, K, L):
    """ceil(R * C_out / 2) * ceil(L / 512) * K * 16 bytes: two floats per row-channel, section and 512-sample tile."""
    return -(-R * C_out // 2) * -(-L // 512) * K * 16


def test_the_entries_are_declared_and_bound():
    from grafx_amd import _lib

    header = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    assert "ceil(R * C_out / 2) * ceil(L / 512) * K * 16 bytes" in header
    for name in ("gfx_biquad_cascade_bwd_ws_bytes", "gfx_biquad_cascade_bwd_f32"):
        assert name + "(" in header and name in _lib.SIGNATURES
        assert hasattr(_lib.lib(), name)
    assert _lib.lib().gfx_abi_version() == 2


def test_workspace_query_returns_the_documented_size():
    from grafx_amd import ops

    assert documented(3, 1, 3, 1000) == 2 * 2 * 3 * 16 == 192
    for shape in ((3, 1, 3, 1000), (2, 2, 32, 512), (5, 2, 6, 513), (1, 1, 1, 1), (65601, 2, 3, 64)):
        assert ops.biquad_cascade_bwd_ws_bytes(*shape) == documented(*shape), shape
    assert ops.biquad_cascade_bwd_ws_bytes(1, 2, 1, 512) == 16 and ops.biquad_cascade_bwd_ws_bytes(1, 2, 1, 513) == 32


def test_workspace_query_returns_zero_for_a_bad_argument():
    from grafx_amd import ops

    for i in range(4):
        for bad in (0, -1):
            args = [4, 2, 6, 4096]
            args[i] = bad
            assert ops.biquad_cascade_bwd_ws_bytes(*args) == 0, args


def test_workspace_is_a_small_part_of_one_signal_tensor_at_the_training_shape():
    from grafx_amd import ops

    R, C, K, L = 8192, 2, 6, 131072
    ws, tensor = ops.biquad_cascade_bwd_ws_bytes(R, C, K, L), R * C * L * 4
    print(f"workspace {ws / 1e6:.0f} MB = {100 * ws / tensor:.2f} % of one (R, C, L) tensor")
    assert 0 < ws < 0.05 * tensor


def test_entry_refuses_inconsistent_arguments_before_any_launch():
    """Every check of the entry comes before its first launch, so the refusals need no GPU (abi_checks.device_pointer).
    (The consistent call is made on the GPU, tests/test_gpu_biquad_bwd.py.)"""
    from abi_checks import device_pointer, refused

    from grafx_amd import _lib

    lib = _lib.lib()
    R, Cin, Cf, K, L = 3, 2, 1, 3, 1000
    need = lib.gfx_biquad_cascade_bwd_ws_bytes(R, 2, K, L)
    p, _held = device_pointer()
    rm = _lib.RowMap(R, 0, 2 * L, L)
    good = dict(x=p, xmap=rm, g=p, gmap=rm, gx=p, gxmap=rm, Bs=p, As=p, zi=p, gzf=p, gB=p, gA=p, gzi=p, ws=p, ws_bytes=need,
                R=R, C_in=Cin, C_f=Cf, K=K, L=L, stream=None)
    bad = {
        "a workspace one byte short": dict(ws_bytes=need - 1),
        "no workspace": dict(ws=None),
        "a workspace off the 16-byte grid": dict(ws=p + 4),
        "no input": dict(x=None),
        "no gradient": dict(g=None),
        "no coefficients": dict(Bs=None),
        "no output": dict(gx=None, gB=None, gA=None, gzi=None),
        "33 sections": dict(K=33, ws_bytes=1 << 20),
        "no sections": dict(K=0),
        "no rows": dict(R=0),
        "no samples": dict(L=0),
        "channels that do not broadcast": dict(C_in=2, C_f=3, ws_bytes=1 << 20),
        "shared coefficients over four channels, their gradient asked": dict(C_in=4, C_f=1, ws_bytes=1 << 20),
        "a shared input over four channels, its gradient asked": dict(C_in=1, C_f=4, ws_bytes=1 << 20),
        "an empty row map": dict(xmap=_lib.RowMap(0, 0, 2 * L, L)),
    }
    refused(lib.gfx_biquad_cascade_bwd_f32, good, bad)
