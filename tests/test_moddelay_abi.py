"""The modulated delay line without a GPU: the three C entries are declared, bound and exported with their argument lists;
the workspace query returns the documented size and 0 for bad arguments; every refusal of the entries comes back before a
launch; the constructor takes what is documented and ``physical()`` stays inside the kernels' contract; the float64
yardstick agrees with a brute-force loop, its autograd with the written adjoint, its blocks with its one call; an integer
delay without depth is the shifted input; ``torch_forward`` is the yardstick; and the read position is monotone with runs
of at most two on the drawn parameters."""
import math

import numpy as np
import pytest
import torch

import moddelay_float64 as m64
from abi_checks import device_pointer, entries_match, refused

ENTRIES = ("gfx_moddelay_f32", "gfx_moddelay_bwd_ws_bytes", "gfx_moddelay_bwd_f32")
# V, Dmax, interp of the small float64 checks
SMALL = ((1, 2, "linear"), (2, 8, "cubic"), (3, 21, "cubic"), (2, 13, "linear"))


def test_the_entries_are_declared_bound_and_exported():
    cf, f = "const float*", "float*"
    head = [cf, "gfx_rowmap_t", "{second}", "gfx_rowmap_t"] + ["int64_t"] * 6 + [cf] * 6
    fwd = [t.format(second=f) for t in head] + [cf, "const int64_t*", f, "int64_t*", "void*"]
    bwd = [t.format(second=cf) for t in head] + [f, "gfx_rowmap_t"] + [f] * 6 + ["void*", "size_t", "void*"]
    entries_match(ENTRIES, dict(zip(ENTRIES, (("int", fwd), ("size_t", ["int64_t"] * 4), ("int", bwd)))))


def test_tile_and_workspace_query():
    from grafx_amd import _lib, ops

    assert (ops.MODDELAY_MAX_DELAY, ops.MODDELAY_MAX_VOICES) == (8192, 8)
    assert ops.MODDELAY_GRADS == ("x", "delay", "depth", "rate", "phase", "gain", "dry")
    for dmax in (2, 441, 1764, 8192):
        t = ops.moddelay_tile(dmax, 2)
        # the largest tile of either way fits the CU's 160 KiB of LDS twice: the forward's samples, the backward's positions
        assert t % 256 == 0 and 4 * (t + dmax + 2) <= 80 * 1024 and 6 * (t + dmax + 4) <= 80 * 1024
    for bad in ((1, 2), (8193, 2), (441, 0), (441.0, 2), (True, 2), (441, True)):
        with pytest.raises(ValueError):
            ops.moddelay_tile(*bad)
    query = _lib.lib().gfx_moddelay_bwd_ws_bytes
    for R, C, L, V in ((1, 1, 1, 1), (3, 2, 4097, 3), (2, 5, 4096, 8), (70000, 1, 40, 2), (256, 2, 131072, 4)):
        assert query(R, C, L, V) == 8 * R * -(-L // ops.moddelay_tile(441, C)) * (1 + 3 * V + 2 * V * C), (R, C, L, V)
    for bad in ((0, 2, 100, 2), (-1, 2, 100, 2), (2, 0, 100, 2), (2, 2, 0, 2), (2, 2, -5, 2), (2, 2, 100, 0), (2, 2, 100, 9)):
        assert query(*bad) == 0, bad


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check comes before the first launch, so the refusals need no GPU (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, L, V, Dmax = 3, 2, 5000, 2, 441
    S = Dmax + 2
    need = lib.gfx_moddelay_bwd_ws_bytes(R, C, L, V)
    p, _held = device_pointer()
    far = p + 4 * R * C * L      # a second signal that does not overlap the first, then a third, then two states
    third = far + 4 * R * C * L
    z0 = third + 4 * R * C * L
    z1 = z0 + 4 * R * C * S
    q0, q1 = z1 + 4 * R * C * S, z1 + 4 * R * C * S + 8 * R
    rm, empty, neg = _lib.RowMap(R, 0, C * L, L), _lib.RowMap(0, 0, C * L, L), _lib.RowMap(R, 0, -C * L, L)
    six = dict(delay=p, depth=p, rate=p, phase=p, gain=p, dry=p)
    fwd = dict(x=p, xmap=rm, y=far, ymap=rm, R=R, C=C, L=L, V=V, interp=1, max_delay=Dmax, **six, zi=None, pos_in=None, zf=None,
               pos_out=None, stream=None)
    bwd = dict(x=p, xmap=rm, gy=far, gmap=rm, R=R, C=C, L=L, V=V, interp=1, max_delay=Dmax, **six, gx=third, gxmap=rm,
               g_delay=p, g_depth=p, g_rate=p, g_phase=p, g_gain=p, g_dry=p, ws=p, ws_bytes=need, stream=None)
    bad = {
        "no signal": dict(x=None), "an empty row map": dict(xmap=empty), "no rows": dict(R=0), "negative rows": dict(R=-3),
        "no channels": dict(C=0), "no samples": dict(L=0), "negative length": dict(L=-5), "no voices": dict(V=0),
        "nine voices": dict(V=9), "an unknown interpolation": dict(interp=2), "a negative interpolation": dict(interp=-1),
        "a delay line of 1": dict(max_delay=1), "a delay line of 8193": dict(max_delay=8193),
        **{f"no {name}": {name: None} for name in six},
        "more than 2^31 - 1 row-channels": dict(R=1 << 16, C=1 << 15),
        "more than 2^31 - 1 workgroups": dict(R=1 << 20, L=2048 * (1 << 11) + 1),
        "a negative stride": dict(xmap=neg),
    }
    only_fwd = {"no output": dict(y=None), "an empty output row map": dict(ymap=empty), "an output that is the input": dict(y=p),
                "an output that overlaps the input": dict(y=p + 4), "a negative output stride": dict(ymap=neg),
                "a history without a position": dict(zi=z0), "a position without a history": dict(pos_in=q0),
                "a new history without a new position": dict(zf=z1), "a new position alone": dict(pos_out=q1),
                "zf is zi": dict(zi=z0, pos_in=q0, zf=z0, pos_out=q1),
                "zf overlaps zi": dict(zi=z0, pos_in=q0, zf=z0 + 4 * (R * C * S - 1), pos_out=q1),
                "pos_out is pos_in": dict(zi=z0, pos_in=q0, zf=z1, pos_out=q0)}
    only_bwd = {"no output gradient": dict(gy=None), "an empty gradient row map": dict(gmap=empty),
                "nothing asked for": dict(gx=None, **{"g_" + name: None for name in six}), "gx is x": dict(gx=p),
                "gx is gy": dict(gx=far), "gx overlaps x a sample later": dict(gx=p + 4), "an empty gx row map": dict(gxmap=empty),
                "a parameter gradient without a workspace": dict(ws=None), "a workspace that is not 8-byte aligned": dict(ws=p + 4)}
    refused(lib.gfx_moddelay_f32, fwd, {**bad, **only_fwd})
    refused(lib.gfx_moddelay_bwd_f32, bwd, {**bad, **only_bwd})
    refused(lib.gfx_moddelay_bwd_f32, bwd, {"a workspace one byte short": dict(ws_bytes=need - 1)}, code=-2)


def test_constructor_and_parameter_size():
    import grafx_amd.processors as P

    m = P.ModulatedDelay()
    assert (m.num_voices, m.min_delay, m.max_delay, m.max_rate, m.sample_rate) == (2, 16, 1764, 8.0, 44100.0)
    assert (m.interpolation, m.processor_channel, m.latency, m.state_samples) == ("cubic", "stereo", 0, 1766)
    assert m.parameter_size() == {"z_delay": 2, "z_depth": 2, "z_rate": 2, "phase": (2, 2), "log_gain": (2, 2), "log_dry": 1}
    assert m.state_dict() == {} and m.accepts_strided_rows
    m.stream_check()
    mono = P.ModulatedDelay(8, 0, 8192, interpolation="linear", processor_channel="mono")
    assert mono.parameter_size()["phase"] == (8, 1) and mono.state_samples == 8194
    for kwargs, why in ((dict(max_delay=8193), "8192 at most"), (dict(min_delay=1764), "below max_delay"),
                        (dict(min_delay=0, max_delay=1), ">= 2"), (dict(num_voices=9), "8 at most"), (dict(num_voices=0), ">= 1"),
                        (dict(interpolation="sinc"), "'linear' or 'cubic'"), (dict(max_rate=0.0), "positive"),
                        (dict(max_rate=-1.0), "positive"), (dict(sample_rate=0), "positive"), (dict(num_voices=2.0), "integer"),
                        (dict(max_delay=True), "integer"), (dict(processor_channel="midside"), "'mono' or 'stereo'"),
                        (dict(min_delay=1, max_delay=2, num_voices=1), None)):
        if why is None:
            P.ModulatedDelay(**kwargs)
            continue
        with pytest.raises(ValueError, match=why):
            P.ModulatedDelay(**kwargs)


@pytest.mark.parametrize("kwargs", [dict(), dict(min_delay=0, max_delay=8192, max_rate=20.0), dict(min_delay=1, max_delay=2),
                                    dict(max_rate=0.01, max_delay=8192), dict(min_delay=400, max_delay=441, sample_rate=8000)])
def test_physical_stays_inside_the_contract(kwargs):
    """For z at +-30 and everything between, in float32: the delay's swing inside [max(1, min_delay), max_delay] and the
    slope 2 pi rate depth within 1/2, evaluated in float64 on the float32 values the kernel gets."""
    import grafx_amd.processors as P

    m = P.ModulatedDelay(num_voices=3, **kwargs)
    grid = torch.tensor([-30.0, -8.0, -1.0, 0.0, 0.5, 3.0, 12.0, 30.0])
    zd, zp, zr = (t.reshape(-1, 3) for t in torch.meshgrid(grid, grid, grid[:6], indexing="ij"))
    R = zd.shape[0]
    zr = torch.cat([zr[:-1], torch.full((1, 3), 30.0)])
    delay, depth, rate, phase, gain, dry = m.physical(zd, zp, zr, torch.zeros(R, 3, 2), torch.zeros(R, 3, 2), torch.zeros(R, 1))
    assert all(t.dtype == torch.float32 for t in (delay, depth, rate, phase, gain, dry))
    assert (tuple(delay.shape), tuple(phase.shape), tuple(gain.shape), tuple(dry.shape)) == ((R, 3), (R, 3, 2), (R, 3, 2), (R,))
    delay, depth, rate = delay.double(), depth.double(), rate.double()
    lo, hi = max(1, m.min_delay), m.max_delay
    assert bool((depth >= 0).all()) and float((delay - depth).min()) >= lo and float((delay + depth).max()) <= hi
    assert float((2 * math.pi * rate * depth).max()) <= 0.5 and float(rate.max()) <= m.max_rate / m.sample_rate * (1 + 1e-7)
    assert float(depth.max()) > 0.4 * min((hi - lo) / 2, 0.45 / (2 * math.pi * float(rate.min())))      # (and it does swing)
    assert torch.equal(gain, torch.ones_like(gain)) and torch.equal(dry, torch.ones(R))


def _case(V, Dmax, seed, R=4, C=2, L=60):
    return m64.bright_rows(R, C, L, seed), m64.draw_parameters(R, V, C, Dmax, seed + 100)


@pytest.mark.parametrize("V,Dmax,interp", SMALL)
def test_the_yardstick_agrees_with_a_brute_force_loop(V, Dmax, interp):
    x, params = _case(V, Dmax, seed=V + Dmax)
    y, (zf, pos) = m64.forward(x, *params, Dmax, interp)
    assert np.abs(y.numpy() - m64.brute(x, *params, Dmax, interp)).max() <= 1e-13
    assert pos.tolist() == [60] * 4 and torch.equal(zf[..., -60:] if Dmax + 2 >= 60 else zf, x.double()[..., -(Dmax + 2):])
    gen = torch.Generator().manual_seed(1)
    state = (torch.randn(4, 2, Dmax + 2, generator=gen), torch.tensor([0, 7, 12345, 2 ** 31 - 5]))
    y, (zf, pos) = m64.forward(x, *params, Dmax, interp, state)
    assert np.abs(y.numpy() - m64.brute(x, *params, Dmax, interp, state)).max() <= 1e-13
    assert torch.equal(pos, state[1] + 60)
    assert torch.equal(zf, torch.cat([state[0].double(), x.double()], -1)[..., -(Dmax + 2):])


@pytest.mark.parametrize("V,Dmax,interp", SMALL)
def test_autograd_of_the_yardstick_agrees_with_the_written_adjoint(V, Dmax, interp):
    x, params = _case(V, Dmax, seed=10 + V + Dmax, L=90)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    auto = m64.gradients(x, g, *params, Dmax, interp)
    written = m64.adjoint(x, g, *params, Dmax, interp)
    for name, a, w in zip(("x", "delay", "depth", "rate", "phase", "gain", "dry"), auto, written):
        assert np.abs(a.numpy() - w).max() <= 1e-11 * max(1.0, np.abs(w).max()), name
        assert np.abs(w).max() > 0, name


@pytest.mark.parametrize("V,Dmax,interp", SMALL)
def test_blocks_equal_one_call_exactly(V, Dmax, interp):
    x, params = _case(V, Dmax, seed=20)
    whole, (wz, wpos) = m64.forward(x, *params, Dmax, interp)
    ys, state, at = [], None, 0
    for n in (7, 1, 20, 32):
        y, state = m64.forward(x[..., at:at + n], *params, Dmax, interp, state)
        ys.append(y)
        at += n
    assert at == 60 and torch.equal(torch.cat(ys, -1), whole)
    assert torch.equal(state[0], wz) and torch.equal(state[1], wpos)


@pytest.mark.parametrize("interp", ["linear", "cubic"])
@pytest.mark.parametrize("Dmax,D", [(2, 1), (2, 2), (21, 1), (21, 13), (21, 21)])
def test_an_integer_delay_without_depth_is_the_shifted_input(interp, Dmax, D):
    x = m64.bright_rows(2, 2, 50, 5)
    ones = torch.ones(2, 1)
    params = (D * ones, 0 * ones, 1e-3 * ones, torch.rand(2, 1, 2), torch.full((2, 1, 2), 0.5), torch.tensor([0.25, 2.0]))
    y, _ = m64.forward(x, *params, Dmax, interp)
    xd = x.double()
    shifted = torch.nn.functional.pad(xd, (D, 0))[..., :50]
    assert torch.equal(y, torch.tensor([0.25, 2.0], dtype=torch.float64).reshape(2, 1, 1) * xd + 0.5 * shifted)


@pytest.mark.parametrize("V,Dmax,interp", SMALL)
def test_torch_forward_is_the_definition(V, Dmax, interp):
    """torch_forward in float64 on the CPU against the yardstick on the physical parameters it maps to, in one call and in
    two blocks."""
    import grafx_amd.processors as P

    m = P.ModulatedDelay(V, 0, Dmax, max_rate=60.0, interpolation=interp)
    gen = torch.Generator().manual_seed(3)
    z = [torch.randn(3, V, generator=gen, dtype=torch.float64) for _ in range(3)]
    z += [torch.rand(3, V, 2, generator=gen, dtype=torch.float64), 0.3 * torch.randn(3, V, 2, generator=gen, dtype=torch.float64),
          0.3 * torch.randn(3, 1, generator=gen, dtype=torch.float64)]
    x = m64.bright_rows(3, 2, 80, 4).double()
    phys = m.physical(*z)
    want, (wz, wpos) = m64.forward(x, *phys, Dmax, interp)
    got = m.torch_forward(x, *z)
    assert float((got - want).abs().max()) <= 1e-14
    a, sa = m.torch_forward(x[..., :25], *z, return_state=True)
    b, sb = m.torch_forward(x[..., 25:], *z, state=sa, return_state=True)
    assert torch.equal(torch.cat([a, b], -1), got) and torch.equal(sb[0], wz) and torch.equal(sb[1], wpos)
    assert sa[1].dtype == torch.int64 and sa[1].tolist() == [25] * 3


@pytest.mark.parametrize("Dmax", [2, 8, 441, 1764, 8192])
def test_the_read_position_is_monotone_with_runs_of_at_most_two(Dmax):
    delay, depth, rate, phase, _, _ = m64.draw_parameters(7, 4, 2, Dmax, seed=Dmax)
    assert float((2 * math.pi * rate.double() * depth.double()).max()) <= 0.5
    m = m64.read_positions(delay, depth, rate, phase, 20000, Dmax)
    step = m[..., 1:] - m[..., :-1]
    assert int(step.min()) >= 0 and int(step.max()) <= 2
    assert not bool(((step[..., 1:] == 0) & (step[..., :-1] == 0)).any())      # no value three times in a row


def test_wrappers_refuse_cpu_tensors():
    from grafx_amd import ops

    x, p2, p3, dry = torch.zeros(1, 1, 8), torch.ones(1, 1), torch.ones(1, 1, 1), torch.ones(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moddelay(x, p2, p2, p2, p3, p3, dry, 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.moddelay_bwd(x, x, p2, p2, p2, p3, p3, dry, 4)
