"""The feedback delay without a GPU: the four C entries are declared, bound and exported with their argument lists; the
workspace queries return the documented sizes and 0 for bad arguments; every refusal of the entries comes back before a
launch; the constructor takes what is documented and ``physical()`` stays inside the kernels' contract; the float64
yardstick agrees with a brute-force loop, its autograd with the written adjoint, its blocks with its one call;
``torch_forward`` is the yardstick; and an impulse through an integer delay gives the closed-form echoes, straight and
ping-pong."""
import numpy as np
import pytest
import torch

import fbdelay_float64 as f64
from abi_checks import device_pointer, entries_match, refused

ENTRIES = ("gfx_fbdelay_ws_bytes", "gfx_fbdelay_f32", "gfx_fbdelay_bwd_ws_bytes", "gfx_fbdelay_bwd_f32")
# R, C, Dmax, L of the small float64 checks: the loop goes round several times
SMALL = ((4, 2, 128, 420), (3, 1, 100, 400), (4, 2, 77, 300))


def test_the_entries_are_declared_bound_and_exported():
    cf, f = "const float*", "float*"
    fwd = [cf, "gfx_rowmap_t", f, "gfx_rowmap_t"] + ["int64_t"] * 4 + [cf] * 5 + [cf, cf, f, f, f, "void*", "size_t", "void*"]
    bwd = ([cf, "gfx_rowmap_t", cf, "gfx_rowmap_t", cf, cf] + ["int64_t"] * 4 + [cf] * 5 + [f, "gfx_rowmap_t"] + [f] * 5
           + ["void*", "size_t", "void*"])
    entries_match(ENTRIES, dict(zip(ENTRIES, (("size_t", ["int64_t"] * 3), ("int", fwd), ("size_t", ["int64_t"] * 3),
                                              ("int", bwd)))))


def test_constants_and_workspace_queries():
    from grafx_amd import _lib, ops

    assert (ops.FBDELAY_MIN_DELAY, ops.FBDELAY_MAX_DELAY) == (64, 65536)
    assert ops.FBDELAY_GRADS == ("x", "delay", "damping", "feedback", "dry", "wet")
    assert ops.FBDELAY_CHUNK % 256 == 0 and ops.FBDELAY_CHUNK >= 256
    fwd, bwd = _lib.lib().gfx_fbdelay_ws_bytes, _lib.lib().gfx_fbdelay_bwd_ws_bytes
    for R, C, L in ((1, 1, 1), (3, 2, 4097), (2, 2, 4096), (70000, 1, 40), (256, 2, 131072)):
        assert fwd(R, C, L) == 4 * R * C * L, (R, C, L)
        assert bwd(R, C, L) == 8 * R * -(-L // 2048) * (2 + 2 * C + C * C) + 4 * R * C * L, (R, C, L)
    for bad in ((0, 2, 100), (-1, 2, 100), (2, 0, 100), (2, 3, 100), (2, 2, 0), (2, 2, -5)):
        assert fwd(*bad) == 0 and bwd(*bad) == 0, bad


def test_entries_refuse_bad_arguments_before_any_launch():
    """Every check comes before the first launch, so the refusals need no GPU (abi_checks.device_pointer)."""
    from grafx_amd import _lib

    lib = _lib.lib()
    R, C, L, Dmax = 3, 2, 5000, 441
    S = Dmax + 1
    need, need_bwd = lib.gfx_fbdelay_ws_bytes(R, C, L), lib.gfx_fbdelay_bwd_ws_bytes(R, C, L)
    p, _held = device_pointer()
    sig = 4 * R * C * L
    far, third, qs, wsig, wsp = (p + k * sig for k in range(1, 6))            # signals that do not overlap, then the workspace
    z0 = wsp + need_bwd + 64
    z1 = z0 + 4 * R * C * S
    q0 = z1 + 4 * R * C * S
    q1 = q0 + 4 * R * C
    assert q1 + 4 * R * C - p <= 4 * (1 << 22)
    rm, empty, neg = _lib.RowMap(R, 0, C * L, L), _lib.RowMap(0, 0, C * L, L), _lib.RowMap(R, 0, -C * L, L)
    five = dict(delay=p, damping=p, feedback=p, dry=p, wet=p)
    fwd = dict(x=p, xmap=rm, y=far, ymap=rm, R=R, C=C, L=L, max_delay=Dmax, **five, zi=None, q_in=None, zf=None, q_out=None,
               q=None, ws=wsp, ws_bytes=need, stream=None)
    bwd = dict(x=p, xmap=rm, gy=far, gmap=rm, q=qs, w=wsig, R=R, C=C, L=L, max_delay=Dmax, **five, gx=third, gxmap=rm,
               g_delay=p, g_damping=p, g_feedback=p, g_dry=p, g_wet=p, ws=wsp, ws_bytes=need_bwd, stream=None)
    bad = {
        "no signal": dict(x=None), "an empty row map": dict(xmap=empty), "no rows": dict(R=0), "negative rows": dict(R=-3),
        "no channels": dict(C=0), "three channels": dict(C=3), "no samples": dict(L=0), "negative length": dict(L=-5),
        "a delay line of 63": dict(max_delay=63), "a delay line of 65537": dict(max_delay=65537),
        **{f"no {name}": {name: None} for name in five},
        "more than 2^31 - 1 rows": dict(R=1 << 31, L=1), "a negative stride": dict(xmap=neg),
        "no workspace": dict(ws=None), "a misaligned workspace": dict(ws=wsp + 2),
    }
    only_fwd = {"no output": dict(y=None), "an empty output row map": dict(ymap=empty), "an output that is the input": dict(y=p),
                "an output that overlaps the input": dict(y=p + 4), "a negative output stride": dict(ymap=neg),
                "a history without q_in": dict(zi=z0), "q_in without a history": dict(q_in=q0),
                "a new history without q_out": dict(zf=z1), "q_out alone": dict(q_out=q1),
                "zf is zi": dict(zi=z0, q_in=q0, zf=z0, q_out=q1),
                "zf overlaps zi": dict(zi=z0, q_in=q0, zf=z0 + 4 * (R * C * S - 1), q_out=q1),
                "a workspace that is the input": dict(ws=p), "a workspace that is the output": dict(ws=far)}
    only_bwd = {"no output gradient": dict(gy=None), "an empty gradient row map": dict(gmap=empty), "no q": dict(q=None),
                "no w": dict(w=None), "nothing asked for": dict(gx=None, **{"g_" + name: None for name in five}),
                "gx is x": dict(gx=p), "gx is gy": dict(gx=far), "gx overlaps x a sample later": dict(gx=p + 4),
                "an empty gx row map": dict(gxmap=empty), "a workspace that is not 8-byte aligned": dict(ws=wsp + 4)}
    refused(lib.gfx_fbdelay_f32, fwd, {**bad, **only_fwd})
    refused(lib.gfx_fbdelay_bwd_f32, bwd, {**bad, **only_bwd})
    refused(lib.gfx_fbdelay_f32, fwd, {"a workspace one byte short": dict(ws_bytes=need - 1)}, code=-2)
    refused(lib.gfx_fbdelay_bwd_f32, bwd, {"a workspace one byte short": dict(ws_bytes=need_bwd - 1)}, code=-2)


def test_constructor_and_parameter_size():
    import grafx_amd.processors as P

    m = P.FeedbackDelay()
    assert (m.min_delay, m.max_delay, m.max_feedback, m.max_damping) == (64, 22050, 0.95, 0.95)
    assert (m.processor_channel, m.num_channels, m.latency, m.state_samples) == ("stereo", 2, 0, 22051)
    assert m.parameter_size() == {"z_delay": 2, "z_feedback": 1, "z_cross": 1, "z_damping": 2, "log_wet": 1, "log_dry": 1}
    assert m.state_dict() == {} and m.accepts_strided_rows
    m.stream_check()
    mono = P.FeedbackDelay(64, 65536, processor_channel="mono")
    assert mono.parameter_size() == {"z_delay": 1, "z_feedback": 1, "z_damping": 1, "log_wet": 1, "log_dry": 1}
    assert mono.state_samples == 65537
    for kwargs, why in ((dict(max_delay=65537), "65536 at most"), (dict(min_delay=63), ">= 64"), (dict(min_delay=22050), "below max_delay"),
                        (dict(min_delay=30000), "below max_delay"), (dict(max_feedback=1.0), r"inside \(0, 1\)"),
                        (dict(max_feedback=0.0), r"inside \(0, 1\)"), (dict(max_damping=1.5), r"inside \(0, 1\)"),
                        (dict(max_damping=-0.1), r"inside \(0, 1\)"), (dict(max_damping=True), r"inside \(0, 1\)"),
                        (dict(min_delay=64.0), "integer"), (dict(max_delay=1000.5), "integer"), (dict(max_delay=True), "integer"),
                        (dict(processor_channel="midside"), "'mono' or 'stereo'"), (dict(min_delay=64, max_delay=65), None)):
        if why is None:
            P.FeedbackDelay(**kwargs)
            continue
        with pytest.raises(ValueError, match=why):
            P.FeedbackDelay(**kwargs)


@pytest.mark.parametrize("kwargs", [dict(), dict(min_delay=64, max_delay=65536), dict(min_delay=64, max_delay=65),
                                    dict(min_delay=100, max_delay=128, max_feedback=0.999, max_damping=0.999),
                                    dict(processor_channel="mono", max_feedback=0.5)])
def test_physical_stays_inside_the_contract(kwargs):
    """For z at +-30 and everything between, in float32: the delay inside [max(64, min_delay), max_delay], 0 <= a < 1 and
    every row sum of |F| < 1, evaluated in float64 on the float32 values the kernel gets."""
    import grafx_amd.processors as P

    m = P.FeedbackDelay(**kwargs)
    C = m.num_channels
    grid = torch.tensor([-30.0, -8.0, -1.0, 0.0, 0.5, 3.0, 12.0, 30.0])
    zd, zf, zc, za = (t.reshape(-1, 1) for t in torch.meshgrid(grid, grid, grid, grid, indexing="ij"))
    R = zd.shape[0]
    z = dict(z_delay=zd.expand(R, C), z_feedback=zf, z_damping=za.expand(R, C), log_wet=torch.zeros(R, 1), log_dry=torch.zeros(R, 1))
    if C == 2:
        z["z_cross"] = zc
    delay, a, F, dry, wet = m.physical(**z)
    assert all(t.dtype == torch.float32 for t in (delay, a, F, dry, wet))
    assert (tuple(delay.shape), tuple(a.shape), tuple(F.shape), tuple(dry.shape), tuple(wet.shape)) == ((R, C), (R, C), (R, C, C), (R,), (R,))
    delay, a, F = delay.double(), a.double(), F.double()
    assert float(delay.min()) >= max(64, m.min_delay) and float(delay.max()) <= m.max_delay
    assert float(delay.max()) - float(delay.min()) > 0.99 * (m.max_delay - m.min_delay)                 # (and it does move)
    assert float(a.min()) >= 0 and float(a.max()) < 1 and float(a.max()) > 0.99 * m.max_damping
    rows = F.abs().sum(-1)
    assert float(rows.max()) < 1 and float(rows.max()) > 0.99 * m.max_feedback and float(F.min()) >= 0
    assert torch.equal(dry, torch.ones(R)) and torch.equal(wet, torch.ones(R))


def _case(R, C, Dmax, L, seed):
    return f64.bright_rows(R, C, L, seed), f64.draw_parameters(R, C, Dmax, seed + 100)


@pytest.mark.parametrize("R,C,Dmax,L", SMALL)
def test_the_yardstick_agrees_with_a_brute_force_loop(R, C, Dmax, L):
    x, params = _case(R, C, Dmax, L, seed=R + Dmax)
    y, (zf, ql), (q, w) = f64.forward(x, *params, Dmax, signals=True)
    by, bq, bw, _ = f64.brute(x, *params, Dmax, signals=True)
    assert np.abs(y.numpy() - by).max() <= 1e-12 and np.abs(q.numpy() - bq).max() <= 1e-12
    assert np.abs(w.numpy() - bw).max() <= 1e-12
    assert torch.equal(zf, w[..., -(Dmax + 1):]) and torch.equal(ql, q[..., -1])
    gen = torch.Generator().manual_seed(1)
    state = (torch.randn(R, C, Dmax + 1, generator=gen), torch.randn(R, C, generator=gen))
    y, (zf, ql) = f64.forward(x, *params, Dmax, state)
    assert np.abs(y.numpy() - f64.brute(x, *params, Dmax, state)).max() <= 1e-12
    short, (zs, _) = f64.forward(x[..., :50], *params, Dmax, state)           # shorter than the history: it shifts
    assert torch.equal(short, y[..., :50]) and torch.equal(zs[..., :-50], state[0].double()[..., 50:])


@pytest.mark.parametrize("R,C,Dmax,L", SMALL)
def test_autograd_of_the_yardstick_agrees_with_the_written_adjoint(R, C, Dmax, L):
    x, params = _case(R, C, Dmax, L, seed=10 + R + Dmax)
    g = torch.randn(x.shape, generator=torch.Generator().manual_seed(2), dtype=torch.float64)
    auto = f64.gradients(x, g, *params, Dmax)
    written = f64.adjoint(x, g, *params, Dmax)
    for name, a, w in zip(f64.NAMES, auto, written):
        assert a.shape == w.shape, name
        assert np.abs(a.numpy() - w).max() <= 1e-11 * np.abs(w).max(), name
        assert np.abs(w).max() > 0 and bool((np.abs(w).reshape(R, -1).max(-1) > 0).all()), name


@pytest.mark.parametrize("R,C,Dmax,L", [(4, 2, 128, 200), (3, 1, 100, 200), (4, 2, 77, 200)])
def test_blocks_concatenate_to_the_one_call(R, C, Dmax, L):
    x, params = _case(R, C, Dmax, L, seed=20)
    whole, (wz, wq) = f64.forward(x, *params, Dmax)
    ys, state, at = [], None, 0
    for n in (7, 1, 120, 72):
        y, state = f64.forward(x[..., at:at + n], *params, Dmax, state)
        ys.append(y)
        at += n
    assert at == L
    assert float((torch.cat(ys, -1) - whole).abs().max()) <= 1e-13
    assert float((state[0] - wz).abs().max()) <= 1e-13 and float((state[1] - wq).abs().max()) <= 1e-13


@pytest.mark.parametrize("channel,Dmax", [("stereo", 128), ("mono", 100), ("stereo", 77)])
def test_torch_forward_is_the_definition(channel, Dmax):
    """torch_forward in float64 on the CPU against the yardstick on the physical parameters it maps to, in one call and in
    two blocks; it is differentiable in every parameter."""
    import grafx_amd.processors as P

    m = P.FeedbackDelay(64, Dmax, processor_channel=channel)
    C, R, L = m.num_channels, 3, 400
    gen = torch.Generator().manual_seed(3)
    z = {k: torch.randn(R, n, generator=gen, dtype=torch.float64) * (0.3 if k.startswith("log") else 1.0)
         for k, n in m.parameter_size().items()}
    x = f64.bright_rows(R, C, L, 4).double()
    phys = m.physical(**z)
    want, (wz, wq) = f64.forward(x, *phys, Dmax)
    got = m.torch_forward(x, **z)
    assert float((got - want).abs().max()) <= 1e-13
    a, sa = m.torch_forward(x[..., :150], **z, return_state=True)
    b, sb = m.torch_forward(x[..., 150:], **z, state=sa, return_state=True)
    assert float((torch.cat([a, b], -1) - got).abs().max()) <= 1e-13
    assert float((sb[0] - wz).abs().max()) <= 1e-13 and float((sb[1] - wq).abs().max()) <= 1e-13
    assert sa[0].shape == (R, C, Dmax + 1) and sa[1].shape == (R, C)
    leaves = {k: v.clone().requires_grad_(True) for k, v in z.items()}
    m.torch_forward(x, **leaves).square().sum().backward()
    assert all(v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0 for v in leaves.values())


def _impulse_setup(C, D0, D1, fb, cross, wet):
    L = 5 * (D0 + D1)
    x = torch.zeros(1, C, L)
    x[0, 0, 0] = 1.0
    delay = torch.tensor([[float(D0), float(D1)][:C]])
    F = fb * torch.tensor([[[1 - cross, cross], [cross, 1 - cross]]])[:, :C, :C] if C == 2 else torch.full((1, 1, 1), fb)
    return x, (delay, torch.zeros(1, C), F, torch.tensor([0.0]), torch.tensor([wet])), L


def test_an_impulse_echoes_in_closed_form():
    """An integer delay D without damping or cross feed: y[k D] = wet fb^(k - 1), zero elsewhere."""
    D, fb, wet = 70, 0.5, 0.75
    for C in (1, 2):
        x, params, L = _impulse_setup(C, D, 90, fb, 0.0, wet)
        y, _ = f64.forward(x, *params, 128)
        want = torch.zeros(1, C, L, dtype=torch.float64)
        for k in range(1, (L - 1) // D + 1):
            want[0, 0, k * D] = wet * fb ** (k - 1)
        assert float((y - want).abs().max()) <= 1e-15


def test_a_ping_pong_alternates_the_channels():
    """cross = 1: the impulse of channel 0 comes out of channel 0 after D0, of channel 1 after D0 + D1, of channel 0 after
    2 D0 + D1, ..., each echo fb times the one before."""
    D0, D1, fb, wet = 70, 90, 0.5, 0.75
    x, params, L = _impulse_setup(2, D0, D1, fb, 1.0, wet)
    y, _ = f64.forward(x, *params, 128)
    want = torch.zeros(1, 2, L, dtype=torch.float64)
    at, k = D0, 0
    while at < L:
        want[0, k % 2, at] = wet * fb ** k
        k += 1
        at += D1 if k % 2 else D0
    assert k >= 5 and float((y - want).abs().max()) <= 1e-15


def test_wrappers_refuse_cpu_tensors():
    from grafx_amd import ops

    x, p2, p3, one = torch.zeros(1, 1, 8), torch.full((1, 1), 64.0), torch.zeros(1, 1, 1), torch.ones(1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fbdelay(x, p2, p3[0], p3, one, one, 64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.fbdelay_bwd(x, x, x, x, p2, p3[0], p3, one, one, 64)
