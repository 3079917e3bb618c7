"""gfx_dynamics_bwd_f32 on every launch path, gfx_dyn_gain_bwd_f32 and gfx_dyn_dx_f32 against the float64 yardstick of
tests/dynamics_float64.py: float64 autograd of the reference's expressions on inputs that keep clear of the jumps of the
gradient (tests/test_dynamics_float64.py asserts that on the CPU).  Every path is held to the same float64 arrays, so no two
paths differ by more than twice the bound."""
import functools

import pytest
import torch
from conftest import NORTH_STAR_TOL, assert_close_rows, assert_parity, rel_err_rows

import dynamics_float64 as f64

pytestmark = pytest.mark.gpu
TOL = NORTH_STAR_TOL      # what the compressor's gradients meet through the goldens

# kept scan on the row kernel | kept scan on the one-shot tiles | scan rebuilt inside the tiles | scan rebuilt by its own pass
PATHS = ("kept-rows", "kept-oneshot", "rescan-tiles", "rescan-pass")
# the case of every path whose gx goes into a NaN-filled strided (B, n, C, L) view: two workgroup tiles and a ragged
# float4, stereo -- rows 0 .. 2 on the tiles (where the path has them), rows 3 .. 5 on the row kernel
STRIDED = (4100, 257, "hard", False, 2)

# (case: row) whose pole gradient cannot be held to 1e-5 of its own value: in these rows it is what is left of terms of
# both signs -- sum |t| / |sum t| over the samples' terms t = dL/denv d env/da, in float64: 199, 67, 301 and 340, against 1 .. 16
# in the rows that meet the bound -- so a float32 evaluation that is good to 2e-7 of the terms is 1.3e-5 .. 6.4e-5 of the
# remainder away.  These comparisons go through conftest.assert_parity instead: the kernel has to be at least as close to
# float64 as float32 torch autograd of the same expressions is (measured 4.1e-5 .. 3.9e-4).  Every other row of these cases,
# and every row of every other case, is held to 1e-5.  The tests are in tests/parity_exceptions_allowed.json by name.
TIE_BREAK = {(2048, 257, "hard", True, 1): 2, (2999, 257, "exponential", True, 2): 3,
             (4100, 4001, "quadratic", True, 1): 3, (4100, 4001, "exponential", True, 2): 3}


def _id(v):
    return "gate" if v is True else "comp" if v is False else str(v)


def _spec_id(spec):
    return "-".join(map(_id, spec))


@functools.lru_cache(maxsize=None)
def _on_gpu(spec):
    """The case's float32 tensors on the GPU (log_knee None for the hard knees, as the processors call the ops)."""
    c = f64.case(*spec) if len(spec) == 5 else f64.gain_case(*spec)
    d = {k: None if v is None else v.cuda() for k, v in c._asdict().items() if isinstance(v, torch.Tensor) or v is None}
    if c.knee == "hard":
        d["log_knee"] = None
    return c, d


def _rows(t):
    """Per-row scalars as (R, 1): each taken against its own size by the per-row metric."""
    return t.reshape(-1, 1)


def _check(got, want, what):
    """A float32 result against float64, every row (last axis) against its own peak; the figures are printed first."""
    got = got.detach().cpu()
    err = (got.double() - want).reshape(-1, want.shape[-1]).abs().amax(-1) / want.reshape(-1, want.shape[-1]).abs().amax(-1)
    peak, l2 = rel_err_rows(got, want)
    print(f"{what}: worst row peak-rel {peak:.2e} rel-L2 {l2:.2e} | rows " + " ".join(f"{v:.1e}" for v in err.tolist()))
    assert_close_rows(got, want, TOL, what)


@functools.lru_cache(maxsize=None)
def _dalpha32(spec):
    """float32 torch autograd of the same expressions on the GPU (the partner of test_gpu_autograd.py::
    test_native_dynamics_backward_matches_torch_autograd_of_the_same_formulas), with the clamped pole as the leaf."""
    from grafx_amd import autograd as diff

    c, d = _on_gpu(spec)
    a = torch.sigmoid(d["z"]).clamp(max=1 - 1e-5).requires_grad_(True)
    h = (1 - a) * torch.exp(torch.arange(c.N, device="cuda")[None, :] * torch.log(a))      # diff.one_pole_fir behind the clamp
    e = torch.relu(diff.convolve(d["x"].square().mean(-2), h, "causal", exact=True))
    g = diff.log_gain(torch.log(e + 1e-5), d["log_threshold"] - 6, d["log_ratio"], c.log_knee.cuda(), c.knee, c.gate)
    return torch.autograd.grad((torch.exp(g)[:, None, :] * d["x"] * d["w"]).sum(), a)[0].reshape(-1).cpu()


def _backward(path, c, d, out=None, pole=True):
    from grafx_amd import ops

    p = (d["log_threshold"], d["log_ratio"], d["log_knee"], d["z"])
    if path.startswith("kept"):
        schedule = "rows" if path == "kept-rows" else "oneshot"
        u1 = torch.full(d["x"].shape[::2], float("nan"), device="cuda")
        ops.dynamics_fused(d["x"], *p, smoother=1, iir_len=c.N, knee=c.knee, gate=c.gate, schedule=schedule, u1_out=u1)
        return ops.dynamics_bwd(d["x"], d["w"], *p, c.N, c.knee, c.gate, out=out, pole=pole, u1=u1, schedule=schedule)
    return ops.dynamics_bwd(d["x"], d["w"], *p, c.N, c.knee, c.gate, out=out, pole=pole, rescan=path == "rescan-tiles")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("spec", f64.SMOOTHED, ids=_spec_id)
def test_dynamics_bwd_matches_float64_autograd(spec, path):
    """gx, every column of gparams and dalpha (the derivative with respect to the CLAMPED pole, as the op documents -- also
    in the row whose clamp is active; the chain rule's zero is DynamicsFn's, tests/test_gpu_training_paths.py) of six rows
    with poles from instant to the clamp, to 1e-5 of each row's own peak."""
    c, d = _on_gpu(spec)
    want = f64.grads(c)
    R, C, L = c.x.shape
    what = f"dynamics_bwd {_spec_id(spec)} {path}"
    if spec == STRIDED:
        buf = torch.full((2, R // 2 + 2, C, L), float("nan"), device="cuda")
        gx, gp, da = _backward(path, c, d, out=buf[:, 1:-1])
        assert bool(torch.isnan(buf[:, 0]).all()) and bool(torch.isnan(buf[:, -1]).all()), "written outside the view"
        gx = gx.reshape(R, C, L)
    else:
        gx, gp, da = _backward(path, c, d)
    _check(gx, want.gx, what + " gx")
    for k, name in enumerate(("log_threshold", "log_ratio", "log_knee")):
        _check(_rows(gp[:, k]), _rows(want.gparams[:, k]), f"{what} d{name}")      # (hard knee: d/dlog_knee is exactly zero)
    keep = [r for r in range(R) if r != TIE_BREAK.get(spec)]
    _check(_rows(da[keep]), _rows(want.dalpha[keep]), what + " dalpha")
    if spec in TIE_BREAK:
        r = TIE_BREAK[spec]
        assert_parity(da[r:r + 1].cpu(), _dalpha32(spec)[r:r + 1], want.dalpha[r:r + 1], TOL, f"{what} dalpha of row {r}")


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("spec", [(4100, 257, "quadratic", False, 2), (2999, 257, "exponential", True, 1)], ids=_spec_id)
def test_dynamics_bwd_without_the_pole_gradient_matches_float64_autograd(spec, path):
    """``pole=False`` (a frozen z_alpha) is a pair of instantiations of its own in the row kernel, with and without the live
    truncation term, and a run-time branch of the tiles: gx and gparams are held to the same float64 arrays."""
    c, d = _on_gpu(spec)
    want = f64.grads(c)
    what = f"dynamics_bwd {_spec_id(spec)} {path} pole=False"
    gx, gp, da = _backward(path, c, d, pole=False)
    assert da is None
    _check(gx, want.gx, what + " gx")
    for k, name in enumerate(("log_threshold", "log_ratio", "log_knee")):
        _check(_rows(gp[:, k]), _rows(want.gparams[:, k]), f"{what} d{name}")


@pytest.mark.parametrize("spec", f64.UNSMOOTHED, ids=_spec_id)
def test_dyn_gain_bwd_matches_float64_autograd(spec):
    """The gain computer's backward (the unsmoothed DynamicsFn) on a given envelope: gain, d/d env and the parameter
    gradients against the yardstick's curve evaluated on the same float32 envelope."""
    from grafx_amd import ops

    c, d = _on_gpu(spec)
    want = f64.grads(c)
    gain, denv, gp = ops.dyn_gain_bwd(d["x"], d["w"], d["env"], d["log_threshold"], d["log_ratio"], d["log_knee"], c.knee, c.gate)
    what = f"dyn_gain_bwd {_spec_id(spec)}"
    _check(gain, want.gain, what + " gain")
    _check(denv, want.denv, what + " denv")
    for k, name in enumerate(("log_threshold", "log_ratio", "log_knee")):
        _check(_rows(gp[:, k]), _rows(want.gparams[:, k]), f"{what} d{name}")


@pytest.mark.parametrize("C", f64.CHANNELS)
@pytest.mark.parametrize("L", f64.GAIN_LENGTHS)
def test_dyn_dx_matches_float64(L, C):
    """gx = gain gy + (2 / C) de x on the float32 gain and energy gradient of a compressor case, in float64."""
    from grafx_amd import ops

    c, d = _on_gpu((L, "quadratic", False, C))
    g = f64.grads(c)
    gain, de = g.gain.float(), g.denv.float()
    want = gain.double()[:, None, :] * c.w.double() + (2 / C) * de.double()[:, None, :] * c.x.double()
    _check(ops.dyn_dx(d["x"], d["w"], gain.cuda(), de.cuda()), want, f"dyn_dx L={L} C={C}")
