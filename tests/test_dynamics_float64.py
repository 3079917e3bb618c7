"""The float64 yardstick of the dynamics backward (tests/dynamics_float64.py) and the screening of its inputs, on the CPU:
what keeps tests/test_gpu_dynamics_bwd_float64.py honest is asserted here on the inputs alone."""
import pytest
import torch

import dynamics_float64 as f64


def _id(v):
    return "gate" if v is True else "comp" if v is False else str(v)


def _case(spec):
    return f64.case(*spec) if len(spec) == 5 else f64.gain_case(*spec)


@pytest.mark.parametrize("spec", f64.SMOOTHED + f64.UNSMOOTHED, ids=lambda s: "-".join(map(_id, s)))
def test_the_inputs_keep_clear_of_the_jumps_of_the_gradient(spec):
    """Every sample of a hard-knee row is at least MARGIN away from the corner G = T (a hundred times float32's rounding
    of G), the envelope of every row is positive (the relu is the other switch; no row is silent), and every region of a
    curve that a row populates holds at least MIN_REGION of it.  An input that misses this gets another construction,
    never another threshold."""
    c = _case(spec)
    gap, floor = f64.margin(c)
    frac = f64.regions(c)
    print(f"\n{'-'.join(map(_id, spec))}: min |G - T| per row " + " ".join(f"{v:.1e}" for v in gap.tolist())
          + " | min env per row " + " ".join(f"{v:.1e}" for v in floor.tolist()))
    print("  below / inside / above the knee per row: " + "  ".join("/".join(f"{v:.2f}" for v in r) for r in frac.tolist()))
    assert float(floor.min()) > 0
    if c.knee == "hard":
        assert float(gap.min()) >= f64.MARGIN, gap.tolist()
        assert float(frac[:, 1].max()) == 0 and float(frac[:, (0, 2)].min()) >= f64.MIN_REGION, frac.tolist()
    else:
        assert float(frac.min()) >= f64.MIN_REGION, frac.tolist()
    for t in (c.x, c.w, c.log_threshold, c.log_ratio, c.log_knee):
        assert t.dtype == torch.float32 and bool(torch.isfinite(t).all())
    assert _case(spec) is c      # computed once


@pytest.mark.parametrize("L,N", [(516, 257), (2999, 257), (516, 1023), (4100, 4001)])
def test_the_written_fir_is_the_truncated_recursion(L, N):
    x, _, z, _ = f64._smoothed_signal(L, N, 2)
    e, a = x.double().square().mean(-2), f64.pole(z)
    got, want = f64.smooth(e, a, N), f64.smooth_by_recursion(e, a, N)
    err = (got - want).abs().amax(-1) / want.abs().amax(-1)
    assert float(err.max()) <= 1e-12, err.tolist()
    assert float(a[-1]) == f64.A_MAX and float(a[0]) < 1e-8          # the clamp is active in the last row only
    assert bool((a[:-1] < f64.A_MAX).all())


@pytest.mark.parametrize("gate", [False, True], ids=_id)
@pytest.mark.parametrize("knee", f64.KNEES)
def test_autograd_of_the_pole_is_a_central_difference(knee, gate):
    """dalpha of the yardstick against the five-point central difference in float64, every row against its own value.
    Bound: the step h (dynamics_float64.dalpha_by_differences) is at most 1e-5 of the scale on which the sum varies with a,
    so the truncation error, of the order of that ratio's fourth power, is nothing (4e-11 for the instant row: 1e-7 on a scale
    of 4e-5); the rounding error is 1e-16 sqrt(516) |y w| / h = 1e-15 / h, i.e. 1e-8 against derivatives of 0.3 and more
    (1e-5 against 4e3 and more in the clamped row); a sample of the clamped row that crosses an end of the quadratic knee
    inside the stencil adds (1 / 516) (h / (1 - a)) / W, about 1e-7, and its stencil points a + k h are themselves rounded
    to 1e-16, 5e-7 of its step of 1e-10 at the most.  1e-6 holds all of that, and a wrong term of the
    derivative is wrong by its whole size."""
    c = f64.case(516, 257, knee, gate, 1)
    got, want = f64.grads(c).dalpha, f64.dalpha_by_differences(c)
    err = (got - want).abs() / want.abs()
    print(f"\n{knee} {_id(gate)}: dalpha " + " ".join(f"{v:.3e}" for v in got.tolist()) + " | rel. difference "
          + " ".join(f"{v:.1e}" for v in err.tolist()))
    assert float(err.max()) <= 1e-6, err.tolist()


@pytest.mark.parametrize("gate", [False, True], ids=_id)
@pytest.mark.parametrize("knee", f64.KNEES)
def test_the_forward_is_the_oracle_processor(knee, gate):
    """The yardstick's forward on doubles against the CPU oracle's processor with the "iir" smoother on the same float32
    inputs (an FFT convolution in float32, hence 1e-5 and not more)."""
    import oracle

    c = f64.case(516, 257, knee, gate, 2)
    y = f64.grads(c).y
    m = (oracle.OracleNoiseGate if gate else oracle.OracleCompressor)(energy_smoother="iir", knee=knee, iir_len=c.N)
    want = m(c.x, c.log_threshold, c.log_ratio, c.log_knee, c.z)
    err = (y - want.double()).abs().amax((-2, -1)) / want.double().abs().amax((-2, -1))
    assert float(err.max()) <= 1e-5, err.tolist()
