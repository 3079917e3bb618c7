"""The two-rows-per-transform aliasing (csrc/czt_pair.hip) at the bottom of the float range: a row near 1e-37 next to a row
at unit level, both rows near 1e-37, and a partner 2^-100 or 2^60 away (reference: core/convolution.py:119-134,
y = irfft_{P-1}(rfft_P(z)); here torch.fft in float64 on the float32-rounded rows).

One complex transform carries both rows of a pair, brought to one binade by an exact power of two (pair_scale).  Whichever
row is the quiet one, EVERY row is held to its own peak -- never the pair's -- and to what the one-row transforms of czt.hip
(ops.ALIAS_PAIRS = False: the reference's independent rows) give on the same input.  Sizes: 4001 (one tile), 135 071
(35 tiles: czt_pair_in / mid / out), 299 999 (the fused outer radix-4 level), 1 000 001 (two outer levels).

Every test prints its figures (row, error over the row's own peak) before it asserts: run with -s to read them."""
import pytest
import torch

pytestmark = pytest.mark.gpu

Q_LEVELS = [1e-20, 1e-30, 1e-35, 1e-37]
PRECISE_TOL = 1.5e-7                 # tests/test_gpu_odd_alias_pair.py: the double-precision form, for P < 500 000


def _want(z):
    return torch.fft.irfft(torch.fft.rfft(z.double()))


def _tol(P):
    return 3e-6 if P < 700000 else 5e-6       # the standing bounds of tests/test_gpu_odd_alias_pair.py


def _one_row_form(fn):
    from grafx_amd import ops

    old = ops.ALIAS_PAIRS
    ops.ALIAS_PAIRS = False
    try:
        return fn()
    finally:
        ops.ALIAS_PAIRS = old


def _row_errors(got, want):
    """max |got - want| of every row over the row's OWN peak (float64)."""
    return (got.double() - want).abs().amax(-1) / want.abs().amax(-1)


def _report(tag, rel):
    print(f"\n  {tag}: " + " ".join(f"{float(e):.2e}" for e in rel.flatten()), end="")


# ---- (a) a row at unit level and a row at q in one pair -------------------------------------------------------------------
@pytest.mark.parametrize("q", Q_LEVELS)
@pytest.mark.parametrize("P", [4001, 135071, 299999, 1000001])
def test_a_row_near_the_bottom_of_the_range_next_to_a_row_at_unit_level(P, q):
    """Pair (0, 1) has the quiet row second, pair (2, 3) has it first, row 4 is alone in its transform.  The float form, the
    double-precision form (with and without its fused clamp) and the one-row forms: every row within the standing bound
    of ITS OWN peak."""
    from grafx_amd import ops

    torch.manual_seed(1)
    z = torch.randn(5, P, device="cuda")
    z[1] *= q                    # float32 first: the reference below is that of the rounded rows
    z[2] *= q
    want = _want(z)
    figures = {"pair": _row_errors(ops.odd_alias(z), want),
               "one-row": _row_errors(_one_row_form(lambda: ops.odd_alias(z)), want)}
    bounds = {"pair": _tol(P), "one-row": _tol(P)}
    if P < 500000:
        figures["pair precise"] = _row_errors(ops.odd_alias(z, precise=True), want)
        figures["one-row precise"] = _row_errors(_one_row_form(lambda: ops.odd_alias(z, precise=True)), want)
        clamped = want.clamp_min(0)
        figures["pair precise relu"] = ((ops.odd_alias(z, precise=True, relu=True).double() - clamped).abs().amax(-1)
                                        / want.abs().amax(-1))
        bounds.update({"pair precise": PRECISE_TOL, "one-row precise": PRECISE_TOL, "pair precise relu": PRECISE_TOL})
    for form, rel in figures.items():
        _report(f"P={P} q={q:g} {form}", rel)
    for form, rel in figures.items():
        for r in range(5):
            assert float(rel[r]) <= bounds[form], f"{form}, row {r}: {float(rel[r]):.2e} of its own peak (q = {q:g})"


# ---- (b) both rows of a pair at q: no relative scaling can help, the pair may not be worse than one transform per row ----
@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("q", Q_LEVELS)
@pytest.mark.parametrize("P", [4001, 135071, 299999])
def test_two_quiet_rows_in_a_pair_are_no_worse_than_each_alone(P, q, precise):
    """err_pair <= max(bound x peak, 2 x err_one_row) for every row: one complex transform carries both rows' rounding, and
    aligning binades leaves up to a factor 2 between the components."""
    from grafx_amd import ops

    torch.manual_seed(2)
    z = torch.randn(4, P, device="cuda") * q
    want = _want(z)
    pair = _row_errors(ops.odd_alias(z, precise=precise), want)
    alone = _row_errors(_one_row_form(lambda: ops.odd_alias(z, precise=precise)), want)
    _report(f"P={P} q={q:g} precise={precise} pair", pair)
    _report(f"P={P} q={q:g} precise={precise} one-row", alone)
    bound = PRECISE_TOL if precise else _tol(P)
    for r in range(4):
        assert float(pair[r]) <= max(bound, 2 * float(alone[r])), \
            f"row {r}: pair {float(pair[r]):.2e}, one-row {float(alone[r]):.2e} of its own peak (q = {q:g})"


# ---- (c) a row's bits do not depend on how quiet (or loud) its partner is ------------------------------------------------
@pytest.mark.parametrize("precise", [False, True])
@pytest.mark.parametrize("k", [-100, -60, 60])
@pytest.mark.parametrize("P", [4001, 135071, 299999])
def test_a_partner_far_down_or_up_the_range_changes_no_bit(P, k, precise):
    """2^k on one row of a pair multiplies that row of the result by 2^k, bit for bit, and leaves its partner's bits alone,
    for either row.  2^-100 keeps every randn sample a normal float (exactness is a fair demand); 2^60 guards the scale
    against overflow."""
    from grafx_amd import ops

    torch.manual_seed(P)
    z = torch.randn(2, P, device="cuda")
    lo, n = (7, 5000) if P > 5007 else (7, None)
    base = ops.odd_alias(z, lo, n, precise=precise)
    for row in (0, 1):
        zz = z.clone()
        zz[row] *= 2.0 ** k
        got = ops.odd_alias(zz, lo, n, precise=precise)
        partner = 1 - row
        moved = int((got[partner] != base[partner]).sum()), int((got[row] != base[row] * 2.0 ** k).sum())
        print(f"\n  P={P} k={k} precise={precise} row {row}: {moved[0]} samples of the partner and {moved[1]} of the row differ", end="")
        assert torch.equal(got[partner], base[partner]), (row, k)
        assert torch.equal(got[row], base[row] * 2.0 ** k), (row, k)


# ---- (d) the rows' maxima supplied by the convolution kernel -------------------------------------------------------------
LEVELS = [1e-33, 1.0, 1.0, 1e-33, 1.0]      # pair (0, 1): the quiet row first; pair (2, 3): second; row 4 alone
CONV_TOL = 1e-5                              # the convolution tests' bound (tests/test_gpu_fftconv.py), per row here
CONV_SHAPES = [(3000, 1002), (131072, 4000)]                    # P = 4001 and 135 071


def _levelled(L, N):
    torch.manual_seed(L + N)
    x = torch.randn(5, 1, L, device="cuda") * torch.tensor(LEVELS, device="cuda")[:, None, None]
    h = torch.randn(5, 1, N, device="cuda") / N ** 0.5
    return x, h


def _aliased_convolution_f64(x, h):
    """oracle.lti.convolve in float64: the reference's convolve() (core/convolution.py:119-134), all P - 1 samples."""
    from oracle import lti

    return lti.convolve(x.double(), h.double(), "full")


@pytest.mark.parametrize("L,N", CONV_SHAPES)
def test_supplied_maxima_of_rows_at_very_different_levels(L, N):
    """The console's route to gfx_odd_alias_pair_f32 with given row maxima: the full-length convolution leaves max |z| of
    its rows, the aliasing takes the words.  Per row against the float64 aliasing of the float64 linear convolution;
    into a strided (B, n, C, L) view the same bits; slices are ranges of the full result."""
    from grafx_amd import ops

    x, h = _levelled(L, N)
    rm = {}
    z = ops.fftconv(x, ops.fir_spectrum(h.reshape(5, N)), N, 1, Lout=L + N - 1, rowmax=rm)
    assert "words" in rm
    assert torch.equal(rm["words"].view(torch.float32).view(5, 1), z.abs().amax(-1))
    got = ops.odd_alias(z, 0, L, rowmax=rm["words"])
    want = _aliased_convolution_f64(x, h)[..., :L]
    rel = _row_errors(got, want)
    _report(f"L={L} N={N} supplied maxima", rel)
    buf = torch.zeros(1, 8, 1, L, device="cuda")
    ops.odd_alias(z, 0, L, out=buf[:, 2:7], rowmax=rm["words"])
    lo, n = L // 3, L // 5
    part = ops.odd_alias(z, lo, n, rowmax=rm["words"])
    for r in range(5):
        assert float(rel[r]) <= CONV_TOL, f"row {r} (level {LEVELS[r]:g}): {float(rel[r]):.2e} of its own peak"
    assert torch.equal(buf[0, 2:7], got)
    assert float(buf[:, :2].abs().max()) == 0.0 and float(buf[:, 7:].abs().max()) == 0.0
    assert torch.equal(part, got[..., lo : lo + n])


# ---- (e) through the processors ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,N", CONV_SHAPES)
def test_processors_keep_every_rows_own_error_at_very_different_levels(L, N):
    """convolve(mode="causal") and FIRConvolution(mode="zerophase") at an odd L + N - 1 (the aliasing path, pairs of rows)
    per row against oracle.lti.convolve in float64, at the convolution tests' bound of the row's own peak."""
    from grafx_amd.processors.core.convolution import FIRConvolution, convolve
    from oracle import lti

    assert (L + N - 1) % 2 == 1
    x, h = _levelled(L, N)
    with torch.no_grad():
        causal = convolve(x, h, mode="causal")
        zero = FIRConvolution(mode="zerophase", flashfftconv=False)(x, h)
    rel_c = _row_errors(causal, lti.convolve(x.double(), h.double(), "causal"))
    rel_z = _row_errors(zero, lti.convolve(x.double(), h.double(), "zerophase"))
    _report(f"L={L} N={N} convolve causal", rel_c)
    _report(f"L={L} N={N} FIRConvolution zerophase", rel_z)
    for r in range(5):
        assert float(rel_c[r]) <= CONV_TOL, f"causal, row {r} (level {LEVELS[r]:g}): {float(rel_c[r]):.2e}"
        assert float(rel_z[r]) <= CONV_TOL, f"zerophase, row {r} (level {LEVELS[r]:g}): {float(rel_z[r]):.2e}"


# ---- beyond the transforms' range: the message that names the way out ----------------------------------------------------
def test_a_length_beyond_the_transforms_raises_the_error_that_names_the_way_out():
    """P = 11 184 813, one past the largest length of the chirp-z plans: convolve() and the in-place form of
    convolve_taps() raise the NotImplementedError of odd_length_alias(), not the plan build's status code; under
    set_exact_convolution(True) the same call is a plain linear convolution and returns."""
    from grafx_amd import ops
    from grafx_amd.processors.core.convolution import convolve, convolve_taps, set_exact_convolution

    L, N = 11184800, 14
    assert not ops.odd_alias_supported(L + N - 1) and ops.odd_alias_supported(L + N - 3)
    torch.manual_seed(0)
    x = torch.randn(1, 1, L, device="cuda")
    h = torch.randn(1, 1, N, device="cuda")
    Hs = ops.fir_spectrum(h.reshape(1, N))
    out = torch.empty_like(x)
    with torch.no_grad():
        with pytest.raises(NotImplementedError, match="set_exact_convolution"):
            convolve(x, h, mode="causal")
        with pytest.raises(NotImplementedError, match="set_exact_convolution"):
            convolve_taps(x, Hs, N, 1, "causal", out=out)
        set_exact_convolution(True)
        try:
            y = convolve(x, h, mode="causal")
            assert convolve_taps(x, Hs, N, 1, "causal", out=out) is out
        finally:
            set_exact_convolution(False)
    assert y.shape == x.shape
    lo = 5000000
    want = x[0, 0, lo - N + 1 : lo + 1000].double().unfold(0, N, 1) @ h[0, 0].double().flip(0)    # y[n] = sum_k h[k] x[n - k]
    for got in (y, out):
        assert (got[0, 0, lo : lo + 1000].double() - want).abs().max() <= CONV_TOL * want.abs().max()
