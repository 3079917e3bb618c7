"""Every operator wrapper, the processors, the renders and the captured replays on a stream that is not the default one.

The rest of the GPU suite runs on torch's default stream.  Here every call is made with a side stream current:

* consumer order (`test_wrapper_reads_what_its_stream_wrote`, section 3's renders): the float inputs are filled on the side
  stream behind a device-side delay (tests/stream_order.py), so a kernel launched on any other stream reads the previous
  contents -- a second valid draw -- and the result differs from the default-stream result, which must match bit for bit;
* producer order (`test_result_is_complete_on_the_callers_stream`): the result of a multi-kernel entry, cloned on the side
  stream and handed to the default stream by one event, is complete;
* cache handoff (`test_*_handoff`): a table that is built once and kept (ops.built_once, ops._alias_plan) is complete before
  a second, independent stream can pick it up.

Safety: only float signals and parameters are filled late.  Everything a kernel indexes through or branches on -- source
indices, segment pointers, masks, mix schedule codes, row-maxima words that are inputs, plans and bases, row maps, lengths,
flags -- is valid and synchronised before any delay starts.

Wrappers that synchronise with the host on every warm call cannot pass the self-check of `ordered_call` and would be named
in HOST_SYNCHRONISING below with the line that synchronises; it may hold three entries at most."""
import math

import pytest
import torch

import stream_order
from stream_order import mismatches, ordered_call, produced_on

pytestmark = pytest.mark.gpu

# wrapper -> "file:line  the synchronising statement".  Empty: no wrapper of ops.py calls .item(), .tolist() or synchronize()
# on a warm call (ops._alias_plan and ops.built_once synchronise on a cache miss only; the misses happen in the
# default-stream call that computes `want`).
HOST_SYNCHRONISING = {}

R = 5


def test_at_most_three_wrappers_synchronise_on_a_warm_call():
    assert len(HOST_SYNCHRONISING) <= 3, sorted(HOST_SYNCHRONISING)


@pytest.fixture(scope="module", autouse=True)
def _host_times():
    yield
    stream_order.dump_host_times()


def _ops():
    from grafx_amd import ops

    return ops


def _g(seed, *key):
    import zlib

    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()) + 7919 * seed)


def _rn(g, *shape):
    return torch.randn(*shape, generator=g).cuda()


def _ru(g, *shape):
    return torch.rand(*shape, generator=g).cuda()


# ------------------------------------------------------------------------------------------------ the negative control
def test_negative_control_a_call_on_the_wrong_stream_is_reported():
    """y = x * 2 issued on the default stream while its input is filled late on the side stream: plain torch, none of the
    project's kernels.  The helper must report the mismatch -- the method can fail."""
    g = _g(0, "control")
    real, late = _rn(g, R, 2, 64), _rn(g, R, 2, 64)
    want = real * 2
    got = ordered_call(lambda: late * 2, [(late, real)], "negative control", call_stream=torch.cuda.default_stream())
    assert mismatches(got, want), "a multiplication issued on the wrong stream went unnoticed"
    # ... and the same call on the right stream passes
    late.copy_(_rn(g, R, 2, 64))
    assert not mismatches(ordered_call(lambda: late * 2, [(late, real)], "positive control"), want)


def test_a_finished_delay_fails_the_case():
    """The self-check: a call that synchronises with the host outlives any delay and must fail, not pass."""
    x = torch.zeros(4, device="cuda")

    def waits():
        torch.cuda.current_stream().synchronize()
        return x + 1

    with pytest.raises(stream_order.Unproven):
        ordered_call(waits, [], "a synchronising call", delay_ms=1.0)


# ------------------------------------------------------------------------------------------------ the table of cases
# name -> (make(seed) -> {name: float tensor}, call(tensors) -> result tree).  `make(0)` is the real draw, `make(1)` the
# prefill of the late tensors; everything else a call needs (indices, plans, schedules) is made when the case is built,
# before any delay.  A case is a function that returns the pair, so that nothing touches the GPU at collection time.
CASES = {}
PRODUCER = []     # the multi-kernel entries that also get the producer-order check


def case(name, producer=False):
    def add(build):
        CASES[name] = build
        if producer:
            PRODUCER.append(name)
        return build

    return add


def _dyn_params(g, n):
    return (torch.randn(n, generator=g).clamp(-2.5, 2.5).cuda(), (0.5 * torch.randn(n, generator=g)).cuda(),
            (0.5 * torch.randn(n, generator=g)).cuda())


# ---- FIR convolution
def _fftconv(L, N, schedule="auto", tee=False, rowmax=False, C=2, Cf=1, full=False):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "fftconv", L, N)
            return {"x": _rn(g, R, C, L), "h": _rn(g, R * Cf, N) / math.sqrt(N)}

        def call(t):
            Hs = ops.fir_spectrum(t["h"])
            tee_buf = torch.empty(R, C, L, device="cuda") if tee else None
            rm = {} if rowmax else None
            y = ops.fftconv(t["x"], Hs, N, Cf, Lout=L + N - 1 if full else None, tee=tee_buf, schedule=schedule, rowmax=rm)
            return y, tee_buf, (rm or {}).get("words")

        return make, call

    return build


case("fftconv one partition")(_fftconv(1024, 128))
case("fftconv one partition, tee")(_fftconv(1024, 128, tee=True))
case("fftconv window workspace, auto", producer=True)(_fftconv(20000, 8200))
case("fftconv window workspace, tile")(_fftconv(20000, 8200, schedule="tile"))
case("fftconv pipe")(_fftconv(16384, 4001, schedule="pipe"))
case("fftconv rowmax")(_fftconv(1024, 128, rowmax=True, full=True))


def _correlation(L, N, C):
    """fir_spectrum_reversed + fftconv with part_len_for: the long-filter gradient of autograd.convolve (a filter of L taps
    from the signal itself, N outputs)."""
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "corr", L, N)
            return {"x": _rn(g, R, C, L), "g": _rn(g, R, C, L)}

        def call(t):
            P = ops.part_len_for(L, N)
            return ops.fftconv(t["g"], ops.fir_spectrum_reversed(t["x"], part_len=P), L, C, Lout=N, off=L - 1, part_len=P)

        return make, call

    return build


case("fir_spectrum_reversed + fftconv, short")(_correlation(100, 8, 2))
case("fftconv long partitions (Nf 40000, Lout 513)", producer=True)(_correlation(40000, 513, 1))


def _fftconv_state(L, N):
    def build():
        ops = _ops()
        C, Cf = 2, 1

        def make(s):
            g = _g(s, "fftconv_state", L, N)
            return {"x": _rn(g, R, C, L), "h": _rn(g, R * Cf, N) / math.sqrt(N), "zi": _rn(g, R, C, N - 1)}

        def call(t):
            zf = torch.empty(R, C, N - 1, device="cuda")
            return ops.fftconv_state(t["x"], ops.fir_spectrum(t["h"]), N, Cf, zi=t["zi"], zf=zf)

        return make, call

    return build


case("fftconv_state one partition")(_fftconv_state(1024, 128))
case("fftconv_state window workspace")(_fftconv_state(20000, 8200))


def _fir_grad(L, N):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "fir_grad", L, N)
            return {"x": _rn(g, R, 2, L), "g": _rn(g, R, 1, L)}

        return make, lambda t: ops.fir_grad(t["x"], t["g"], N, 0)

    return build


case("fir_grad (100, 8)")(_fir_grad(100, 8))
case("fir_grad (40000, 4001)")(_fir_grad(40000, 4001))


@case("fir_direct")
def _fir_direct():
    ops = _ops()

    def make(s):
        g = _g(s, "fir_direct")
        return {"x": _rn(g, R, 2, 64), "h": _rn(g, R, 1, 5)}

    return make, lambda t: ops.fir_direct(t["x"], t["h"])


# ---- odd-length aliasing (the plans are built by the default-stream call that computes `want`)
P_ALIAS = 1151


def _odd_alias(rows, precise, view=False, rowmax=False):
    def build():
        ops = _ops()
        lo, length = 3, P_ALIAS - 1 - 7

        def make(s):
            return {"z": _rn(_g(s, "odd_alias", rows, precise), rows, P_ALIAS)}

        # the maxima words are an input of the pair form: made from the real rows, before any delay
        words = make(0)["z"].abs().amax(-1).view(torch.int32) if rowmax else None

        def call(t):
            if view:
                buf = torch.zeros(rows // 2, 3, 1, length, device="cuda")
                return ops.odd_alias(t["z"], lo, length, out=buf[:, :2]).clone()
            if rowmax:
                return ops.odd_alias(t["z"], lo, length, precise=True, rowmax=words, relu=True)
            return ops.odd_alias(t["z"], lo, length, precise=precise)

        return make, call

    return build


case("odd_alias one row")(_odd_alias(1, False))
case("odd_alias one row, precise")(_odd_alias(1, True))
case("odd_alias pairs", producer=True)(_odd_alias(4, False))
case("odd_alias pairs, precise")(_odd_alias(4, True))
case("odd_alias pairs, out= a view")(_odd_alias(4, False, view=True))
case("odd_alias pairs, precise, rowmax= and relu")(_odd_alias(4, True, rowmax=True))


def _odd_alias_adjoint(precise):
    def build():
        ops = _ops()

        def make(s):
            return {"g": _rn(_g(s, "odd_alias_adjoint", precise), 4, P_ALIAS - 1)}

        return make, lambda t: ops.odd_alias_adjoint(t["g"], P_ALIAS, precise=precise)

    return build


case("odd_alias_adjoint")(_odd_alias_adjoint(False))
case("odd_alias_adjoint, precise")(_odd_alias_adjoint(True))


# ---- small transforms
def _rdft(n):
    def build():
        ops = _ops()
        return (lambda s: {"x": _rn(_g(s, "rdft", n), R, n)}), (lambda t: ops.rdft(t["x"]))

    return build


def _irdft(n):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "irdft", n)
            return {"X": torch.complex(_rn(g, R, n // 2 + 1), _rn(g, R, n // 2 + 1))}

        return make, lambda t: ops.irdft(t["X"], n)

    return build


for _n in (384, 4001):
    case(f"rdft n={_n}")(_rdft(_n))
    case(f"irdft n={_n}")(_irdft(_n))


@case("stft (3001, 384, 192)")
def _stft():
    ops = _ops()
    window = torch.hann_window(384).cuda()
    return (lambda s: {"x": _ru(_g(s, "stft"), R, 3001) * 2 - 1}), (lambda t: ops.stft(t["x"], window, 192))


# ---- reverb
def _reverb_module(ir_len):
    from grafx_amd.processors import STFTMaskedNoiseReverb

    return STFTMaskedNoiseReverb(ir_len=ir_len, gain_envelope=True, flashfftconv=False).cuda()


def _stft_reverb_ir(ir_len, schedule, per_row_noise):
    def build():
        ops = _ops()
        m = _reverb_module(ir_len)
        basis = m._istft_basis(torch.device("cuda", torch.cuda.current_device()))
        K, T = m.num_bins, m.num_frames

        def make(s):
            g = _g(s, "stft_reverb_ir", ir_len, per_row_noise)
            t = {"p0": _rn(g, R, 2, K), "p1": _rn(g, R, 2, K) - 3.0, "genv": 0.5 * _rn(g, R, 2, T)}
            if per_row_noise:
                t["noise"] = torch.complex(_rn(g, R, 2, K, T), _rn(g, R, 2, K, T))
            return t

        def call(t):
            return ops.stft_reverb_ir(t.get("noise", m.noise_stft), t["p0"], t["p1"], t["genv"], m.window, basis, ir_len,
                                      m.hop_length, True, schedule=schedule)

        return make, call

    return build


for _ir in (400, 5953):
    for _sched in ("gemm", "fft"):
        case(f"stft_reverb_ir ir_len={_ir} {_sched}, shared noise", producer=(_ir, _sched) == (5953, "fft"))(
            _stft_reverb_ir(_ir, _sched, False))
        case(f"stft_reverb_ir ir_len={_ir} {_sched}, noise per row", producer=(_ir, _sched) == (400, "gemm"))(
            _stft_reverb_ir(_ir, _sched, True))


@case("istft_basis")
def _istft_basis():
    """The bases are an opaque buffer: compared through the impulse responses synthesised from them (fixed parameters)."""
    ops = _ops()
    m = _reverb_module(400)
    g = _g(0, "istft_basis parameters")
    p0, p1 = _rn(g, R, 2, m.num_bins), _rn(g, R, 2, m.num_bins) - 3.0

    def make(s):
        return {"window": torch.hann_window(384).cuda() * (0.75 + 0.5 * _ru(_g(s, "istft_basis"), 384))}

    def call(t):
        basis = ops.istft_basis(t["window"])
        return ops.stft_reverb_ir(m.noise_stft, p0, p1, None, t["window"], basis, 400, m.hop_length, True)

    return make, call


def _noise_shaping_ir(fade):
    def build():
        ops = _ops()
        C, K, ir_len, T = 2, 4, 48, 64

        def make(s):
            g = _g(s, "noise_shaping_ir", fade)
            return {"noise": _ru(g, C, K, T) * 2 - 1, "ld": _rn(g, R, C, K), "lgain": _rn(g, R, C, K), "lf": _rn(g, R, C, K),
                    "zf": _rn(g, R, C, K)}

        def call(t):
            return ops.noise_shaping_ir(t["noise"], t["ld"], t["lgain"], t["lf"] if fade else None, t["zf"] if fade else None,
                                        ir_len, -0.2, -0.005)

        return make, call

    return build


case("noise_shaping_ir")(_noise_shaping_ir(False))
case("noise_shaping_ir, fade in")(_noise_shaping_ir(True))


# ---- filter design
def _biquads(g, K, dtype=torch.float32):
    Bs = torch.randn(R, 1, K, 3, generator=g) * 0.2 + torch.tensor([1.0, 0, 0])
    As = torch.tensor([1.0, -1.2, 0.5]).expand(R, 1, K, 3) + 0.05 * torch.randn(R, 1, K, 3, generator=g)
    return Bs.to(dtype).cuda(), As.to(dtype).cuda()


def _iir_fsm_fir(N, dtype):
    def build():
        ops = _ops()
        plan = ops.iir_fsm_plan(N, torch.device("cuda"))     # (None at 8192: the tile's own inverse transform)
        torch.cuda.synchronize()

        def make(s):
            Bs, As = _biquads(_g(s, "iir_fsm_fir", N), 2, dtype)
            return {"Bs": Bs, "As": As}

        return make, lambda t: ops.iir_fsm_fir(t["Bs"], t["As"], N, plan)

    return build


for _N in (65, 8192):
    case(f"iir_fsm_fir N={_N}")(_iir_fsm_fir(_N, torch.float32))
    case(f"iir_fsm_fir N={_N}, float64 coefficients")(_iir_fsm_fir(_N, torch.float64))


@case("iir_fsm_bwd")
def _iir_fsm_bwd():
    from grafx_amd import autograd as diff

    ops = _ops()
    N = 65
    delays = diff._fsm_delays(N, torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.synchronize()

    def make(s):
        g = _g(s, "iir_fsm_bwd")
        Bs, As = _biquads(g, 2)
        return {"Bs": Bs, "As": As, "G": torch.complex(_rn(g, R, 1, N // 2 + 1), _rn(g, R, 1, N // 2 + 1))}

    return make, lambda t: ops.iir_fsm_bwd(t["Bs"], t["As"], t["G"], delays, N)


def _peq(shelving, bwd):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "peq", shelving, bwd)
            t = {k: 0.5 * _rn(g, R, 1, 3) for k in ("w0", "qi", "lg")}
            if bwd:
                t.update(gB=_rn(g, R, 1, 3, 3), gA=_rn(g, R, 1, 3, 3))
            return t

        if bwd:
            return make, lambda t: ops.peq_coeffs_bwd(t["w0"], t["qi"], t["lg"], t["gB"], t["gA"], use_shelving=shelving)
        return make, lambda t: ops.peq_coeffs(t["w0"], t["qi"], t["lg"], use_shelving=shelving)

    return build


for _sh in (True, False):
    case(f"peq_coeffs shelving={_sh}")(_peq(_sh, False))
    case(f"peq_coeffs_bwd shelving={_sh}")(_peq(_sh, True))


def _biquad_coeffs(normalized):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "biquad_coeffs", normalized)
            t = {"Bin": _rn(g, R, 2, 3), "a1": _rn(g, R, 2), "a2": _rn(g, R, 2)}
            if normalized:
                t["A0"] = _ru(g, R, 2) + 0.5
            return t

        return make, lambda t: ops.biquad_coeffs(t["Bin"], t["a1"], t["a2"], t.get("A0"))

    return build


case("biquad_coeffs")(_biquad_coeffs(False))
case("biquad_coeffs, A0")(_biquad_coeffs(True))


def _biquad_cascade(stateful):
    def build():
        ops = _ops()
        K, C, L = 3, 2, 5000

        def make(s):
            g = _g(s, "biquad_cascade", stateful)
            rad, th = 0.5 + 0.4 * torch.rand(R, C, K, generator=g), 3.0 * torch.rand(R, C, K, generator=g)
            As = torch.stack([torch.ones_like(rad), -2 * rad * torch.cos(th), rad * rad], -1)
            Bs = torch.stack([torch.ones_like(rad), -1.6 * torch.cos(th), 0.64 * torch.ones_like(rad)], -1)
            t = {"x": _rn(g, R, C, L), "Bs": Bs.cuda(), "As": As.cuda()}
            if stateful:
                t["zi"] = 0.1 * _rn(g, R, C, K, 2)
            return t

        if stateful:
            return make, lambda t: ops.biquad_cascade(t["x"], t["Bs"], t["As"], zi=t["zi"], return_state=True)
        return make, lambda t: ops.biquad_cascade(t["x"], t["Bs"], t["As"])

    return build


case("biquad_cascade K=3 L=5000")(_biquad_cascade(False))
case("biquad_cascade K=3 L=5000, zi and return_state")(_biquad_cascade(True))


# ---- dynamics
def _dynamics_fused(smoother, schedule, L, N):
    def build():
        ops = _ops()
        C = 2

        def make(s):
            g = _g(s, "dynamics_fused", smoother, L)
            lt, lr, lk = _dyn_params(g, R)
            return {"x": _rn(g, R, C, L), "lt": lt, "lr": lr, "lk": lk, "z": _rn(g, R)}

        def call(t):
            u1 = torch.empty(R, L, device="cuda") if smoother == 1 else None
            y = ops.dynamics_fused(t["x"], t["lt"], t["lr"], t["lk"], t["z"], smoother, N, "quadratic", False, schedule=schedule,
                                   u1_out=u1)
            return y, u1

        return make, call

    return build


for _sm in (0, 1):
    for _sched in ("oneshot", "rows"):
        for _L, _N in ((64, 33), (20000, 1023)):
            case(f"dynamics_fused smoother={_sm} {_sched} L={_L} iir_len={_N}",
                 producer=(_sm, _sched, _L) == (1, "oneshot", 20000))(_dynamics_fused(_sm, _sched, _L, _N))


def _mix_static(n):
    """One destination summing the n rows of every graph: schedule codes and gather indices, on the device before any delay."""
    ops = _ops()
    codes, n_acc, pre, post = ops.mix_schedule([list(range(n))], n)
    assert not pre and not post
    sched = torch.tensor(codes, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    return sched, n_acc


@case("dynamics_fused with a fused mix")
def _dynamics_mix():
    ops = _ops()
    B, n, C, L = 2, 3, 2, 64
    sched, n_acc = _mix_static(n)

    def make(s):
        g = _g(s, "dynamics_mix")
        lt, lr, lk = _dyn_params(g, B * n)
        return {"x": _rn(g, B, n, C, L), "lt": lt, "lr": lr, "lk": lk, "z": _rn(g, B * n)}

    def call(t):
        mix = {"sched": sched, "n_acc": n_acc, "out": torch.zeros(B, 1, C, L, device="cuda")}
        y = ops.dynamics_fused(t["x"], t["lt"], t["lr"], t["lk"], t["z"], 1, 33, "quadratic", False,
                               out=torch.empty(B, n, C, L, device="cuda"), mix=mix)
        return y, (mix["out"] if mix.get("done") else None)

    return make, call


def _dynamics_bwd(path):
    def build():
        ops = _ops()
        C, L, N, knee = 2, 64, 33, "exponential"

        def make(s):
            g = _g(s, "dynamics_bwd", path)
            lt, lr, lk = _dyn_params(g, R)
            return {"x": _rn(g, R, C, L), "gy": _rn(g, R, C, L), "lt": lt, "lr": lr, "lk": lk, "z": _rn(g, R)}

        def call(t):
            a = (t["x"], t["gy"], t["lt"], t["lr"], t["lk"], t["z"])
            if path == "kept scan":
                u1 = torch.empty(R, L, device="cuda")
                ops.dynamics_fused(a[0], *a[2:], 1, N, knee, False, u1_out=u1, schedule="rows")
                return ops.dynamics_bwd(*a, N, knee, False, u1=u1, schedule="rows")
            return ops.dynamics_bwd(*a, N, knee, False, rescan=path == "rescan")

        return make, call

    return build


for _path in ("kept scan", "rescan", "plain"):
    case(f"dynamics_bwd {_path}")(_dynamics_bwd(_path))


@case("dyn_gain_bwd")
def _dyn_gain_bwd():
    ops = _ops()

    def make(s):
        g = _g(s, "dyn_gain_bwd")
        lt, lr, lk = _dyn_params(g, R)
        return {"x": _rn(g, R, 2, 64), "gy": _rn(g, R, 2, 64), "env": _rn(g, R, 64).square(), "lt": lt, "lr": lr, "lk": lk}

    return make, lambda t: ops.dyn_gain_bwd(t["x"], t["gy"], t["env"], t["lt"], t["lr"], t["lk"], "quadratic", False)


@case("dyn_dx")
def _dyn_dx():
    ops = _ops()

    def make(s):
        g = _g(s, "dyn_dx")
        return {"x": _rn(g, R, 2, 64), "gy": _rn(g, R, 2, 64), "gain": _ru(g, R, 64), "de": _rn(g, R, 64)}

    return make, lambda t: ops.dyn_dx(t["x"], t["gy"], t["gain"], t["de"])


@case("onepole_dz")
def _onepole_dz():
    ops = _ops()

    def make(s):
        g = _g(s, "onepole_dz")
        return {"g": _ru(g, R, 64), "U": _ru(g, R, 64), "D": _ru(g, R, 64), "coef": _ru(g, R, 4) + 0.1}

    return make, lambda t: ops.onepole_dz(t["g"], t["U"], t["D"], t["coef"], 17)


# ---- one-pole entries
@case("energy")
def _energy():
    ops = _ops()
    return (lambda s: {"x": _rn(_g(s, "energy"), R, 2, 64)}), (lambda t: ops.energy(t["x"]))


@case("onepole")
def _onepole():
    ops = _ops()

    def make(s):
        g = _g(s, "onepole")
        return {"u": _rn(g, R, 64).square(), "z": _rn(g, R)}

    return make, lambda t: ops.onepole(t["u"], t["z"], 33)


@case("onepole_energy with rowmax")
def _onepole_energy():
    ops = _ops()

    def make(s):
        g = _g(s, "onepole_energy")
        return {"x": _rn(g, R, 2, 64), "z": _rn(g, R)}

    def call(t):
        rm = {}
        return ops.onepole_energy(t["x"], t["z"], 33, rowmax=rm), rm["words"]

    return make, call


@case("onepole_fir")
def _onepole_fir():
    ops = _ops()
    return (lambda s: {"z": _rn(_g(s, "onepole_fir"), R)}), (lambda t: ops.onepole_fir(t["z"], 300))


# ---- ballistics (L = 1031: more than one chunk of the chunked schedule)
L_BAL = 1031


def _ballistics(which, schedule):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "ballistics", which, schedule)
            lt, lr, lk = _dyn_params(g, R)
            return {"x": _rn(g, R, 2, L_BAL), "u": _ru(g, R, L_BAL) * 2, "coef": _ru(g, R, 2) * 0.96 + 0.02, "z": _rn(g, R, 2),
                    "zi": _ru(g, R) + 0.1, "gr": _ru(g, R, L_BAL), "lt": lt, "lr": lr, "lk": lk}

        def call(t):
            if which == "ballistics":
                return ops.ballistics(t["u"], t["coef"], coefficients=True, schedule=schedule, zi=t["zi"], return_state=True)
            if which == "ballistics_energy":
                return ops.ballistics_energy(t["x"], t["coef"], coefficients=True, schedule=schedule, zi=t["zi"], return_state=True)
            if which == "dynamics_ballistics":
                return ops.dynamics_ballistics(t["x"], t["lt"], t["lr"], t["lk"], t["z"], "exponential", False, schedule=schedule,
                                               zi=t["zi"], return_state=True)
            y = ops.ballistics(t["u"], t["z"], schedule="rows", zi=t["zi"])
            return ops.ballistics_bwd(t["u"], y, t["gr"], t["z"], schedule=schedule, zi=t["zi"])

        return make, call

    return build


for _which in ("ballistics", "ballistics_energy", "dynamics_ballistics", "ballistics_bwd"):
    for _sched in ("chunks", "rows"):
        case(f"{_which} {_sched}, zi and return_state")(_ballistics(_which, _sched))


# ---- gain
def _dyn_gain(gate, log_out):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "dyn_gain", gate, log_out)
            lt, lr, lk = _dyn_params(g, R)
            return {"env": _rn(g, R, 64).square(), "lt": lt, "lr": lr, "lk": lk}

        return make, lambda t: ops.dyn_gain(t["env"], t["lt"], t["lr"], t["lk"], "quadratic", gate, log_out)

    return build


case("dyn_gain")(_dyn_gain(False, False))
case("dyn_gain gate, log_out")(_dyn_gain(True, True))


def _apply_gain(exp_gain):
    def build():
        ops = _ops()

        def make(s):
            g = _g(s, "apply_gain", exp_gain)
            return {"x": _rn(g, R, 2, 64), "gain": 0.5 * _rn(g, R, 64)}

        return make, lambda t: ops.apply_gain(t["x"], t["gain"], exp_gain=exp_gain)

    return build


case("apply_gain")(_apply_gain(False))
case("apply_gain exp_gain")(_apply_gain(True))


@case("dyn_gain_apply")
def _dyn_gain_apply():
    ops = _ops()

    def make(s):
        g = _g(s, "dyn_gain_apply")
        lt, lr, lk = _dyn_params(g, R)
        return {"x": _rn(g, R, 2, 64), "env": _rn(g, R, 64).square(), "lt": lt, "lr": lr, "lk": lk}

    return make, lambda t: ops.dyn_gain_apply(t["x"], t["env"], t["lt"], t["lr"], t["lk"], "quadratic", False)


@case("stereo_gain")
def _stereo_gain():
    ops = _ops()

    def make(s):
        g = _g(s, "stereo_gain")
        return {"x": _rn(g, R, 2, 64), "lg": 0.5 * _rn(g, R, 2)}

    return make, lambda t: ops.stereo_gain(t["x"], t["lg"])


@case("stereo_gain with a fused mix")
def _stereo_gain_mix():
    ops = _ops()
    B, n, C, L = 2, 3, 2, 64
    sched, n_acc = _mix_static(n)

    def make(s):
        g = _g(s, "stereo_gain_mix")
        return {"x": _rn(g, B, n, C, L), "lg": 0.5 * _rn(g, B * n, 2)}

    def call(t):
        mix = {"sched": sched, "n_acc": n_acc, "out": torch.zeros(B, 1, C, L, device="cuda")}
        y = ops.stereo_gain(t["x"], t["lg"], out=torch.empty(B, n, C, L, device="cuda"), mix=mix)
        return y, (mix["out"] if mix.get("done") else None)

    return make, call


# ---- waveshapers
@case("row_mean")
def _row_mean():
    ops = _ops()
    return (lambda s: {"x": _rn(_g(s, "row_mean"), R, 2, 64) + 3}), (lambda t: ops.row_mean(t["x"]))


def _waveshaper(name, kw, rows, C, L, bwd):
    def build():
        from test_gpu_waveshaper_bwd import MODES, _module, _ops_arguments

        ops = _ops()
        m = _module(name, tuple(sorted(dict(kw).items())))

        def make(s):
            g = _g(s, "waveshaper", name, sorted(dict(kw).items()), bwd)
            t = {k: 0.5 * _rn(g, rows, n) for k, n in m.parameter_size().items()}
            if MODES[name] >= 2 and "log_pre_gain" in t:
                t["log_pre_gain"] = -t["log_pre_gain"].abs()
            t["x"] = _ru(g, rows, C, L) * 1.8 - 0.9
            if bwd:
                t["gy"] = _rn(g, rows, C, L)
            return t

        def call(t):
            args, _ = _ops_arguments(m, name, {k: v for k, v in t.items() if k not in ("x", "gy")})
            if bwd:
                return ops.waveshaper_bwd(t["x"], t["gy"], **args)
            return ops.waveshaper(t["x"], **args)

        return make, call

    return build


def _waveshaper_cases():
    from test_gpu_next_rows2 import NL

    for tag in sorted(NL):
        case(f"waveshaper {tag}")(_waveshaper(*NL[tag], R, 2, 64, False))
    # the backward: remove_dc (the means' kernel, then the pass) and a polynomial of order 10 (per-workgroup partial sums)
    case("waveshaper_bwd tanh_b (remove_dc)", producer=True)(_waveshaper(*NL["tanh_b"], 3, 2, 4099, True))
    case("waveshaper_bwd cheb_a (K = 10)")(_waveshaper(*NL["cheb_a"], 3, 2, 4099, True))


_waveshaper_cases()


# ---- routing
@case("gather_sum and gather_sum_fanout")
def _gather_sum():
    ops = _ops()
    B, V, C, L, J = 2, 4, 2, 64, 3
    dests = [[0, 1], [2], [0, 2, 3]]
    src = torch.tensor([s for d in dests for s in d]).cuda()
    seg = torch.tensor([0] + [sum(len(d) for d in dests[: j + 1]) for j in range(J)]).cuda()
    uniq = sorted({s for d in dests for s in d})
    usrc = torch.tensor(uniq).cuda()
    mask = torch.tensor([sum(1 << j for j, d in enumerate(dests) if s in d) for s in uniq]).cuda()
    torch.cuda.synchronize()     # the indices are on the device before any delay

    def call(t):
        out, fan = torch.zeros(B, J, C, L, device="cuda"), torch.zeros(B, J, C, L, device="cuda")
        ops.gather_sum(t["buf"], src, seg, out)
        assert ops.gather_sum_fanout(t["buf"], usrc, mask, fan), "gather_sum_fanout refused the call"
        return out, fan

    return (lambda s: {"buf": _rn(_g(s, "gather_sum"), B, V, C, L)}), call


# ------------------------------------------------------------------------------------------------ section 2: the tests
def _want(name):
    make, call = CASES[name]()
    real = make(0)
    want = call(real)
    torch.cuda.synchronize()
    return make, call, real, want


@pytest.mark.parametrize("name", list(CASES))
def test_wrapper_reads_what_its_stream_wrote(name):
    assert name.split()[0] not in HOST_SYNCHRONISING
    make, call, real, want = _want(name)
    late = make(1)
    assert all(not torch.equal(late[k], real[k]) for k in real), "the prefill is the real draw"
    got = ordered_call(lambda: call(late), [(late[k], real[k]) for k in real], name)
    bad = mismatches(got, want)
    assert not bad, f"{name} on a side stream differs from the default-stream result: {bad}"


@pytest.mark.parametrize("name", PRODUCER)
def test_result_is_complete_on_the_callers_stream(name):
    make, call, real, want = _want(name)
    bad = mismatches(produced_on(lambda: call(real)), want)
    assert not bad, f"{name}: the result handed over by an event differs from the default-stream result: {bad}"


# ------------------------------------------------------------------------------------------------ section 3: processors, renders
B3, L3 = 2, 4096


def _chain():
    """in -> equaliser (fsm, 257 taps) -> compressor (iir, 255) -> reverb (1501 taps) -> out, on the GPU."""
    from grafx_amd.data import GRAFX, NodeConfigs, convert_to_tensor
    from grafx_amd.processors import Compressor, ParametricEqualizer, STFTMaskedNoiseReverb
    from grafx_amd.render import prepare_render, reorder_for_fast_render

    procs = {"eq": ParametricEqualizer(num_filters=3, flashfftconv=False, fsm_fir_len=257).cuda(),
             "compressor": Compressor(energy_smoother="iir", iir_len=255, flashfftconv=False).cuda(),
             "reverb": STFTMaskedNoiseReverb(ir_len=1501, flashfftconv=False).cuda()}
    G = GRAFX(config=NodeConfigs(["eq", "compressor", "reverb"]))
    G.add_serial_chain(["in", "eq", "compressor", "reverb", "mix", "out"])
    rd = prepare_render(reorder_for_fast_render(convert_to_tensor(G), method="beam")).to("cuda")
    return procs, G, rd


def _draw(procs, G, seed, length=L3):
    """(x, parameters) on the GPU: a valid draw of the signal and of every parameter (std 0.3)."""
    from grafx_amd.utils import create_empty_parameters

    torch.manual_seed(seed)
    params = {t: {k: v.detach().cuda() for k, v in d.items()} for t, d in create_empty_parameters(procs, G, std=0.3).items()}
    x = (0.3 * torch.randn(B3, 1, 2, length, generator=torch.Generator().manual_seed(seed))).cuda()
    return x, params


def _pairs(late, real):
    (lx, lp), (rx, rp) = late, real
    return [(lx, rx)] + [(lp[t][k], rp[t][k]) for t in rp for k in rp[t]]


def test_render_joins_the_callers_stream():
    """render_grafx, inference path: its copy and prepare streams wait for the caller's stream, not the default one."""
    from grafx_amd.render import render_grafx

    procs, G, rd = _chain()
    real, late = _draw(procs, G, 1), _draw(procs, G, 2)

    def render(d):
        with torch.no_grad():
            y, _, buf = render_grafx(procs, d[0], d[1], rd)
        return y, buf

    want = render(real)
    torch.cuda.synchronize()
    got = ordered_call(lambda: render(late), _pairs(late, real), "render_grafx", stream_order.RENDER_DELAY_MS)
    assert not mismatches(got, want)
    assert not mismatches(produced_on(lambda: render(real)), want)


def test_training_step_on_a_side_stream():
    """Forward and backward() under the side stream: the output and the gradients of every parameter and of the input."""
    from grafx_amd.render import render_grafx

    procs, G, rd = _chain()
    real, late = _draw(procs, G, 3), _draw(procs, G, 4)

    def step(d):
        x = d[0].detach().requires_grad_()
        params = {t: {k: v.detach().requires_grad_() for k, v in p.items()} for t, p in d[1].items()}
        y, _, _ = render_grafx(procs, x, params, rd)
        y.square().mean().backward()
        assert x.grad is not None and all(v.grad is not None for p in params.values() for v in p.values())
        return y.detach(), x.grad, {t: {k: v.grad for k, v in p.items()} for t, p in params.items()}

    step(real)                      # (the first step builds the tables of the training path: ops.built_once)
    want = step(real)
    torch.cuda.synchronize()
    got = ordered_call(lambda: step(late), _pairs(late, real), "training step", stream_order.RENDER_DELAY_MS)
    assert not mismatches(got, want)


def test_streamed_blocks_on_a_side_stream():
    """Two consecutive blocks with state= / return_state=True (ballistics compressor: the streamable smoother)."""
    from grafx_amd.processors import Compressor
    from grafx_amd.processors.core._buffer_io import carry_leaves
    from grafx_amd.render import render_grafx

    procs, G, rd = _chain()
    procs["compressor"] = Compressor(energy_smoother="ballistics", iir_len=255, flashfftconv=False).cuda()
    real, late = _draw(procs, G, 5), _draw(procs, G, 6)
    n = L3 // 2

    def blocks(d):
        out, state = [], None
        with torch.no_grad():
            for k in range(2):
                y, _, buf, state = render_grafx(procs, d[0][..., k * n : (k + 1) * n], d[1], rd, state=state, return_state=True)
                out.append((y, buf, [carry_leaves(state.carries[i]) for i in sorted(state.carries)]))
        return out

    want = blocks(real)
    torch.cuda.synchronize()
    got = ordered_call(lambda: blocks(late), _pairs(late, real), "streamed blocks", stream_order.RENDER_DELAY_MS)
    assert not mismatches(got, want)


def test_captured_render_replays_on_a_side_stream():
    from grafx_amd.render import CapturedRender, render_grafx

    procs, G, rd = _chain()
    real, late = _draw(procs, G, 7), _draw(procs, G, 8)
    with torch.no_grad():
        want = render_grafx(procs, real[0], real[1], rd)
    want = (want[0], want[2])
    fast = CapturedRender(procs, late[0], late[1], rd)
    torch.cuda.synchronize()

    def replay():
        y, _, buf = fast(late[0], late[1])      # the static inputs are copied in on the current stream, then the replay
        return y, buf

    got = ordered_call(replay, _pairs(late, real), "CapturedRender", stream_order.RENDER_DELAY_MS)
    assert not mismatches(got, want)


def test_captured_stream_replays_on_a_side_stream():
    from grafx_amd.processors import Compressor
    from grafx_amd.render import CapturedStream, render_grafx, silent_state

    procs, G, rd = _chain()
    procs["compressor"] = Compressor(energy_smoother="ballistics", iir_len=255, flashfftconv=False).cuda()
    n = 512
    real, late = _draw(procs, G, 9, 2 * n), _draw(procs, G, 10, 2 * n)
    want, state = [], None
    with torch.no_grad():
        state = silent_state(procs, real[0][..., :n], real[1], rd)
        for k in range(2):
            y, _, buf, state = render_grafx(procs, real[0][..., k * n : (k + 1) * n], real[1], rd, state=state, return_state=True)
            want.append((y, buf))
    stream = CapturedStream(procs, late[0][..., :n], late[1], rd)
    torch.cuda.synchronize()

    def replay():
        stream.update_parameters(late[1])
        out = []
        for k in range(2):
            y, _, buf = stream(late[0][..., k * n : (k + 1) * n])
            out.append((y.clone(), buf.clone()))
        return out

    got = ordered_call(replay, _pairs(late, real), "CapturedStream", stream_order.RENDER_DELAY_MS)
    assert not mismatches(got, want)


# ------------------------------------------------------------------------------------------------ section 4: cache handoff
def _scrub_free_blocks(stream):
    """Fill the memory the caching allocator holds free for ``stream`` with 0xFF bytes (NaN as floats).  A table that has not
    been built yet is a fresh allocation on that stream: without this it may be a recycled block that still holds the
    finished table of an earlier owner (seen on the MI355X: the equaliser's 257-tap plan right after the filter's), and
    the unfinished table would pass.  Blocks are recycled per stream, so the stream's own free blocks are what matters;
    memory that comes fresh from the driver read as zeros."""
    torch.cuda.synchronize()
    held = []
    with torch.cuda.stream(stream):
        for size in (16 << 20, 1 << 20, 64 << 10, 4 << 10, 512):
            for _ in range(2048):
                before = torch.cuda.memory_reserved()
                held.append(torch.empty(size, dtype=torch.uint8, device="cuda").fill_(255))
                if torch.cuda.memory_reserved() > before:     # from the driver: no free block of this size is left
                    break
    torch.cuda.synchronize()
    del held


def _handoff(use):
    """``use()`` on stream A behind a delay (the build of a missing table is queued behind it) and at once on an
    independent stream B -> (A's result, B's result), both streams synchronised.  The host may block inside the build."""
    A, B = stream_order.side_streams(2)     # shown to run beside each other: B does not queue up behind A's delay
    _scrub_free_blocks(A)
    stream_order.delayed(A)
    with torch.cuda.stream(A):
        a = use()
    with torch.cuda.stream(B):
        b = use()
    A.synchronize()
    B.synchronize()
    torch.cuda.synchronize()
    return a, b


def _assert_handoff(a, b, want, label):
    assert not mismatches(b, want), f"{label}: the second stream picked up an unfinished table: {mismatches(b, want)}"
    assert not mismatches(a, want), f"{label}: the building stream's own result differs: {mismatches(a, want)}"


def test_iir_filter_plan_handoff():
    from grafx_amd.processors.core.iir import IIRFilter

    Bs, As = _biquads(_g(0, "handoff iir"), 2)
    want = IIRFilter(fsm_fir_len=257, flashfftconv=False).cuda().fsm_fir(Bs, As)
    torch.cuda.synchronize()
    fresh = IIRFilter(fsm_fir_len=257, flashfftconv=False).cuda()
    _assert_handoff(*_handoff(lambda: fresh.fsm_fir(Bs, As)), want, "IIRFilter._plan")


def test_parametric_equalizer_plan_handoff():
    from grafx_amd.processors import ParametricEqualizer

    def new():
        return ParametricEqualizer(num_filters=3, flashfftconv=False, fsm_fir_len=257).cuda()

    g = _g(0, "handoff peq")
    x = 0.3 * _rn(g, R, 2, 4096)
    params = {k: 0.3 * _rn(g, R, *((n,) if isinstance(n, int) else n)) for k, n in new().parameter_size().items()}
    with torch.no_grad():
        want = new()(x, **params)
    torch.cuda.synchronize()
    fresh = new()

    def use():
        with torch.no_grad():
            return fresh(x, **params)

    _assert_handoff(*_handoff(use), want, "ParametricEqualizer's IIRFilter._plan")


def _reverb_params(m, g):
    return {k: 0.3 * _rn(g, R, *n) for k, n in m.parameter_size().items()}


def test_reverb_basis_handoff():
    from grafx_amd.processors import STFTMaskedNoiseReverb

    def new():
        return STFTMaskedNoiseReverb(ir_len=400, flashfftconv=False).cuda()

    params = _reverb_params(new(), _g(0, "handoff basis"))
    with torch.no_grad():
        want = new().compute_ir(**params)
    torch.cuda.synchronize()
    fresh = new()

    def use():
        with torch.no_grad():
            return fresh.compute_ir(**params)

    _assert_handoff(*_handoff(use), want, "STFTMaskedNoiseReverb._basis")


def test_reverb_envelope_handoff():
    from grafx_amd.processors import STFTMaskedNoiseReverb

    def new():
        return STFTMaskedNoiseReverb(ir_len=400, flashfftconv=False).cuda()

    params = _reverb_params(new(), _g(0, "handoff envelope"))
    weight = _rn(_g(0, "handoff envelope weight"), R, 2, 400)

    def use_of(m):
        def use():
            p = {k: v.detach().clone().requires_grad_() for k, v in params.items()}
            ir = m.compute_ir(**p)
            (ir * weight).sum().backward()
            return ir.detach(), {k: v.grad for k, v in p.items()}

        return use

    want = use_of(new())()
    torch.cuda.synchronize()
    _assert_handoff(*_handoff(use_of(new())), want, "STFTMaskedNoiseReverb._envelope")


def test_fsm_delays_handoff():
    from grafx_amd import autograd as diff

    ops = _ops()
    N = 263                       # a tap length of this test alone
    dev = torch.device("cuda", torch.cuda.current_device())
    Bs, As = _biquads(_g(0, "handoff delays"), 2)
    gh = _rn(_g(0, "handoff delays gh"), R, 1, N)
    plan = ops.iir_fsm_plan(N, dev)
    torch.cuda.synchronize()

    def use():
        b, a = Bs.clone().requires_grad_(), As.clone().requires_grad_()
        diff.FsmFirFn.apply(b, a, N, plan).backward(gh)
        return b.grad, a.grad

    want = use()
    torch.cuda.synchronize()
    assert diff._DELAYS.pop((N, dev.type, dev.index), None) is not None
    _assert_handoff(*_handoff(use), want, "autograd._fsm_delays")


def test_alias_plan_handoff():
    """ops._alias_plan already synchronises after its build: this guards it."""
    ops = _ops()
    P = 1153                      # a length of this test alone
    z = _rn(_g(0, "handoff alias"), 4, P)
    dev = z.device
    want = ops.odd_alias(z)
    torch.cuda.synchronize()
    key = (P, dev.type, dev.index, False, True)
    assert ops._ALIAS_PLANS.pop(key, None) is not None
    torch.cuda.synchronize()
    _assert_handoff(*_handoff(lambda: ops.odd_alias(z)), want, "ops._alias_plan")
