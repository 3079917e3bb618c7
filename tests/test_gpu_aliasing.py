"""The aliasing rule of the ops surface (include/grafx_amd.h, grafx_amd/_plumbing.py: _apart): no tensor a call writes
shares an element with one it reads, with another one it writes, or with itself.  Every kernel takes its pointers
``__restrict__`` and most read more than the element they store, so such a call would be a wrong answer that depends on
timing; it is refused with a ValueError ("share memory") before anything is allocated or launched.

One table over every wrapper that writes caller memory and every (written, read) pair it names.  The refusals share one
(B, V, C, L) = (2, 6, 2, 300) buffer and x = buf[:, 0:2]; nothing here runs an aliased call: each case checks the refusal
and that the buffer and every state passed are the bits they were.  The other half is that the guard refuses nothing it
should not: the same wrappers with disjoint row ranges of one buffer -- interleaved in memory, never touching -- give the
bits of the call on fresh contiguous tensors and leave the rest of the buffer alone, at lengths that cross a tile
boundary of each kernel."""
import functools

import pytest
import torch

from conftest import assert_close

pytestmark = pytest.mark.gpu

B, V, C, L0 = 2, 6, 2, 300
R = 2 * B                 # rows of a two-node range
N = 33                    # taps of the convolutions, memory of the smoother
P = L0 + 1                # odd_alias: z (R, C, P) -> out (R, C, P - 1)


def _buffer(L):
    g = torch.Generator().manual_seed(L)
    return (torch.rand(B, V, C, L, generator=g) * 2 - 1).cuda()


def _fresh(name, *shape):
    """A seeded tensor in [0, 1) -- a signal, a gradient, an envelope, a gain or a state alike."""
    g = torch.Generator().manual_seed(sum(map(ord, name)) + len(shape))
    return torch.rand(*shape, generator=g).cuda()


def _carve(buf, shape, at, dtype=torch.float32):
    """A contiguous tensor of ``shape`` made of the buffer's memory from float ``at`` on."""
    n = 1
    for s in shape:
        n *= s
    return buf.view(-1)[at : at + n].view(dtype).view(shape)


@functools.lru_cache(maxsize=None)
def _params():
    from grafx_amd import ops

    g = torch.Generator().manual_seed(5)
    p = [(0.3 * torch.randn(R, generator=g)).cuda() for _ in range(4)]        # log_threshold, log_ratio, log_knee, z_alpha
    rad, th = 0.5 + 0.4 * torch.rand(R, C, 1, generator=g), 3.0 * torch.rand(R, C, 1, generator=g)
    h = (torch.randn(R, C, N, generator=g) / N).cuda()
    return {"p": p, "za2": torch.randn(R, 2, generator=g).cuda(),
            "As": torch.stack([torch.ones_like(rad), -2 * rad * torch.cos(th), rad * rad], -1).cuda(),
            "Bs": torch.stack([torch.ones_like(rad), -1.6 * torch.cos(th), 0.64 * torch.ones_like(rad)], -1).cuda(),
            "pre": (0.3 * torch.randn(R, 1, generator=g)).cuda(), "bias": (0.1 * torch.randn(R, 1, generator=g)).cuda(),
            "h": h, "Hs": ops.fir_spectrum(h.view(R * C, N)), "log_gain": (0.3 * torch.randn(R, 2, generator=g)).cuda()}


def _call(name, x, **t):
    """One call of wrapper ``name`` on the signal ``x`` -> every tensor it wrote or returned.  ``t``: the tensors the case
    places (written: out, tee, zf, u1_out; read: gy, g, env, u1, zi, dc, z, rowmax); a read tensor that is not given is a
    seeded one of its own."""
    from grafx_amd import ops

    q, L = _params(), x.shape[-1]
    lt, lr, lk, za = q["p"]
    out = t.get("out")

    def read(key, *shape):
        return t[key] if key in t else _fresh(name + key, *shape)

    if name == "fftconv":
        return ops.fftconv(x, q["Hs"], N, C, Lout=t.get("Lout"), out=out, tee=t.get("tee")), t.get("tee")
    if name == "fftconv_state":
        return ops.fftconv_state(x, q["Hs"], N, C, zi=read("zi", R, C, N - 1), out=out, zf=t.get("zf"))
    if name == "fir_direct":
        return (ops.fir_direct(x, q["h"], Lout=t.get("Lout"), out=out),)
    if name == "dynamics_fused":
        return ops.dynamics_fused(x, lt, lr, lk, za, 1, N, "quadratic", False, out=out, u1_out=t.get("u1_out")), t.get("u1_out")
    if name == "dynamics_bwd":
        return ops.dynamics_bwd(x, read("gy", *x.shape), lt, lr, lk, za, N, "quadratic", False, out=out, u1=t.get("u1"))
    if name == "dynamics_ballistics":
        return ops.dynamics_ballistics(x, lt, lr, lk, q["za2"], "quadratic", False, out=out, zi=read("zi", R), return_state=True)
    if name == "apply_gain":
        return (ops.apply_gain(x, read("g", R, L), out=out),)
    if name == "dyn_gain_apply":
        return (ops.dyn_gain_apply(x, read("env", R, L), lt, lr, lk, "quadratic", False, out=out),)
    if name == "stereo_gain":
        return (ops.stereo_gain(x, q["log_gain"], out=out),)
    if name == "biquad_cascade":
        return ops.biquad_cascade(x, q["Bs"], q["As"], out=out, zi=read("zi", R, C, 1, 2))
    if name == "waveshaper":
        return (ops.waveshaper(x, ops.WS_TANH, q["pre"], None, p0=q["bias"], remove_dc=True, dc=read("dc", R * C), out=out),)
    if name == "waveshaper_bwd":
        gx, grads = ops.waveshaper_bwd(x, read("gy", *x.shape), ops.WS_TANH, q["pre"], None, p0=q["bias"], remove_dc=True,
                                       dc=read("dc", R * C), out=out)
        return (gx, *grads.values())
    if name == "odd_alias":                     # (x is not its input: z is)
        return (ops.odd_alias(read("z", R, C, P), out=out, rowmax=t.get("rowmax")),)
    raise KeyError(name)


OUTPUT_WRAPPERS = ["fftconv", "fftconv_state", "fir_direct", "dynamics_fused", "dynamics_bwd", "dynamics_ballistics",
                   "apply_gain", "dyn_gain_apply", "stereo_gain", "biquad_cascade", "waveshaper", "waveshaper_bwd"]
FREE = 2 * C * L0         # first float of buf[0, 2:4], a destination apart from x


def _refusals():
    """(wrapper, what shares memory, buf -> the tensors of the call)."""
    cases = []
    for name in OUTPUT_WRAPPERS:        # out against x: the four destinations of the issue
        cases += [(name, "out is x", lambda b: {"out": b[:, 0:2]}),
                  (name, "out is the shifted range", lambda b: {"out": b[:, 1:3]}),
                  (name, "out overlaps itself", lambda b: {"out": b[:, :1].expand(B, 2, C, L0)})]
    for name in ("fftconv", "fir_direct"):    # the entries that take a shorter result: Lout
        cases.append((name, "out is x one sample on", lambda b: {"out": b[:, 0:2, :, 1:], "Lout": L0 - 1}))
    gy, grad_out = (lambda b: b[:, 2:4]), (lambda b: b[:, 4:6])
    cases += [
        ("fftconv", "tee is x", lambda b: {"tee": b[:, 0:2]}),
        ("fftconv", "tee is the shifted range", lambda b: {"tee": b[:, 1:3]}),
        ("fftconv", "tee overlaps itself", lambda b: {"tee": b[:, :1].expand(B, 2, C, L0)}),
        ("fftconv", "out and tee overlap", lambda b: {"out": b[:, 2:4], "tee": b[:, 3:5]}),
        ("fftconv_state", "out over zi", lambda b: {"out": b[:, 2:4], "zi": _carve(b, (R, C, N - 1), FREE)}),
        ("fftconv_state", "zf in x", lambda b: {"zf": _carve(b, (R, C, N - 1), 0)}),
        ("fftconv_state", "zf in out", lambda b: {"out": b[:, 2:4], "zf": _carve(b, (R, C, N - 1), FREE)}),
        ("fftconv_state", "zf is zi", lambda b: (lambda z: {"zi": z, "zf": z})(_fresh("state", R, C, N - 1))),
        ("fftconv_state", "zf is zi eight floats on",
         lambda b: (lambda s: {"zi": s[:-8].view(R, C, N - 1), "zf": s[8:].view(R, C, N - 1)})(_fresh("state", R * C * (N - 1) + 8))),
        ("dynamics_fused", "u1_out in x", lambda b: {"u1_out": _carve(b, (R, L0), 0)}),
        ("dynamics_fused", "u1_out in out", lambda b: {"out": b[:, 2:4], "u1_out": _carve(b, (R, L0), FREE)}),
        ("dynamics_bwd", "out is gy", lambda b: {"gy": gy(b), "out": b[:, 2:4]}),
        ("dynamics_bwd", "out is gy's shifted range", lambda b: {"gy": gy(b), "out": b[:, 3:5]}),
        ("dynamics_bwd", "out over u1", lambda b: {"gy": gy(b), "out": grad_out(b), "u1": _carve(b, (R, L0), 2 * FREE)}),
        ("dynamics_ballistics", "out over zi", lambda b: {"out": b[:, 2:4], "zi": _carve(b, (R,), FREE)}),
        ("apply_gain", "out over g", lambda b: {"out": b[:, 2:4], "g": _carve(b, (R, L0), FREE)}),
        ("dyn_gain_apply", "out over env", lambda b: {"out": b[:, 2:4], "env": _carve(b, (R, L0), FREE)}),
        ("biquad_cascade", "out over zi", lambda b: {"out": b[:, 2:4], "zi": _carve(b, (R, C, 1, 2), FREE)}),
        ("waveshaper", "out over dc", lambda b: {"out": b[:, 2:4], "dc": _carve(b, (R * C,), FREE)}),
        ("waveshaper_bwd", "out is gy", lambda b: {"gy": gy(b), "out": b[:, 2:4]}),
        ("waveshaper_bwd", "out is gy's shifted range", lambda b: {"gy": gy(b), "out": b[:, 3:5]}),
        ("waveshaper_bwd", "out over dc", lambda b: {"gy": gy(b), "out": grad_out(b), "dc": _carve(b, (R * C,), 2 * FREE)}),
        # odd_alias: z (R, C, 301) is the buffer's first floats, so its first 300 columns are a destination of the right shape
        ("odd_alias", "out is z", lambda b: (lambda z: {"z": z, "out": z[..., : P - 1]})(_carve(b, (R, C, P), 0))),
        ("odd_alias", "out is a range over z", lambda b: {"z": _carve(b, (R, C, P), 0), "out": b[:, 1:3]}),
        ("odd_alias", "out overlaps itself", lambda b: {"out": b[:, :1].expand(B, 2, C, L0)}),
        ("odd_alias", "out over rowmax", lambda b: {"out": b[:, 2:4], "rowmax": _carve(b, (R * C,), FREE, torch.int32)}),
    ]
    return cases


@pytest.mark.parametrize("name, what, place", _refusals(), ids=[f"{n}-{w.replace(' ', '_')}" for n, w, _ in _refusals()])
def test_a_call_that_shares_memory_is_refused_with_every_tensor_untouched(name, what, place):
    buf = _buffer(L0)
    t = place(buf)
    kept = {k: v.clone() for k, v in t.items() if isinstance(v, torch.Tensor)}
    before = buf.clone()
    with pytest.raises(ValueError, match="share memory"):
        _call(name, buf[:, 0:2], **t)
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), before.view(torch.int32)), f"{name}, {what}: the buffer changed"
    for k, v in kept.items():
        assert torch.equal(t[k].contiguous().view(torch.int32), v.contiguous().view(torch.int32)), f"{name}, {what}: {k} changed"


# Lengths that cross a boundary of the kernel that runs (and the lengths the issue named, where they differ):
#   dynamics: 1024-sample tiles (DTILE, csrc/dyn_common.hpp) and 2048 samples per workgroup of the one-shot tiles (OS_GTILE);
#     the ballistics walk cuts a row into chunks from 512 samples on (csrc/ballistics.hip: chunks of at least 256)
#   convolution: a tile of a 33-tap filter keeps 16384 - 512 = 15872 samples (conv_geom, csrc/fftconv_tile.hpp); the short FIR
#     writes 4096 samples per workgroup (FM_SEG, csrc/fir_mfma.hip)
#   cascade: 512 samples per tile (BQ_TILE = 64 lanes x BQ_E, csrc/biquad_kernel.hpp)
#   the element-wise entries have no tile of their own: they ride along at the dynamics lengths
LENGTHS = {"fftconv": (8200, 15900), "fftconv_state": (8200, 15900), "fir_direct": (4200,), "biquad_cascade": (520,),
           "odd_alias": (L0,)}
DISJOINT = [(name, L) for name in OUTPUT_WRAPPERS + ["odd_alias"] for L in LENGTHS.get(name, (1100, 2100))]


@pytest.mark.parametrize("name, L", DISJOINT)
def test_disjoint_ranges_of_one_buffer_are_not_refused_and_give_the_bits_of_fresh_tensors(name, L):
    from grafx_amd import ops

    buf = _buffer(L)
    x, out, third = buf[:, 0:2], buf[:, 2:4], buf[:, 4:6]
    here, fresh = {"out": out}, {}
    if name == "fftconv":
        here["tee"], fresh["tee"] = third, torch.empty(R, C, L, device="cuda")
    if name == "fftconv_state":
        here["zf"], fresh["zf"] = torch.empty(R, C, N - 1, device="cuda"), torch.empty(R, C, N - 1, device="cuda")
    if name == "dynamics_fused":
        here["u1_out"], fresh["u1_out"] = torch.empty(R, L, device="cuda"), torch.empty(R, L, device="cuda")
    if name in ("dynamics_bwd", "waveshaper_bwd"):       # the gradient is a third range of the same buffer
        here["gy"], fresh["gy"] = third, third.reshape(R, C, L)
    if name == "dynamics_bwd":                           # with the scan the forward kept
        u1 = torch.empty(R, L, device="cuda")
        ops.dynamics_fused(x.reshape(R, C, L), *_params()["p"], 1, N, "quadratic", False, u1_out=u1)
        here["u1"] = fresh["u1"] = u1
    want = _call(name, x.reshape(R, C, L), **fresh)      # (reshape of a strided range: a contiguous copy)
    before = buf.clone()
    got = _call(name, x, **here)
    torch.cuda.synchronize()
    assert got[0].data_ptr() == out.data_ptr()
    assert len(got) == len(want)
    for k, (a, b) in enumerate(zip(got, want)):
        assert (a is None) == (b is None), f"{name}: result {k}"
        if a is not None:
            assert a.numel() == b.numel() and torch.equal(a.reshape(b.shape).view(torch.int32), b.contiguous().view(torch.int32)), \
                f"{name} L={L}: result {k} differs from the call on fresh tensors"
    given = [1] + ([2] if name == "fftconv" else [])     # node pairs the call was given to write
    for pair in range(V // 2):
        if pair not in given:
            rows = slice(2 * pair, 2 * pair + 2)
            assert torch.equal(buf[:, rows].contiguous().view(torch.int32), before[:, rows].contiguous().view(torch.int32)), \
                f"{name} L={L}: rows {rows} of the buffer changed"


@pytest.mark.parametrize("n_fft, hop, T, dtype, limit", [
    (385, 96, 3001, torch.float32, "n_fft must be even"),
    (2050, 512, 5000, torch.float32, "from 2 to 2048"),
    (384, 0, 3001, torch.float32, "hop must be at least 1"),
    (384, 192, 192, torch.float32, "more than n_fft // 2 = 192"),
    (384, 192, 3001, torch.float64, "float32"),
])
def test_stft_names_the_limit_it_refuses_a_call_for(n_fft, hop, T, dtype, limit):
    from grafx_amd import ops

    x = _fresh("stft", 3, T)
    with pytest.raises(ValueError, match=limit):
        ops.stft(x, torch.hann_window(n_fft, device="cuda", dtype=dtype), hop)
    with pytest.raises(ValueError, match="one-dimensional float32 tensor on cuda"):
        ops.stft(x, torch.hann_window(384), 192)                        # a window on the CPU
    with pytest.raises(ValueError, match="one-dimensional"):
        ops.stft(x, torch.hann_window(384, device="cuda").view(2, 192), 192)


@pytest.mark.parametrize("n_fft", [2048, 2])
def test_stft_at_the_ends_of_its_range_matches_torch_stft(n_fft):
    """The largest and the smallest frame on the shortest row each takes (T = n_fft // 2 + 1, one sample more than the
    reflect padding needs), against torch.stft in float64 on the CPU at the 2e-6 of tests/test_gpu_small_dft.py."""
    from grafx_amd import ops

    T, hop = n_fft // 2 + 1, max(n_fft // 4, 1)
    x = _fresh("stft", 3, T) * 2 - 1
    w = torch.hann_window(n_fft)
    got = ops.stft(x, w.cuda(), hop)
    want = torch.stft(x.cpu().double(), n_fft=n_fft, hop_length=hop, window=w.double(), return_complex=True)
    assert got.shape == want.shape and got.dtype == torch.complex64
    assert_close(torch.view_as_real(got.cpu()), torch.view_as_real(want).float(), 2e-6, f"stft n_fft={n_fft} T={T}")
