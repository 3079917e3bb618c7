"""SHA-256 of every tensor the five fused effects return, fixed seeds: how a change that must keep their bits is checked.

    GRAFX_AMD_LIB=<library A> python tools/effect_digests.py a.json
    GRAFX_AMD_LIB=<library B> python tools/effect_digests.py b.json
    python tools/effect_digests.py --compare a.json b.json              (exit status 1 when a digest differs)

R = 3, C = 2.  Limiter, modulated delay (linear, cubic) and feedback delay (C = 1, 2) at two tiles + 17 samples: forward,
backward with ``want`` = all and each gradient alone, two blocks with state.  Waveshaper and oversampled waveshaper (factor
2) at L = 1000: the four modes with and without ``remove_dc``, forward, backward with ``want`` = all, ("x",) and each given
parameter alone, and the backward under ``inverse_post_gain``.  A measurement tool, not a test; needs the GPU.
"""

import hashlib
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from grafx_amd import ops  # noqa: E402
import grafx_amd.processors as P  # noqa: E402

R, C = 3, 2
OUT = {}


def put(key, t):
    if t is None:
        OUT[key] = None
    elif isinstance(t, dict):
        for k, v in t.items():
            put(f"{key}/{k}", v)
    elif isinstance(t, (tuple, list)):
        for i, v in enumerate(t):
            put(f"{key}/{i}", v)
    else:
        assert key not in OUT, key
        OUT[key] = hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def gen(seed):
    return torch.Generator().manual_seed(seed)


def limiter():
    D, H, N = 7, 0, 3
    L = 2 * ops.limiter_tile(D + 1 + H) + 17
    x = (torch.randn(R, C, L, generator=gen(1)) * 0.3).cuda()
    g = torch.randn(R, C, L, generator=gen(2)).cuda()
    lc = torch.log(torch.tensor([0.25, 0.12, 0.2])).cuda()
    h = torch.tensor([0.25, 0.5, 0.25]).cuda()
    for comp in (False, True):
        tag = f"limiter/comp={comp}"
        put(f"{tag}/fwd", ops.limiter(x, lc, h, D, H, compensate=comp, return_gain=True))
        for want in (ops.LIMITER_GRADS, ("x",), ("log_ceiling",)):
            put(f"{tag}/bwd/{'+'.join(want)}", ops.limiter_bwd(x, g, lc, h, D, H, compensate=comp, want=want))
    cut = L // 2 + 5
    y0, s0 = ops.limiter(x[..., :cut], lc, h, D, H, return_state=True)
    y1, s1 = ops.limiter(x[..., cut:], lc, h, D, H, state=s0)
    put("limiter/blocks", (y0, s0, y1, s1))


def moddelay():
    V, Dmax = 2, 8
    L = 2 * ops.moddelay_tile(Dmax, C) + 17
    x = torch.randn(R, C, L, generator=gen(3)).cuda()
    g = torch.randn(R, C, L, generator=gen(4)).cuda()
    q = gen(5)
    delay = 3.0 + 2.0 * torch.rand(R, V, generator=q)
    depth = 0.5 + torch.rand(R, V, generator=q)
    rate = (0.4 / (2 * math.pi * depth.double())).float() * torch.rand(R, V, generator=q)
    params = tuple(t.cuda() for t in (delay, depth, rate, torch.rand(R, V, C, generator=q), torch.randn(R, V, C, generator=q) / V,
                                      torch.tensor([0.5, 1.0, 0.0])))
    for interp in ("linear", "cubic"):
        tag = f"moddelay/{interp}"
        put(f"{tag}/fwd", ops.moddelay(x, *params, Dmax, interp))
        for want in (ops.MODDELAY_GRADS, *((n,) for n in ops.MODDELAY_GRADS)):
            put(f"{tag}/bwd/{'+'.join(want)}", ops.moddelay_bwd(x, g, *params, Dmax, interp, want=want))
        cut = L // 2 + 5
        y0, s0 = ops.moddelay(x[..., :cut], *params, Dmax, interp, return_state=True)
        y1, s1 = ops.moddelay(x[..., cut:], *params, Dmax, interp, state=s0)
        put(f"{tag}/blocks", (y0, s0, y1, s1))


def fbdelay():
    Dmax = 128
    L = 2 * 2048 + 17
    for Cc in (1, 2):
        x = torch.randn(R, Cc, L, generator=gen(6 + Cc)).cuda()
        g = torch.randn(R, Cc, L, generator=gen(8 + Cc)).cuda()
        q = gen(10 + Cc)
        delay = 64.0 + 64.0 * torch.rand(R, Cc, generator=q)
        damping = 0.8 * torch.rand(R, Cc, generator=q)
        fb = (torch.rand(R, Cc, Cc, generator=q) - 0.5) * (1.6 / Cc)
        params = tuple(t.cuda() for t in (delay, damping, fb, torch.tensor([0.5, 1.0, 0.0]), torch.tensor([1.0, 0.3, 0.7])))
        tag = f"fbdelay/C={Cc}"
        y, (qs, w) = ops.fbdelay(x, *params, Dmax, tape=True)
        put(f"{tag}/fwd", (y, qs, w))
        for want in (ops.FBDELAY_GRADS, *((n,) for n in ops.FBDELAY_GRADS)):
            put(f"{tag}/bwd/{'+'.join(want)}", ops.fbdelay_bwd(x, g, qs, w, *params, Dmax, want=want))
        cut = L // 2 + 5
        y0, s0 = ops.fbdelay(x[..., :cut], *params, Dmax, return_state=True)
        y1, s1 = ops.fbdelay(x[..., cut:], *params, Dmax, state=s0)
        put(f"{tag}/blocks", (y0, s0, y1, s1))


def shapers():
    L = 1000
    x = (torch.rand(R, C, L, generator=gen(20)) * 1.8 - 0.9).cuda()
    g = torch.randn(R, C, L, generator=gen(21)).cuda()
    q = gen(22)
    pre, post = (-0.5 * torch.rand(R, 1, generator=q)).cuda(), (0.3 * torch.randn(R, 1, generator=q)).cuda()
    modes = {
        "tanh": (ops.WS_TANH, dict(p0=(0.3 * torch.randn(R, 1, generator=q)).cuda())),
        "piecewise": (ops.WS_PIECEWISE, dict(p0=(0.3 * torch.randn(R, 2, generator=q)).cuda(),
                                             p1=(0.5 * torch.randn(R, 2, generator=q)).cuda())),
        "power": (ops.WS_POWER, dict(p0=(0.5 * torch.randn(R, 6, generator=q)).cuda(), use_tanh=True)),
        "chebyshev": (ops.WS_CHEBYSHEV, dict(p0=(0.5 * torch.randn(R, 10, generator=q)).cuda())),
    }
    m = P.TanhDistortion(oversample=2).cuda()
    over = (2, m.os_h_up, m.os_offset_up, m.os_h_dn, m.os_offset_dn)
    for name, (mode, kw) in modes.items():
        given = ["log_pre_gain", "log_post_gain"] + [k for k in ("p0", "p1") if k in kw]
        for dc in (False, True):
            for what, fwd, bwd, extra in (("waveshaper", ops.waveshaper, ops.waveshaper_bwd, ()),
                                          ("oversampled", ops.oversampled_waveshaper, ops.oversampled_waveshaper_bwd, over)):
                tag = f"{what}/{name}/dc={dc}"
                args = dict(log_pre_gain=pre, log_post_gain=post, remove_dc=dc, **kw)
                put(f"{tag}/fwd", fwd(x, mode, *extra, **args))
                for want in (ops.WS_GRADS, ("x",), *((n,) for n in given)):
                    put(f"{tag}/bwd/{'+'.join(want)}", bwd(x, g, mode, *extra, want=want, **args))
        put(f"waveshaper/{name}/inverse_post", ops.waveshaper_bwd(x, g, mode, log_pre_gain=pre, inverse_post_gain=True, **kw))
        put(f"oversampled/{name}/inverse_post",
            ops.oversampled_waveshaper_bwd(x, g, mode, *over, log_pre_gain=pre, inverse_post_gain=True, **kw))


def compare(pa, pb):
    a, b = json.load(open(pa)), json.load(open(pb))
    if a.keys() != b.keys():
        sys.exit(f"the two files hold other cases: {sorted(set(a) ^ set(b))[:10]}")
    bad = [k for k in a if a[k] != b[k]]
    n = sum(v is not None for v in a.values())
    print(f"digests: {n} per library, {len(a) - n} results that are None in both, {len(bad)} differ")
    for k in bad[:40]:
        print("DIFFERS", k)
    sys.exit(1 if bad else 0)


def main():
    if sys.argv[1] == "--compare":
        compare(*sys.argv[2:4])
    for fn in (limiter, moddelay, fbdelay, shapers):
        fn()
    torch.cuda.synchronize()
    with open(sys.argv[1], "w") as f:
        json.dump(OUT, f, indent=0, sort_keys=True)
    print(f"{sys.argv[1]}: {len(OUT)} entries, {sum(v is not None for v in OUT.values())} digests, "
          f"library {os.environ.get('GRAFX_AMD_LIB') or 'the default one'}")


if __name__ == "__main__":
    main()
