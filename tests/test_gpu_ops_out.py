"""dynamics_fused, biquad_cascade and waveshaper check a caller's ``out=`` like every other entry (ops._output): a
destination with the wrong rows, channels or length is refused in Python, before any pointer reaches the library -- a
RowMap carries strides only, so the kernel would have written past it -- and a correct strided view of the render's
(B, V, C, L) buffer gives the bits of the call without ``out``."""
import pytest
import torch

pytestmark = pytest.mark.gpu

R, C, L = 2, 2, 64
SENTINEL = -7.0


def _entries():
    from grafx_amd import ops

    g = torch.Generator().manual_seed(11)
    x = torch.randn(R, C, L, generator=g).cuda()
    p = [(0.3 * torch.randn(R, generator=g)).cuda() for _ in range(4)]
    rad, th = 0.5 + 0.4 * torch.rand(R, C, 1, generator=g), 3.0 * torch.rand(R, C, 1, generator=g)
    As = torch.stack([torch.ones_like(rad), -2 * rad * torch.cos(th), rad * rad], -1).cuda()
    Bs = torch.stack([torch.ones_like(rad), -1.6 * torch.cos(th), 0.64 * torch.ones_like(rad)], -1).cuda()
    pre, bias = (0.3 * torch.randn(R, 1, generator=g)).cuda(), (0.1 * torch.randn(R, 1, generator=g)).cuda()
    return x, {"dynamics_fused": lambda x, out: ops.dynamics_fused(x, *p, 1, 33, "quadratic", False, out=out),
               "biquad_cascade": lambda x, out: ops.biquad_cascade(x, Bs, As, out=out),
               "waveshaper": lambda x, out: ops.waveshaper(x, ops.WS_TANH, pre, None, p0=bias, out=out)}


@pytest.mark.parametrize("name", ["dynamics_fused", "biquad_cascade", "waveshaper"])
def test_wrong_out_is_refused_before_the_launch(name):
    x, entries = _entries()
    for shape in ((R - 1, C, L), (R, C - 1, L), (R, C + 1, L), (R, C, L - 1)):     # a row too few, channels, length 63
        out = torch.full(shape, SENTINEL, device="cuda")
        with pytest.raises(ValueError, match=name):
            entries[name](x, out)
        torch.cuda.synchronize()
        assert bool((out == SENTINEL).all()), f"{name}: a refused out {shape} was written"


@pytest.mark.parametrize("name", ["dynamics_fused", "biquad_cascade", "waveshaper"])
def test_strided_out_view_gives_the_bits_of_a_new_tensor(name):
    x, entries = _entries()
    want = entries[name](x, None)
    buf = torch.full((1, 6, C, L), SENTINEL, device="cuda")
    buf[:, 0:2] = x.view(1, R, C, L)
    got = entries[name](buf[:, 0:2], buf[:, 2:4])
    assert got.data_ptr() == buf[:, 2:4].data_ptr()
    assert torch.equal(buf[:, 2:4].reshape(R, C, L).view(torch.int32), want.view(torch.int32))
    assert bool((buf[:, 4:6] == SENTINEL).all())          # and nothing behind the view
