"""The native STFT loss on the GPU against its float64 definition (tests/stft_loss_float64.py): the sums and the gradient of
the two ops entries at the shapes where the kernels can go wrong, the module end to end, the guarantees on bits, memory and
layouts, and the refusals."""
import pytest
import torch
from conftest import assert_close

import stft_loss_float64 as f64

pytestmark = pytest.mark.gpu
TOL = 1e-5
NAMES = "ABED"      # the order of the four sums


def ident(shape):
    return "{}/{}/{}".format(*shape[:3])


def window(n_fft):
    return f64.hann(n_fft, dtype=torch.float32).cuda()


def on_gpu(n_fft, hop, L, kind):
    return tuple(x.cuda() for x in f64.inputs(n_fft, hop, L, kind))


# ------------------------------------------------------------------------------------------------ 1: the sums
@pytest.mark.parametrize("kind", f64.KINDS)
@pytest.mark.parametrize("shape", f64.SHAPES, ids=ident)
def test_sums_match_float64(shape, kind):
    from grafx_amd import ops

    n_fft, hop, L, eps = shape
    pred, target = on_gpu(n_fft, hop, L, kind)
    got = ops.stft_loss_sums(pred, target, window(n_fft), hop, eps)
    want, _ = f64.reference(n_fft, hop, L, eps, kind)
    assert got.shape == (f64.ROWS, 4) and got.dtype == torch.float32
    for r in range(f64.ROWS):
        for c, name in enumerate(NAMES):
            print(f"{ident(shape)} {kind} row {r} {name}: {float(got[r, c]):.9g} vs {float(want[r, c]):.9g}")
            assert_close(got[r, c].reshape(1), want[r, c].reshape(1), TOL, f"{name} of row {r}")


# ------------------------------------------------------------------------------------------------ 2: the gradient
GRADIENT_CASES = ([(s, k, ("A", "E", "D", "random")) for s in f64.FLOORED for k in ("half", "double")]
                  + [(s, "noise", ("A", "E", "D", "random")) for s in f64.SMALL]
                  + [(f64.DEFAULT_EPS, "noise", ("A",))])


@pytest.mark.parametrize("shape,kind,coefs", GRADIENT_CASES, ids=[f"{ident(s)}-{k}" for s, k, _ in GRADIENT_CASES])
def test_gradient_matches_float64_autograd(shape, kind, coefs):
    from grafx_amd import ops

    n_fft, hop, L, eps = shape
    pred, target = on_gpu(n_fft, hop, L, kind)
    for name in coefs:
        coef = f64.coefficients(name, n_fft + hop + L).cuda()
        got = ops.stft_loss_bwd(pred, target, window(n_fft), hop, coef, eps)
        _, want = f64.reference(n_fft, hop, L, eps, kind, name)
        assert got.shape == pred.shape
        assert_close(got, want, TOL, f"gradient for coefficients {name}")


# ------------------------------------------------------------------------------------------------ 3, 4: the module
RESOLUTIONS = ((512, 50, 512), (128, 32, 128))
WEIGHTS = dict(w_sc=1.0, w_log_mag=0.7, w_lin_mag=0.3)


def module_inputs(stereo):
    """The s = 0.5 input at L = 20001 (512/50/20001's draw): three rows, or (2, 2, L) cut from four rows of one draw."""
    if not stereo:
        return f64.inputs(512, 50, 20001, "half")
    target, noise = f64.draw(512, 50, 20001, rows=4)
    return (0.5 * target + 0.02 * noise).view(2, 2, -1), target.view(2, 2, -1).clone()


def graph_names(fn):
    seen, todo, names = set(), [fn], []
    while todo:
        f = todo.pop()
        if f is None or f in seen:
            continue
        seen.add(f)
        names.append(type(f).__name__)
        todo += [g for g, _ in f.next_functions]
    return names


@pytest.mark.parametrize("stereo", [False, True], ids=["rows", "sum_and_difference"])
def test_module_matches_float64_and_trains_on_the_native_node(stereo):
    from grafx_amd.losses import MultiResolutionSTFTLoss

    pred, target = module_inputs(stereo)
    want, want_grad = f64.loss_and_grad(pred, target, RESOLUTIONS, 1.0, 0.7, 0.3, 1.0, sum_and_difference=stereo)
    module = MultiResolutionSTFTLoss([r[0] for r in RESOLUTIONS], [r[1] for r in RESOLUTIONS], eps=1.0,
                                     sum_and_difference=stereo, **WEIGHTS).cuda()
    assert not list(module.parameters())
    p = pred.cuda().requires_grad_(True)
    loss = module(p, target.cuda())
    names = graph_names(loss.grad_fn)
    assert "StftLossSumsFnBackward" in names
    assert not [n for n in names if "stft" in n.lower().replace("stftlosssumsfn", "") or "fft" in n.lower()], names
    loss.backward()
    assert_close(loss.detach().reshape(1), want.reshape(1), TOL, "loss")
    assert_close(p.grad, want_grad, TOL, "pred.grad")


def test_identical_signals_give_zero_loss_and_an_exactly_zero_gradient():
    from grafx_amd import ops
    from grafx_amd.losses import MultiResolutionSTFTLoss

    target = f64.draw(512, 50, 20001)[0].cuda()
    pred = target.clone().requires_grad_(True)
    loss = MultiResolutionSTFTLoss((512, 128), (50, 32), w_lin_mag=1.0).cuda()(pred, target)
    loss.backward()
    assert loss.item() == 0.0
    assert torch.isfinite(pred.grad).all() and torch.count_nonzero(pred.grad) == 0
    sums = ops.stft_loss_sums(target, target, window(512), 50)
    assert torch.count_nonzero(sums[:, (0, 2, 3)]) == 0 and (sums[:, 1] > 0).all()


# ------------------------------------------------------------------------------------------------ 5: bits
def test_results_are_the_same_bits_whatever_the_workspace_held_and_on_a_side_stream():
    from grafx_amd import ops

    n_fft, hop, L, eps = f64.SHAPES[4]
    pred, target = on_gpu(n_fft, hop, L, "half")
    w, coef = window(n_fft), f64.coefficients("random", 7).cuda()
    sums, grad = ops.stft_loss_sums(pred, target, w, hop, eps), ops.stft_loss_bwd(pred, target, w, hop, coef, eps)
    assert torch.equal(sums, ops.stft_loss_sums(pred, target, w, hop, eps))
    assert torch.equal(grad, ops.stft_loss_bwd(pred, target, w, hop, coef, eps))
    ws = torch.full((ops.stft_loss_ws_bytes(f64.ROWS, L, n_fft, hop),), 0xFF, dtype=torch.uint8, device="cuda")
    assert torch.equal(sums, ops.stft_loss_sums(pred, target, w, hop, eps, ws=ws))
    ws.fill_(0xFF)
    assert torch.equal(grad, ops.stft_loss_bwd(pred, target, w, hop, coef, eps, ws=ws))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        sums_side, grad_side = ops.stft_loss_sums(pred, target, w, hop, eps), ops.stft_loss_bwd(pred, target, w, hop, coef, eps)
    side.synchronize()
    assert torch.equal(sums, sums_side) and torch.equal(grad, grad_side)


# ------------------------------------------------------------------------------------------------ 6: accumulate
def test_accumulate_adds_to_the_buffer_and_a_plain_call_overwrites_all_of_it():
    from grafx_amd import ops

    n_fft, hop, L, eps = f64.SHAPES[1]
    pred, target = on_gpu(n_fft, hop, L, "half")
    w, coef = window(n_fft), f64.coefficients("random", 3).cuda()
    plain = ops.stft_loss_bwd(pred, target, w, hop, coef, eps)
    held = torch.randn(f64.ROWS, L, generator=torch.Generator().manual_seed(5)).cuda() * plain.abs().max()
    buf = held.clone()
    assert ops.stft_loss_bwd(pred, target, w, hop, coef, eps, out=buf, accumulate=True) is buf
    assert float((buf - (held + plain)).abs().max()) <= 1e-6 * float((held + plain).abs().max())
    buf.fill_(float("nan"))
    ops.stft_loss_bwd(pred, target, w, hop, coef, eps, out=buf)
    assert torch.equal(buf, plain)
    with pytest.raises(ValueError, match="accumulate"):
        ops.stft_loss_bwd(pred, target, w, hop, coef, eps, accumulate=True)
    # a workspace the entries would answer with a bare error code, 8 bytes off the 16 they need: refused by name
    nbytes = ops.stft_loss_ws_bytes(f64.ROWS, L, n_fft, hop)
    ws = torch.empty(nbytes + 16, dtype=torch.uint8, device="cuda")[8:]
    with pytest.raises(ValueError, match="workspace"):
        ops.stft_loss_sums(pred, target, w, hop, eps, ws=ws)
    with pytest.raises(ValueError, match="workspace"):
        ops.stft_loss_bwd(pred, target, w, hop, coef, eps, out=buf, ws=ws)
    assert torch.equal(buf, plain)


# ------------------------------------------------------------------------------------------------ 7: layouts
def test_a_strided_view_is_read_in_place_and_a_grad_sink_is_written_once():
    from grafx_amd import autograd, ops
    from grafx_amd.losses import MultiResolutionSTFTLoss

    n_fft, hop, L, eps = f64.SHAPES[1]
    target, noise = f64.draw(n_fft, hop, L, rows=4)
    flat_pred, flat_target = (0.5 * target + 0.02 * noise).cuda(), target.cuda()
    big = torch.full((2, 5, 2, L + 24), float("nan"), device="cuda")         # a render buffer: (B, V, C, L) with room to spare
    view = big[:, 3, :, 8:8 + L]
    view.copy_(flat_pred.view(2, 2, L))
    assert not view.is_contiguous()
    before = big.clone()
    w, coef = window(n_fft), f64.coefficients("random", 11, rows=4).cuda()
    want_sums, want_grad = ops.stft_loss_sums(flat_pred, flat_target, w, hop, eps), ops.stft_loss_bwd(flat_pred, flat_target, w, hop, coef, eps)
    ptr = view.data_ptr()
    assert torch.equal(ops.stft_loss_sums(view, flat_target.view(2, 2, L), w, hop, eps), want_sums)
    grad = ops.stft_loss_bwd(view, flat_target.view(2, 2, L), w, hop, coef, eps)
    assert grad.shape == (2, 2, L) and torch.equal(grad.view(4, L), want_grad)
    assert view.data_ptr() == ptr and torch.equal(torch.nan_to_num(big, nan=7.0), torch.nan_to_num(before, nan=7.0))
    # a strided destination, and one that shares memory with what is read
    dest_big = torch.zeros_like(big)
    dest = dest_big[:, 1, :, 4:4 + L]
    ops.stft_loss_bwd(view, flat_target.view(2, 2, L), w, hop, coef, eps, out=dest)
    assert torch.equal(dest.reshape(4, L), want_grad)
    dest.zero_()
    assert torch.count_nonzero(dest_big) == 0               # nothing was written beside the destination
    with pytest.raises(ValueError, match="share memory"):
        ops.stft_loss_bwd(view, flat_target.view(2, 2, L), w, hop, coef, eps, out=big[:, 3, :, 12:12 + L])
    # through autograd: the node writes the gradient of a registered input straight into its sink, once
    module = MultiResolutionSTFTLoss((n_fft,), (hop,), eps=eps).cuda()
    leaf = flat_pred.view(2, 2, L).clone().requires_grad_(True)
    module(leaf, flat_target.view(2, 2, L)).backward()
    src = view.detach().requires_grad_(True)
    sink_big = torch.zeros_like(big)
    sink_view = sink_big[:, 2, :, :L]
    with autograd.grad_sink(src, sink_view) as sink:
        module(src, flat_target.view(2, 2, L)).backward()
        assert sink.writes == 1
    assert torch.equal(sink_view, leaf.grad) and torch.equal(src.grad, leaf.grad)


# ------------------------------------------------------------------------------------------------ 8: many rows
def test_rows_beyond_the_grid_limit_equal_the_three_row_call():
    from grafx_amd import ops

    n_fft, hop, L, eps = f64.SHAPES[0]
    pred3, target3 = on_gpu(n_fft, hop, L, "half")
    R, at = 65537, (0, 65535, 65536)
    g = torch.Generator(device="cuda").manual_seed(8)
    pred, target = torch.randn(R, L, device="cuda", generator=g), torch.randn(R, L, device="cuda", generator=g)
    pred[list(at)], target[list(at)] = pred3, target3
    w = window(n_fft)
    coef = torch.rand(R, 3, device="cuda", generator=g) + 0.25
    coef3 = coef[list(at)].contiguous()
    sums, grad = ops.stft_loss_sums(pred, target, w, hop, eps), ops.stft_loss_bwd(pred, target, w, hop, coef, eps)
    assert torch.equal(sums[list(at)], ops.stft_loss_sums(pred3, target3, w, hop, eps))
    assert torch.equal(grad[list(at)], ops.stft_loss_bwd(pred3, target3, w, hop, coef3, eps))
    assert torch.isfinite(sums).all() and torch.isfinite(grad).all()


# ------------------------------------------------------------------------------------------------ 9: refusals
def test_refusals_and_the_torch_path_outside_the_native_range():
    from grafx_amd import ops
    from grafx_amd.losses import MultiResolutionSTFTLoss

    n_fft, hop, L, eps = f64.SHAPES[1]
    pred, target = on_gpu(n_fft, hop, L, "half")
    with pytest.raises(ValueError, match="target"):
        MultiResolutionSTFTLoss((n_fft,), (hop,), eps=eps).cuda()(pred, target.clone().requires_grad_(True))
    # n_fft = 384: torch.stft, said aloud, and still the float64 loss
    module = MultiResolutionSTFTLoss((n_fft, 384), (hop, 96), eps=eps, **WEIGHTS).cuda()
    p = pred.clone().requires_grad_(True)
    with pytest.warns(ops.FftLibraryWarning):
        loss = module(p, target)
    loss.backward()
    assert "StftLossSumsFnBackward" not in graph_names(loss.grad_fn)
    want, want_grad = f64.loss_and_grad(pred.cpu(), target.cpu(), ((n_fft, hop, n_fft), (384, 96, 384)), 1.0, 0.7, 0.3, eps)
    assert_close(loss.detach().reshape(1), want.reshape(1), TOL, "loss through torch_forward")
    assert_close(p.grad, want_grad, TOL, "gradient through torch_forward")
    # L = n_fft / 2: refused as torch.stft refuses it, by the module and by the ops
    short_p, short_t = pred[:, :n_fft // 2].contiguous(), target[:, :n_fft // 2].contiguous()
    with pytest.warns(ops.FftLibraryWarning), pytest.raises(RuntimeError):
        MultiResolutionSTFTLoss((n_fft,), (hop,), eps=eps).cuda()(short_p, short_t)
    with pytest.raises(ValueError, match="native range"):
        ops.stft_loss_sums(short_p, short_t, window(n_fft), hop, eps)
    with pytest.raises(RuntimeError, match="CPU tensor"):
        ops.stft_loss_sums(pred.cpu(), target.cpu(), window(n_fft).cpu(), hop, eps)


# ------------------------------------------------------------------------------------------------ 10: memory
def test_forward_and_backward_allocate_the_gradient_and_little_else():
    from grafx_amd import ops
    from grafx_amd.losses import MultiResolutionSTFTLoss

    n_fft, hop, L, eps = f64.SHAPES[4]
    R = 8
    target, noise = f64.draw(n_fft, hop, L, rows=R)
    pred = (0.5 * target + 0.02 * noise).cuda().requires_grad_(True)
    target = target.cuda()
    module = MultiResolutionSTFTLoss((n_fft,), (hop,), eps=eps).cuda()
    module(pred, target).backward()                       # first call: whatever the library sets up once
    pred.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    module(pred, target).backward()
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    bound = 1.5 * R * L * 4 + ops.stft_loss_ws_bytes(R, L, n_fft, hop)
    print(f"peak growth {growth} bytes, bound {bound:.0f} (one gradient tensor is {R * L * 4})")
    assert pred.grad is not None and growth <= bound


# ------------------------------------------------------------------------------------------------ 11: a processor
def test_parameter_gradients_through_a_processor_equal_those_of_the_torch_loss():
    from grafx_amd import processors as P
    from grafx_amd.losses import MultiResolutionSTFTLoss

    n_fft, hop, L, eps = f64.SHAPES[1]
    g = torch.Generator().manual_seed(1000 * n_fft + hop + L + 11)
    x = torch.randn(3, 2, L, generator=g).cuda()
    noise = torch.randn(3, 2, L, generator=g).cuda()
    params = {k: torch.randn(3, 1, generator=g).cuda() for k in ("w0", "q_inv")}
    lp = P.LowPassFilter(flashfftconv=False, fsm_fir_len=257).cuda()
    module = MultiResolutionSTFTLoss((n_fft,), (hop,), eps=eps, **WEIGHTS).cuda()
    grads = {}
    for path in ("native", "torch"):
        leaves = {k: v.clone().requires_grad_(True) for k, v in params.items()}
        y = lp(x, **leaves)
        target = 2.0 * y.detach() + 0.02 * noise
        loss = module(y, target) if path == "native" else module.torch_forward(y, target)
        assert ("StftLossSumsFnBackward" in graph_names(loss.grad_fn)) == (path == "native")
        loss.backward()
        grads[path] = {k: v.grad for k, v in leaves.items()}
    for k in params:
        print(k, grads["native"][k].flatten().tolist(), grads["torch"][k].flatten().tolist())
        assert_close(grads["native"][k], grads["torch"][k], TOL, f"gradient of {k}")
