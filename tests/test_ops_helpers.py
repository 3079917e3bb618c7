"""The checks every wrapper of grafx_amd.ops shares (grafx_amd/_plumbing.py and the readers in ops.py), on CPU tensors:
none of them launches anything, and only the state check itself asks for a GPU tensor."""
import pytest
import torch

from grafx_amd import ops
from grafx_amd.ops import (_apart, _cotangent, _int_in, _output, _pair_state, _param_grads, _Pin, _read_mix, _row_chunks,
                           _signal_grad, _state, _taps, _want, _workspace, rowmap)

SHAPE = (2, 2, 64)
CPU = torch.device("cpu")


def _same_map(a, b):
    return all(getattr(a, f) == getattr(b, f) for f, _ in a._fields_)


def test_output_allocates_and_accepts():
    out, omap = _output(None, SHAPE, CPU, "t")
    assert out.shape == SHAPE and out.dtype == torch.float32 and _same_map(omap, rowmap(out)[0])
    plain = torch.zeros(SHAPE)
    buf = torch.zeros(1, 6, 2, 64)
    for t in (plain, buf[:, 2:4]):
        for longer in (False, True):
            got, omap = _output(t, SHAPE, CPU, "t", longer=longer)
            assert got is t and _same_map(omap, rowmap(t)[0])
    assert _output(torch.zeros(2, 2, 65), SHAPE, CPU, "t", longer=True)[0].shape[-1] == 65


@pytest.mark.parametrize("bad, longer", [
    (torch.zeros(1, 2, 64), False), (torch.zeros(3, 2, 64), True),                  # rows
    (torch.zeros(2, 1, 64), False), (torch.zeros(2, 3, 64), True),                  # channels
    (torch.zeros(2, 2, 63), False), (torch.zeros(2, 2, 63), True),                  # shorter
    (torch.zeros(2, 2, 65), False),                                                 # longer, where equality is asked
    (torch.zeros(1, 6, 2, 64)[:, 2:5], False), (torch.zeros(2, 2, 128)[..., ::2], False),   # 3 nodes; a last stride of 2
])
def test_output_refuses(bad, longer):
    with pytest.raises(ValueError):
        _output(bad, SHAPE, CPU, "t", longer=longer)


def test_output_apart():
    buf = torch.zeros(1, 6, 2, 64)
    x = buf[:, 2:4]
    with pytest.raises(ValueError, match="share memory"):
        _output(x, SHAPE, CPU, "t", apart=(x,))
    with pytest.raises(ValueError, match="share memory"):
        _output(buf[:, 3:5], SHAPE, CPU, "t", apart=(x,))
    assert _output(buf[:, 4:6], SHAPE, CPU, "t", apart=(x,))[0].data_ptr() == buf[:, 4:6].data_ptr()
    assert _output(x, SHAPE, CPU, "t")[0] is x          # no list, no refusal
    assert _output(buf[:, 4:6], SHAPE, CPU, "t", apart=(x, None, buf[:, 0:2]))[0] is not None    # None: an argument not given


def test_output_refuses_a_destination_that_overlaps_itself():
    """Several rows of an expanded view are the same floats: torch refuses such a destination for its own ops."""
    row = torch.zeros(1, 1, 2, 64)
    for bad in (row.expand(1, 2, 2, 64), torch.zeros(2, 1, 64).expand(2, 2, 64), torch.zeros(256).as_strided((2, 2, 64), (64, 32, 1))):
        with pytest.raises(ValueError, match="share memory"):
            _output(bad, SHAPE, CPU, "t")
    assert not bool(row.any())


def test_apart_checks_what_is_written_beside_out():
    buf = torch.zeros(1, 6, 2, 64)
    x, state = buf[:, 2:4], torch.zeros(2, 2, 8)
    _apart("t", "tee", None, (x,))
    _apart("t", "tee", buf[:, 4:6], (x, None))
    _apart("t", "zf", state, (x, torch.zeros(2, 2, 8)))
    for name, t, apart in (("tee", buf[:, 3:5], (x,)), ("zf", state, (x, state)), ("zf", state.view(-1)[8:24], (state,)),
                           ("u1_out", buf.view(-1)[256:512].view(2, 128), (x,)), ("tee", buf[:, :1].expand(1, 2, 2, 64), ())):
        with pytest.raises(ValueError, match=f"t: .*{name}.* share memory"):
            _apart("t", name, t, apart)


def test_state_refusals_name_entry_argument_shape_and_value():
    assert _state(None, SHAPE, "entry", "zi") is None
    for bad in ([0.0] * 4, torch.zeros(SHAPE, dtype=torch.float64), torch.zeros(2, 2, 63), torch.zeros(2, 64, 2).transpose(1, 2),
                torch.zeros(SHAPE)):            # the last: everything right but the device
        with pytest.raises(ValueError, match=r"entry: zi must be .*\(2, 2, 64\).*got") as e:
            _state(bad, SHAPE, "entry", "zi")
        assert ("list" if isinstance(bad, list) else str(bad.dtype)) in str(e.value)


@pytest.mark.gpu
def test_state_on_the_gpu():
    good = torch.zeros(SHAPE, device="cuda")
    assert _state(good, SHAPE, "entry", "zf") is good
    for bad in (good.double(), good[:, :, :63], torch.zeros(2, 64, 2, device="cuda").transpose(1, 2)):
        with pytest.raises(ValueError, match=r"entry: zf must be .*\(2, 2, 64\)"):
            _state(bad, SHAPE, "entry", "zf")


def test_workspace_made_when_none_is_given():
    pin = _Pin()
    ptr, nbytes = _workspace("t", None, 64, CPU, pin, ())
    assert nbytes == 64 and pin.ws.dtype == torch.uint8 and pin.ws.numel() == 64 and ptr == pin.ws.data_ptr() != 0
    empty = _Pin()
    assert _workspace("t", None, 0, CPU, empty, ()) == (0, 0) and empty.ws is None


def test_workspace_of_the_caller():
    pin, x = _Pin(), torch.zeros(SHAPE)
    ws = torch.empty(64, dtype=torch.uint8)
    assert _workspace("t", ws, 64, CPU, pin, (x, None)) == (ws.data_ptr(), 64) and pin.ws is None
    longer = torch.empty(100, dtype=torch.uint8)
    assert _workspace("t", longer, 64, CPU, pin, ()) == (longer.data_ptr(), 100)      # the entry is told all of it
    with pytest.raises(ValueError, match="t: .*workspace.* 64 "):
        _workspace("t", torch.empty(63, dtype=torch.uint8), 64, CPU, pin, ())
    with pytest.raises(ValueError, match="uint8"):
        _workspace("t", torch.empty(16, dtype=torch.float32), 64, CPU, pin, ())
    with pytest.raises(ValueError, match="workspace"):
        _workspace("t", torch.empty(128, dtype=torch.uint8)[::2], 64, CPU, pin, ())
    with pytest.raises(ValueError, match="workspace"):                                  # everything right but the device
        _workspace("t", ws, 64, torch.device("cuda", 0), pin, ())
    off = torch.empty(80, dtype=torch.uint8)[8:72]
    assert off.data_ptr() % 16 == 8
    with pytest.raises(ValueError, match="workspace.*16-byte aligned"):
        _workspace("t", off, 64, CPU, pin, (), align=16)
    assert _workspace("t", off, 64, CPU, pin, (), align=1) == (off.data_ptr(), 64)
    with pytest.raises(ValueError, match="workspace") as e:                             # (no alignment asked, none named)
        _workspace("t", off[:63], 64, CPU, pin, ())
    assert "aligned" not in str(e.value)
    with pytest.raises(ValueError, match="t: ws must not share memory"):
        _workspace("t", x.view(torch.uint8).view(-1)[64:128], 64, CPU, pin, (None, x))
    with pytest.raises(ValueError, match="share memory"):                               # the aliasing rule comes first
        _workspace("t", x.view(torch.uint8).view(-1)[:63], 64, CPU, pin, (x,))


def test_int_in():
    lo, hi = 1, 16
    for good in (lo, hi, 7):
        _int_in("t", "factor", good, lo, hi)
    for bad in (True, 3.0, "3", None, lo - 1, hi + 1):
        with pytest.raises(ValueError, match=r"t: factor=.* must be an integer in 1\.\.16") as e:
            _int_in("t", "factor", bad, lo, hi)
        assert f"factor={bad!r}" in str(e.value)


class _SaysGpu(torch.Tensor):
    """A CPU tensor that answers ``is_cuda`` with True: the shape and count checks of _taps come after the device's."""
    is_cuda = property(lambda self: True)


def test_taps():
    on_gpu = lambda t: t.as_subclass(_SaysGpu)  # noqa: E731
    _taps("t", "h", on_gpu(torch.zeros(1)), 8)
    _taps("t", "h", on_gpu(torch.zeros(8)), 8)
    for bad in ([0.0] * 4, None, torch.zeros(4), on_gpu(torch.zeros(4, dtype=torch.float64))):   # type, device, dtype
        with pytest.raises(TypeError, match="t: h_up must be a float32 tensor on the GPU"):
            _taps("t", "h_up", bad, 8)
    for bad in (torch.zeros(2, 2), torch.zeros(0), torch.zeros(9)):                               # 2-D, no tap, one too many
        with pytest.raises(ValueError, match=r"t: h must hold 1\.\.8 taps"):
            _taps("t", "h", on_gpu(bad), 8)


def test_want():
    _want("t", (), ("x", "p0"))
    _want("t", ["p0", "x"], ("x", "p0"))
    with pytest.raises(ValueError, match=r"t: unknown gradients \['h_up'\] \(known: \('x', 'p0'\)\)"):
        _want("t", ("x", "h_up"), ("x", "p0"))
    _want("t", ["p0"], ("x", "p0"), some=True)
    for nothing in ((), []):
        with pytest.raises(ValueError, match=r"^t: no gradient asked for$"):
            _want("t", nothing, ("x", "p0"), some=True)
    with pytest.raises(ValueError, match="unknown gradients"):                          # the unknown name comes first
        _want("t", ("h_up",), ("x", "p0"), some=True)


def test_cotangent():
    x, buf = torch.zeros(SHAPE), torch.zeros(1, 6, 2, 64)
    for gy in (torch.zeros(SHAPE), buf[:, 2:4]):
        assert _same_map(_cotangent("t", gy, x, SHAPE), rowmap(gy)[0])
    for bad in (torch.zeros(2, 2, 63), torch.zeros(2, 1, 64), torch.zeros(3, 2, 64), buf[:, 2:5]):
        with pytest.raises(ValueError, match=r"t: gradient \(.*\) does not match the input \(2, 2, 64\)"):
            _cotangent("t", bad, x, SHAPE)
    with pytest.raises(ValueError, match="last dimension must be contiguous"):
        _cotangent("t", torch.zeros(2, 2, 128)[..., ::2], x, SHAPE)


def test_signal_grad():
    buf = torch.zeros(1, 8, 2, 64)
    x, gy, free = buf[:, 0:2], buf[:, 2:4], buf[:, 4:6]
    ws = buf[:, 6:8].reshape(-1).view(torch.uint8)
    xmap = rowmap(x)[0]
    gx, gxmap = _signal_grad("t", ("x", "p0"), None, SHAPE, xmap, CPU, (x, gy, ws))      # wanted, no out: a new tensor
    assert gx.shape == SHAPE and gx.dtype == torch.float32 and _same_map(gxmap, rowmap(gx)[0])
    gx, gxmap = _signal_grad("t", ("x",), free, SHAPE, xmap, CPU, (x, gy, ws))           # wanted, into out
    assert gx is free and _same_map(gxmap, rowmap(free)[0])
    assert _signal_grad("t", ("p0",), None, SHAPE, xmap, CPU, (x, gy, ws)) == (None, xmap)   # not wanted: the input's row map
    assert _signal_grad("t", ("p0",), free, SHAPE, xmap, CPU, (x, gy, ws)) == (None, xmap)   # ... whatever out is
    for want in (("x", "p0"), ("p0",)):                          # out is checked whether or not "x" is wanted
        for bad in (x, gy, buf[:, 1:3], buf[:, 6:8]):            # the input, the cotangent, half of each, the workspace
            with pytest.raises(ValueError, match="t: out must not share memory"):
                _signal_grad("t", want, bad, SHAPE, xmap, CPU, (x, gy, ws))
        with pytest.raises(ValueError, match="t: out .* does not match rows=2, channels=2, length=64"):
            _signal_grad("t", want, torch.zeros(2, 2, 63), SHAPE, xmap, CPU, (x, gy, ws))


def test_param_grads():
    shapes = {"delay": (3, 2), "phase": (3, 2, 2), "dry": (3,)}
    grads = _param_grads(("x", "phase", "dry"), shapes, CPU)
    assert grads[0] is None and [tuple(g.shape) for g in grads[1:]] == [(3, 2, 2), (3,)]
    assert all(g.dtype == torch.float32 and g.is_contiguous() for g in grads[1:])
    assert _param_grads(("x",), shapes, CPU) == [None, None, None] == _param_grads((), shapes, CPU)
    assert [tuple(g.shape) for g in _param_grads(["dry", "delay", "phase"], shapes, CPU)] == list(shapes.values())   # shapes' order


def test_pair_state():
    on_gpu = lambda t: t.as_subclass(_SaysGpu)  # noqa: E731
    shape, seen = (2, 2, 8), []

    def position(pos):
        seen.append(pos)
        if pos == "bad":
            raise ValueError("t: the state's position must be right")
        return pos

    assert _pair_state("t", None, shape, "position", position) == (None, None) and not seen
    hist = on_gpu(torch.zeros(shape))
    for state in ((hist, 7), [hist, 7]):
        zi, pos = _pair_state("t", state, shape, "position", position)
        assert zi is hist and pos == 7
    for bad in (hist, (hist,), (hist, 7, 7), "ab", {0: hist, 1: 7}, (None, 7), (hist, None), (None, None)):
        with pytest.raises(ValueError, match=r"^t: state must be the pair \(history, position\)$"):
            _pair_state("t", bad, shape, "position", position)
    with pytest.raises(ValueError, match=r"^t: state must be the pair \(history, q_last\)$"):
        _pair_state("t", (hist,), shape, "q_last", position)
    with pytest.raises(ValueError, match=r"t: the state's history must be .*\(2, 2, 8\).*got \(2, 2, 7\)"):
        _pair_state("t", (on_gpu(torch.zeros(2, 2, 7)), 7), shape, "position", position)
    with pytest.raises(ValueError, match="t: the state's position must be right"):      # the second part's own message
        _pair_state("t", (hist, "bad"), shape, "position", position)


@pytest.mark.parametrize("limit", [1, 3, ops.GRID_ROWS_I16_MAX, ops.GRID_YZ_MAX])
def test_row_chunks(limit):
    assert list(_row_chunks(0, limit)) == []
    assert list(_row_chunks(limit, limit)) == [(0, limit)]
    assert list(_row_chunks(limit + 1, limit)) == [(0, limit), (limit, 1)]
    assert (ops.GRID_ROWS_I16_MAX, ops.GRID_YZ_MAX) == (32767, 65535)


def _inline_mix(mix, B, n, C, L):
    """The reading dynamics_fused and stereo_gain each spelled out before they shared _read_mix."""
    mo, sched = mix["out"], mix["sched"]
    if not (mo.shape == (B, mo.shape[1], C, L) and mo.stride(-1) == 1 and sched.numel() == n):
        return None
    ex = mix.get("extras")
    n_ex = 0 if ex is None else ex.shape[0]
    n_pre = mix.get("n_pre", 0)
    return mo, sched, mix["n_acc"], ex, n_pre, n_ex - n_pre, bool(mix.get("skip_rows"))


def test_read_mix():
    B, n, C, L = 2, 3, 2, 64
    sched = torch.arange(n)
    with_extras = {"out": torch.zeros(B, 8, C, L)[:, 1:3], "sched": sched, "n_acc": 2, "extras": torch.zeros(5, 2, dtype=torch.int64),
                   "n_pre": 2, "skip_rows": True}
    without = {"out": torch.zeros(B, 2, C, L), "sched": sched, "n_acc": 1}
    for mix in (with_extras, without):
        got, want = _read_mix(mix, B, n, C, L), _inline_mix(mix, B, n, C, L)
        assert tuple(got)[2:3] + tuple(got)[4:] == want[2:3] + want[4:]
        assert got.out is want[0] and got.sched is want[1] and got.extras is want[3]
    assert (_read_mix(with_extras, B, n, C, L).n_pre, _read_mix(with_extras, B, n, C, L).n_post) == (2, 3)
    assert (_read_mix(without, B, n, C, L).extras, _read_mix(without, B, n, C, L).n_post) == (None, 0)
    for wrong in ((B + 1, n, C, L), (B, n + 1, C, L), (B, n, 1, L), (B, n, C, L + 1)):    # each entry's shape conditions
        assert _read_mix(without, *wrong) is None and _inline_mix(without, *wrong) is None
    assert _read_mix({**without, "out": torch.zeros(B, 2, C, 2 * L)[..., ::2]}, B, n, C, L) is None
