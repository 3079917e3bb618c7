"""Stream-order helpers of tests/test_gpu_caller_stream.py: a device-side delay and the consumer-order check built on it.

The check: a call made on a side stream S must read what S wrote.  The inputs of the call are filled on S *behind a delay*;
a kernel that the wrapper launched on another stream (the default one, say) runs while S still waits and reads what the
inputs held before -- a second valid draw, so it does normal work on the wrong signal and the result differs.

The delay proves something only if it is still running when the wrapper returns to the host: `ordered_call` looks at the
delay's event right then and FAILS the case when it has finished (`Unproven`), it never passes it.  DELAY_MS is set from the
host enqueue times measured on the MI355X (EXPERIMENTS.md, "Caller streams"): at least five times the slowest covered call.
"""
import math
import os
import time

import torch

DELAY_MS = 20.0          # operator wrappers: the slowest warm call (odd_alias) enqueues in 0.29 ms, the median in 0.05 ms
RENDER_DELAY_MS = 100.0  # whole renders, replays and the training step (forward + backward enqueue in 3.0 ms)
HOST_MS = []             # (label, host milliseconds of the call, delay in milliseconds): what ordered_call measured

_RATE = {}               # "kind": "sleep" | "mm", "per_ms": sleep cycles / matrix products per millisecond, "a": the mm operand


class Unproven(AssertionError):
    """The delay had finished when the call returned: the case shows nothing about stream order."""


def _spin(kind, amount):
    if kind == "sleep":
        torch.cuda._sleep(int(amount))
    else:
        a = _RATE["a"]
        out = torch.empty_like(a)
        for _ in range(int(amount)):
            torch.mm(a, a, out=out)


def _calibrate():
    """Units of delay per millisecond, measured once per session with two events: torch.cuda._sleep where it is usable,
    a chain of 2048 x 2048 matrix products otherwise."""
    if _RATE:
        return
    _RATE["a"] = torch.randn(2048, 2048, device="cuda")
    for kind, amount in (("sleep", 2_000_000), ("mm", 32)):
        if kind == "sleep" and not hasattr(torch.cuda, "_sleep"):
            continue
        try:
            _spin(kind, amount)          # warm-up: code objects, the BLAS workspace
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            _spin(kind, amount)
            b.record()
            b.synchronize()
            ms = a.elapsed_time(b)
        except RuntimeError:
            continue
        if ms > 0.05:                    # (a _sleep that returns at once cannot be calibrated)
            _RATE.update(kind=kind, per_ms=amount / ms)
            return
    raise RuntimeError("stream_order: neither torch.cuda._sleep nor a matrix-product chain gives a measurable delay")


def delayed(stream, ms=None):
    """Enqueue a device-side delay of about ``ms`` milliseconds on ``stream`` -> an event recorded behind it."""
    _calibrate()
    ms = DELAY_MS if ms is None else ms
    with torch.cuda.stream(stream):
        _spin(_RATE["kind"], math.ceil(ms * _RATE["per_ms"]))
        event = torch.cuda.Event()
        event.record(stream)
    return event


_SIDE = []              # side streams verified to run beside the default stream and beside each other


def _runs_beside(busy, others):
    """Whether a small kernel on each of ``others`` completes while a delay is pending on ``busy``.  A process has a few
    hardware queues (four by default) and its streams share them: two streams on one queue run one after the other, and a
    delay on one of them then hides every ordering mistake between the two."""
    torch.cuda.synchronize()
    event = delayed(busy, 5.0)
    beside = all(_runs_now(other) and not event.query() for other in others)
    torch.cuda.synchronize()
    return beside


def _runs_now(stream):
    """A small kernel on ``stream``, waited for on the host -> True."""
    with torch.cuda.stream(stream):
        torch.zeros(8, device="cuda").add_(1)
        done = torch.cuda.Event()
        done.record(stream)
    done.synchronize()
    return True


def side_streams(n=1):
    """``n`` side streams (one or two) for the whole session, each shown to run beside the default stream and beside the
    other: candidates come from torch's stream pool until enough of them do."""
    tries = 0
    while len(_SIDE) < n:
        tries += 1
        if tries > 16:
            raise Unproven(f"no {'second ' if _SIDE else ''}stream of torch's pool runs beside the default stream"
                           f"{' and the first side stream' if _SIDE else ''}: nothing can be shown about stream order here")
        s = torch.cuda.Stream()
        if s in _SIDE:
            continue
        if _runs_beside(s, [torch.cuda.default_stream(), *_SIDE]) and all(_runs_beside(o, [s]) for o in _SIDE) \
                and _runs_beside(torch.cuda.default_stream(), [s]):
            _SIDE.append(s)
    return _SIDE[:n]


def leaves(tree, path="result"):
    """(path, tensor) of every tensor in a result: a tensor, None, or tuples / lists / dicts of them."""
    if tree is None or isinstance(tree, (bool, int, float, str)):
        return []
    if isinstance(tree, torch.Tensor):
        return [(path, tree)]
    if hasattr(tree, "items"):
        return [p for k, v in tree.items() for p in leaves(v, f"{path}[{k!r}]")]
    return [p for i, v in enumerate(tree) for p in leaves(v, f"{path}[{i}]")]


def clone_tree(tree):
    if isinstance(tree, torch.Tensor):
        return tree.clone()
    if tree is None or isinstance(tree, (bool, int, float, str)):
        return tree
    if hasattr(tree, "items"):
        return {k: clone_tree(v) for k, v in tree.items()}
    return tuple(clone_tree(v) for v in tree)


def mismatches(got, want):
    """The leaves of ``got`` that are not bit for bit those of ``want`` (and structural differences) -> list of strings."""
    a, b = leaves(got), leaves(want)
    if [p for p, _ in a] != [p for p, _ in b]:
        return [f"structure: {[p for p, _ in a]} vs {[p for p, _ in b]}"]
    bad = []
    for (path, x), (_, y) in zip(a, b):
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(f"{path}: {tuple(x.shape)} {x.dtype} vs {tuple(y.shape)} {y.dtype}")
        elif not torch.equal(x, y):
            d = (x.double() - y.double()).abs() if not x.is_complex() else (x - y).abs()
            bad.append(f"{path}: {int((d != 0).sum())} of {d.numel()} values differ (max |diff| {float(d.max()):.3e})")
    return bad


def ordered_call(fn, late_inputs, label="", delay_ms=None, call_stream=None):
    """The consumer-order check.  ``late_inputs``: (late, real) pairs of device tensors; ``fn()`` reads the ``late`` ones.

    On the session's side stream S (`side_streams`): a delay, then ``late.copy_(real)`` for every pair, then ``fn()`` with
    S current.  Before ``fn`` is called a small kernel on the default stream must complete while the delay is pending (the
    two streams run beside each other), and right after ``fn`` returns to the host the delay must still be running -- else
    `Unproven`.  Then everything is synchronised and the result of ``fn`` is returned for the caller to compare
    (`mismatches`).
    ``call_stream``: issue ``fn`` there instead of on S -- the wrong stream, for the negative control."""
    (S,) = side_streams(1)
    delay_ms = DELAY_MS if delay_ms is None else delay_ms
    torch.cuda.synchronize()
    event = delayed(S, delay_ms)
    with torch.cuda.stream(S):
        for late, real in late_inputs:
            late.copy_(real)
    beside = _runs_now(torch.cuda.default_stream()) and not event.query()
    with torch.cuda.stream(S if call_stream is None else call_stream):
        t0 = time.perf_counter()
        got = fn()
        host_ms = (time.perf_counter() - t0) * 1e3
    pending = not event.query()
    torch.cuda.synchronize()
    HOST_MS.append((label, host_ms, delay_ms))
    if not beside:
        raise Unproven(f"{label}: the default stream did not run while the delay was pending on the side stream (they share "
                       f"a hardware queue?) -- a kernel issued on the wrong stream would have waited too")
    if not pending:
        raise Unproven(f"{label}: the {delay_ms:g} ms delay had finished when the call returned to the host after "
                       f"{host_ms:.2f} ms -- the case proves nothing about stream order (a host synchronisation inside "
                       f"the call, or a delay that is too short)")
    return got


def produced_on(fn, stream=None):
    """The producer-order check: ``fn()`` on a side stream without any delay, a clone of its result taken on that stream,
    and the default stream made to wait for an event recorded behind the clone -> the clone, read on the default stream."""
    S = side_streams(1)[0] if stream is None else stream
    torch.cuda.synchronize()
    with torch.cuda.stream(S):
        snap = clone_tree(fn())
        event = torch.cuda.Event()
        event.record(S)
    torch.cuda.current_stream().wait_event(event)
    seen = clone_tree(snap)          # read on the default stream, ordered behind S by the event alone
    torch.cuda.synchronize()
    return seen


def dump_host_times():
    """Write HOST_MS to $GRAFX_STREAM_TIMES (a JSON path), if set: the measurement behind DELAY_MS."""
    path = os.environ.get("GRAFX_STREAM_TIMES")
    if path and HOST_MS:
        import json

        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump([{"case": c, "host_ms": round(h, 3), "delay_ms": d} for c, h, d in HOST_MS], f, indent=1)
