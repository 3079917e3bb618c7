"""What the in-place renders derive once from a render step and keep on it: the gather-sum plan of a routing sum, its
adjoint (transposed and block form), the fused-mix schedule, and the row questions that would otherwise cost a host sync
per render.

Everything is cached through ``_cached`` under one key convention: ``(device.type, device.index)`` where the value holds
device tensors, no device where it holds only row numbers."""
import torch


def _cached(obj, name, key, build, *args):
    """``build(*args)`` once per (obj, name, key); kept in the object's own ``__dict__``.  Every render asks several times
    per stage: a hit costs two dict lookups, and the callers hand over a function and its arguments, not a closure."""
    try:
        return obj.__dict__[name][key]
    except KeyError:
        value = obj.__dict__.setdefault(name, {})[key] = build(*args)
        return value


def _gather_plan(step, device):
    """(src_idx, seg_ptr, n_out, fan) for gfx_gather_sum_f32, None when the step is a plain slice read, False for an
    unsorted scatter (left to the generic path).  Built once per (step, device) from the reference's own descriptors:
    ``source_reads[0]`` says which buffer rows feed the step, ``aggregations[0]`` how they collapse onto its nodes."""
    return _cached(step, "_plan", (device.type, device.index), _build_gather_plan, step, device)


def _build_gather_plan(step, device):
    read, agg = step.source_reads[0], step.aggregations[0]
    if read.method == "slice" and agg.method == "none":
        return None
    if read.method == "slice":
        sources = list(range(read.idx[0], read.idx[1]))
    else:
        sources = read.idx.tolist()
    E = len(sources)
    if agg.method == "none":
        seg = list(range(E + 1))
    elif agg.method == "sum":
        seg = [0, E]
    else:
        slots = agg.idx.tolist()
        if any(b < a for a, b in zip(slots, slots[1:])):
            return False
        n_out = max(slots) + 1
        seg = [0] * (n_out + 1)
        for j in slots:
            seg[j + 1] += 1
        for j in range(n_out):
            seg[j + 1] += seg[j]
    n_out = len(seg) - 1
    fan = None
    uniq = sorted(set(sources))
    if n_out <= 8 and len(uniq) < E:  # some source feeds several destinations: read each source once
        masks = {u: 0 for u in uniq}
        for j in range(n_out):
            for e in range(seg[j], seg[j + 1]):
                masks[sources[e]] |= 1 << j
        fan = (torch.tensor(uniq, dtype=torch.long, device=device),
               torch.tensor([masks[u] for u in uniq], dtype=torch.long, device=device))
    return (torch.tensor(sources, dtype=torch.long, device=device), torch.tensor(seg, dtype=torch.long, device=device),
            n_out, fan)


def _by_src(plan):
    """{source row: the destination slots it feeds, in increasing order} of a gather plan."""
    src, seg = plan[0].tolist(), plan[1].tolist()
    by_src = {}
    for j in range(len(seg) - 1):
        for e in range(seg[j], seg[j + 1]):
            by_src.setdefault(src[e], []).append(j)
    return by_src


def _transposed_plan(step, plan, device):
    """The adjoint of a gather plan: for every distinct source row, the list of destination slots it fed.
    -> (unique source rows (list), dst_idx tensor, seg_ptr tensor, contiguous?, fan) -- fan = (slot indices, per-slot bit
    mask over the unique source rows) when there are at most 32 of them: the adjoint then reads every slot's gradient once
    (gfx_gather_sum_fanout_f32) instead of once per source row."""
    return _cached(step, "_plan_T", (device.type, device.index), _build_transposed_plan, plan, device)


def _build_transposed_plan(plan, device):
    by_src = _by_src(plan)
    uniq = sorted(by_src)
    dst, ptr = [], [0]
    for u in uniq:
        dst.extend(by_src[u])
        ptr.append(len(dst))
    fan = None
    if len(uniq) <= 32:
        masks = {}
        for k, u in enumerate(uniq):
            for j in by_src[u]:
                masks[j] = masks.get(j, 0) | (1 << k)
        slots = sorted(masks)
        fan = (torch.tensor(slots, dtype=torch.long, device=device),
               torch.tensor([masks[j] for j in slots], dtype=torch.long, device=device))
    return (uniq, torch.tensor(dst, dtype=torch.long, device=device), torch.tensor(ptr, dtype=torch.long, device=device),
            uniq == list(range(uniq[0], uniq[0] + len(uniq))), fan)


def _block_fan(step, plan, device):
    """Block structure of a gather plan's adjoint: when the distinct source rows are contiguous and fall into k blocks of m
    >= 2 consecutive rows that feed the SAME destination slots (the eight channel strips of a console bus: their bus and the
    send), the adjoint has only k distinct rows per graph -> (first source row, k, m, slot index tensor, segment pointer
    tensor) for gfx_gather_sum_f32 over the destination gradients; else None.  The largest such m is taken."""
    return _cached(step, "_block_fan", (device.type, device.index), _build_block_fan, plan, device)


def _build_block_fan(plan, device):
    by_src = _by_src(plan)
    uniq = sorted(by_src)
    n = len(uniq)
    if n >= 2 and uniq == list(range(uniq[0], uniq[0] + n)):
        dests = [tuple(by_src[u]) for u in uniq]
        for m in range(n, 1, -1):
            if n % m == 0 and all(dests[i] == dests[i - i % m] for i in range(n)):
                idx, ptr = [], [0]
                for blk in range(n // m):
                    idx.extend(dests[blk * m])
                    ptr.append(len(idx))
                return (uniq[0], n // m, m, torch.tensor(idx, dtype=torch.long, device=device),
                        torch.tensor(ptr, dtype=torch.long, device=device))
    return None


def _mix_schedule(step, nxt, device):
    """When `nxt` is a routing-sum stage that adds up rows of `step` (and possibly finished rows of other stages):
    {"sched", "n_acc", "extras", "n_pre", "extra_rows"} with which a processor that ``accepts_mix`` computes the sums itself
    (ops.mix_schedule: every destination adds its rows in increasing order, as the gather-sum kernels do); else None."""
    return _cached(step, "_mix_sched", (device.type, device.index, id(nxt)), _build_mix_schedule, step, nxt, device)


def _build_mix_schedule(step, nxt, device):
    from .. import ops

    plan = _gather_plan(nxt, device)
    if not plan:
        return None
    d0, d1 = step.dest_write.idx
    e0 = nxt.dest_write.idx[0]
    src, seg = plan[0].tolist(), plan[1].tolist()
    sched = ops.mix_schedule([[v - d0 for v in src[seg[j]:seg[j + 1]]] for j in range(plan[2])], d1 - d0)
    if sched is None:
        return None
    codes, n_acc, pre, post = sched
    extras = [(d0 + r - e0, c) for r, c in pre + post]
    return {"sched": torch.tensor(codes, dtype=torch.long, device=device), "n_acc": n_acc,
            "extras": torch.tensor(extras, dtype=torch.long, device=device) if extras else None,
            "n_pre": len(pre), "extra_rows": [d0 + r for r, _ in pre + post]}


def _indexes_rows(read, a, b):
    rows = read.idx.tolist() if isinstance(read.idx, torch.Tensor) else list(read.idx)
    return any(a <= r < b for r in rows)


def _reads_rows(step, a, b):
    """Does the stage read a buffer row in [a, b)?  Cached on the stage: an index read lives on the device, and asking it
    costs a host sync per render (illegal while the render is captured into a HIP graph)."""
    read = step.source_reads[0]
    if read.method == "slice":
        return read.idx[0] < b and a < read.idx[1]
    return _cached(step, "_reads_rows", (a, b), _indexes_rows, read, a, b)


def _touches_inputs(read, n_src):
    """Does this read access a source row?  Cached on the descriptor, for the same reason as _reads_rows."""
    if read.method == "slice":
        return read.idx[0] < n_src
    return read.method == "index" and _cached(read, "_touches", (n_src,), _indexes_rows, read, 0, n_src)


def _max_row(plan):
    return int(plan[0].max())


def _plan_max_row(step, plan):
    """Highest buffer row a gather plan reads (cached: the plan lives on the device)."""
    return _cached(step, "_plan_max", (), _max_row, plan)


def _gather(ops, buf, plan, out):
    if plan[3] is not None and ops.gather_sum_fanout(buf, plan[3][0], plan[3][1], out):
        return out
    return ops.gather_sum(buf, plan[0], plan[1], out)
