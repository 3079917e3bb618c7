"""_plumbing._overlap and _plumbing._self_overlap against brute force: the set of storage offsets a view touches, over
seeded random pairs of views of one small storage (at most 512 floats).  The two predicates guard every tensor an entry
writes (the kernels take their pointers ``__restrict__``), so what they may never do is answer False for views that share
an element; on the views the render makes -- ranges of one (B, V, C, L) buffer -- they may not answer True for disjoint
ones either, or the render's own calls would be refused.  No GPU: shapes and strides only."""
import itertools
import random

import pytest
import torch

from grafx_amd._plumbing import _overlap, _self_overlap

PAIRS = 2000
STORAGE = 512


def _offsets(t):
    """Every storage offset the view touches, one entry per index (a repeated offset: the view overlaps itself)."""
    return [t.storage_offset() + sum(i * st for i, st in zip(idx, t.stride()))
            for idx in itertools.product(*(range(n) for n in t.shape))]


def _truth(a, b):
    """(the views share an element, a overlaps itself, b overlaps itself) by brute force."""
    oa, ob = _offsets(a), _offsets(b)
    same = a.untyped_storage().data_ptr() == b.untyped_storage().data_ptr()
    return same and not set(oa).isdisjoint(ob), len(set(oa)) < len(oa), len(set(ob)) < len(ob)


def _span(rng, n, whole=0.0):
    """A non-empty range lo:hi of a dimension of n elements (``whole``: how often all of it)."""
    if rng.random() < whole:
        return 0, n
    lo = rng.randrange(n)
    return lo, rng.randint(lo + 1, n)


def _render_view(rng, buf, like=None):
    """A view the render makes of its (B, V, C, L) buffer: a node range, and/or a range of the samples, and/or one channel.
    ``like``: (node count, sample count, channel) of the other view of the pair, to draw equal extents."""
    _, V, C, L = buf.shape
    if like is not None and rng.random() < 0.4:
        nv, nl, ch = like
        v0, l0 = rng.randrange(V - nv + 1), rng.randrange(L - nl + 1)
    else:
        (v0, v1), (l0, l1) = _span(rng, V), _span(rng, L, whole=0.5)
        nv, nl, ch = v1 - v0, l1 - l0, rng.randrange(C) if rng.random() < 0.3 else None
    t = buf[:, v0:v0 + nv, :, l0:l0 + nl]
    return (t if ch is None else t[:, :, ch]), (nv, nl, ch)


def _family_render(rng):
    buf = torch.zeros(rng.randint(2, 3), rng.randint(3, 6), rng.randint(1, 2), rng.randint(4, 9))
    a, like = _render_view(rng, buf)
    b, _ = _render_view(rng, buf, like)
    return a, b


def _permuted_view(rng, base):
    t = base
    for d in range(t.ndim):
        lo, hi = _span(rng, t.shape[d], whole=0.3)
        t = t.narrow(d, lo, hi - lo)
    t = t.permute(*rng.sample(range(t.ndim), t.ndim))
    if rng.random() < 0.5:         # a dimension repeated without memory of its own
        d = rng.randrange(t.ndim + 1)
        t = t.unsqueeze(d).expand(*t.shape[:d], rng.randint(2, 3), *t.shape[d:])
    return t


def _family_permuted(rng):
    base = torch.zeros(*(rng.randint(2, 6) for _ in range(rng.randint(1, 3))))
    return _permuted_view(rng, base), _permuted_view(rng, base)


def _family_strided(rng):
    """as_strided views of any strides, nested or not; for every other pair the second view is the first one moved."""
    store, views = torch.zeros(STORAGE), []
    for _ in range(2):
        if not views or rng.random() < 0.5:
            shape = [rng.randint(1, 4) for _ in range(rng.randint(1, 3))]
            stride = [rng.randint(1, 7) for _ in shape]
        views.append(store.as_strided(shape, stride, rng.randrange(24)))
    return views


def _family_two_storages(rng):
    family = rng.choice([_family_render, _family_permuted, _family_strided])
    a, b = family(rng)
    return a, torch.zeros(b.untyped_storage().nbytes() // 4).as_strided(b.shape, b.stride(), b.storage_offset())


FAMILIES = {"render": _family_render, "permuted": _family_permuted, "strided": _family_strided,
            "two_storages": _family_two_storages}


@pytest.mark.parametrize("family", FAMILIES)
def test_overlap_predicates_against_brute_force(family):
    rng = random.Random(sum(map(ord, family)))
    shared = 0
    for k in range(PAIRS):
        a, b = FAMILIES[family](rng)
        assert a.untyped_storage().nbytes() <= 4 * STORAGE and b.untyped_storage().nbytes() <= 4 * STORAGE
        what = f"{family} pair {k}: {tuple(a.shape)} {a.stride()} +{a.storage_offset()} / " \
               f"{tuple(b.shape)} {b.stride()} +{b.storage_offset()}"
        truth, a_self, b_self = _truth(a, b)
        shared += truth
        got = _overlap(a, b)
        assert got == _overlap(b, a), what
        assert got or not truth, "shared element missed, " + what
        assert (_self_overlap(a) or not a_self) and (_self_overlap(b) or not b_self), "self-overlap missed, " + what
        if family == "render":        # exact on what the render makes: a false refusal would break its own calls
            assert got == truth, "disjoint views refused, " + what
            assert not a_self and not b_self and not _self_overlap(a) and not _self_overlap(b), what
        if family == "two_storages":
            assert not truth and not got, what
    if family in ("render", "strided"):  # the draw itself: neither answer can pass by being the usual one
        assert 0.25 * PAIRS <= shared <= 0.75 * PAIRS, f"{family}: {shared} of {PAIRS} pairs share an element"


def test_interleaved_rows_that_the_quotient_search_missed():
    """Strides (5, 3) are not nested (5 < 3 * 3): offset 10 is 2 * 5 + 0 * 3 of the first view and 1 + 0 * 5 + 3 * 3 of the
    second.  Trying the two quotients of the offset difference per dimension does not find it."""
    s = torch.zeros(32)
    a, b = s.as_strided((3, 4), (5, 3), 0), s.as_strided((3, 4), (5, 3), 1)
    assert 10 in _offsets(a) and 10 in _offsets(b)
    assert _overlap(a, b) and _overlap(b, a)


def test_unequal_extents_of_one_buffer_are_told_apart():
    buf = torch.zeros(2, 10, 2, 64)
    assert not _overlap(buf[:, 2:5], buf[:, 5:6]) and _overlap(buf[:, 2:5], buf[:, 4:5])
    assert not _overlap(buf[:, 2:5, :, :32], buf[:, 2:4, :, 32:]) and _overlap(buf[:, 2:5, :, :33], buf[:, 2:4, :, 32:])
    assert not _overlap(buf[:, 2:5, 0], buf[:, 2:5, 1]) and _overlap(buf[:, 2:5, 1], buf[:, 4:6])
    row = buf[:1, :1]
    assert _self_overlap(row.expand(2, 3, 2, 64)) and not _self_overlap(buf[:, 2:5]) and not _self_overlap(buf.permute(1, 0, 3, 2))
    assert not _self_overlap(buf[:, :0]) and not _overlap(buf[:, :0], buf)

    class Reversed:
        """What a view with a negative last stride would look like (torch.flip copies, as_strided refuses one): the rows of
        ``t``, last sample first."""

        def __init__(self, t):
            self.t, self.shape = t, t.shape

        def stride(self):
            return (*self.t.stride()[:-1], -self.t.stride(-1))

        def data_ptr(self):
            return self.t.data_ptr() + 4 * (self.t.shape[-1] - 1) * self.t.stride(-1)

        def __getattr__(self, name):          # numel, element_size
            return getattr(self.t, name)

    back = Reversed(buf[:, 2:5, :, 32:])
    assert _overlap(back, buf[:, 2:5, :, 32:]) and _overlap(buf[:, 4:6, :, 63:], back) and not _overlap(back, buf[:, 2:5, :, :32])
    assert not _self_overlap(back) and not _overlap(back, buf[:, 5:7])
    flat = buf.view(-1)               # elements of another width: bounding ranges, in bytes
    assert _overlap(flat.view(torch.uint8)[:4], flat[:1]) and not _overlap(flat.view(torch.uint8)[4:8], flat[:1])
