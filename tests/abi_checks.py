"""The frame the per-op ABI tests (tests/test_*_abi.py) share, for a machine without a GPU: C entries held to the header and
to the ctypes table, a stand-in for a device pointer, and a table of refusals run against an entry.  The prototype lists
and the tables of cases are the content, and stay in their files."""
import torch
from test_abi import ctypes_matches, header_prototypes


def entries_match(entries, want=None):
    """Every name of ``entries`` is declared in the header, bound in _lib.SIGNATURES and exported by the library, and the
    header's prototype agrees with the ctypes signature type by type -- and with ``want[name]`` = (return type, [argument
    types]) as the header spells them, where the file lists them.  The library and the bindings are at ABI version 2."""
    from grafx_amd import _lib

    protos = header_prototypes()
    for name in entries:
        assert name in protos and name in _lib.SIGNATURES and hasattr(_lib.lib(), name), name
        if want is not None:
            assert protos[name] == want[name], name
        ret, params = protos[name]
        res, args = _lib.SIGNATURES[name]
        assert ctypes_matches(ret, res, _lib.RowMap) and len(params) == len(args), name
        assert all(ctypes_matches(c, a, _lib.RowMap) for c, a in zip(params, args)), name
    assert _lib.lib().gfx_abi_version() == 2 == _lib.ABI_VERSION


def device_pointer():
    """-> (p, what keeps it alive): a pointer for the refusals, which come back before any launch, so that it is never
    followed.  Without a GPU it stands for any non-null, 16-byte aligned device pointer.  Where a GPU is visible it is a
    real 16 MB device buffer instead, larger than anything the refusal tests' shapes index: should a check ever slip behind
    a launch there, the test fails on the return code and no kernel has been sent to an address nobody owns."""
    if torch.cuda.is_available():
        held = torch.zeros(1 << 22, dtype=torch.float32, device="cuda")
        return held.data_ptr(), held
    return 0x100000, None


def refused(entry, base, cases, code=-1):
    """``entry`` answers ``code`` (-1: GFX_EINVAL, -2: GFX_ENOSPC) for the arguments ``base`` with each change of ``cases`` =
    {name: {argument: value}} in turn; the failing case's name is the assertion's message."""
    for what, change in cases.items():
        assert entry(*{**base, **change}.values()) == code, what
