"""The public surface of grafx_amd.ops is what tests/golden/ops_surface.json recorded before the wrappers' shared checks
were folded -- at the commit before the first fold, and again, for the functions added since, at the commit before the
pairs of newer wrappers got one body each: every public function and class keeps its parameter names, order and
defaults, and the module-level switches keep their defaults.  No GPU and no built library: signatures only.

The fixture was written by ``describe(ops)`` run on a checkout of those commits, not on the tree under test.  ``rowmap``
and ``profiling`` are the first recording's: they live in _plumbing since, where ``describe`` does not look, and stay
pinned here."""
import inspect
import json
import os

import pytest

from grafx_amd import ops

with open(os.path.join(os.path.dirname(__file__), "golden", "ops_surface.json")) as f:
    SURFACE = json.load(f)

# the switches tests assign as ``ops.X = ...``; the two with an environment variable read it once, at import
SWITCHES = {"MIX_FUSION": None, "ALIAS_PAIRS": "GRAFX_ALIAS_PAIRS", "DYN_LOOKBACK": None, "DYN_SCHEDULE": None,
            "FFTCONV_SCHEDULE": None, "ROWMAX_BYPRODUCT": None, "DYN_BWD_RESCAN": None, "BALLISTICS_SCHEDULE": None,
            "ALIAS_ROWS_PER_CHUNK": "GRAFX_ALIAS_ROWS"}


def parameters(obj):
    """[[name, kind, repr(default) or None for a required parameter], ...]; None where Python gives no signature."""
    try:
        sig = inspect.signature(obj)
    except (TypeError, ValueError):
        return None
    return [[p.name, p.kind.name, None if p.default is p.empty else repr(p.default)] for p in sig.parameters.values()]


def describe(mod):
    """What the fixture holds: the module's own public functions and classes with their parameters, the switches'
    values, and the names of everything else public (constants, tables)."""
    own = {k: v for k, v in vars(mod).items() if not k.startswith("_") and not inspect.ismodule(v)}
    callables = {k: v for k, v in own.items()
                 if (inspect.isfunction(v) or inspect.isclass(v)) and v.__module__ == mod.__name__}
    return {"functions": {k: parameters(v) for k, v in sorted(callables.items()) if inspect.isfunction(v)},
            "classes": {k: parameters(v) for k, v in sorted(callables.items()) if inspect.isclass(v)},
            "switches": {k: getattr(mod, k) for k in SWITCHES},
            "names": sorted(k for k, v in own.items() if k not in callables and k not in SWITCHES and not callable(v))}


def test_fixture_is_the_recorded_surface():
    assert len(SURFACE["functions"]) == 73
    assert set(SURFACE["classes"]) == {"profiling", "FftLibraryWarning"}
    assert set(SURFACE["switches"]) == set(SWITCHES)


@pytest.mark.parametrize("name", sorted(SURFACE["functions"]))
def test_function_keeps_its_signature(name):
    fn = getattr(ops, name, None)
    assert inspect.isfunction(fn), f"ops.{name} is gone"
    assert parameters(fn) == SURFACE["functions"][name]


@pytest.mark.parametrize("name", sorted(SURFACE["classes"]))
def test_class_keeps_its_signature(name):
    cls = getattr(ops, name, None)
    assert inspect.isclass(cls), f"ops.{name} is gone"
    assert parameters(cls) == SURFACE["classes"][name]


@pytest.mark.parametrize("name", sorted(SWITCHES))
def test_switch_keeps_its_default(name):
    assert hasattr(ops, name)
    if SWITCHES[name] is None or SWITCHES[name] not in os.environ:
        assert getattr(ops, name) == SURFACE["switches"][name]
    assert type(getattr(ops, name)) is type(SURFACE["switches"][name])


def test_constants_and_private_names_stay_reachable():
    missing = [k for k in SURFACE["names"] if not hasattr(ops, k)]
    assert not missing, missing
    for k in ("profiling", "rowmap", "_overlap", "_alias_plan", "_alias_pairs", "_ALIAS_PLANS"):
        assert hasattr(ops, k), k
