"""The C-ABI library builds, loads and exports exactly what include/grafx_amd.h declares (CPU only:
no compute call is made here)."""
import os
import re
import subprocess

import pytest

from conftest import ROOT


def header_text():
    text = open(os.path.join(ROOT, "include", "grafx_amd.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def header_symbols():
    return sorted(set(re.findall(r"\b(gfx_[a-z0-9_]+)\s*\(", header_text())))


def header_prototypes():
    """name -> (return type, [parameter type, ...]) of every prototype of the header, the types as written without the
    parameter names ("const float*", "gfx_rowmap_t", "int64_t", ...)."""
    protos = {}
    for ret, name, params in re.findall(r"([A-Za-z_][A-Za-z0-9_ ]*?\**)\s*\b(gfx_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", header_text()):
        types = []
        for param in params.split(","):
            param = " ".join(param.split())
            if param != "void":
                types.append(re.sub(r"\s*\b[A-Za-z_][A-Za-z0-9_]*$", "", param).replace(" *", "*"))
        protos[name] = (" ".join(ret.split()).replace(" *", "*"), types)
    return protos


def ctypes_matches(ctype, ctypes_class, RowMap):
    """Whether an entry of _lib.SIGNATURES is how ctypes must pass a C type of the header."""
    import ctypes

    if ctype == "const char*":                       # only as a return type: a static string
        return ctypes_class is ctypes.c_char_p
    if ctype.endswith("*"):                          # any pointer: an address, or a typed ctypes pointer
        return ctypes_class is ctypes.c_void_p or (isinstance(ctypes_class, type) and issubclass(ctypes_class, ctypes._Pointer))
    exact = {"gfx_rowmap_t": RowMap, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "int": ctypes.c_int,
             "float": ctypes.c_float}
    return ctype in exact and ctypes_class is exact[ctype]


def test_ctypes_table_matches_the_header_prototypes_type_by_type():
    """Entries keep their names when their argument lists change, so every row of _lib.SIGNATURES is held to the header's
    prototype: same number of parameters, each passed as the ctypes class of its C type, same return type."""
    from grafx_amd import _lib

    protos = header_prototypes()
    assert sorted(protos) == header_symbols(), "a prototype of the header was not parsed"
    assert sorted(protos) == sorted(_lib.SIGNATURES)
    wrong = []
    for name, (ret, params) in protos.items():
        res, args = _lib.SIGNATURES[name]
        if not ctypes_matches(ret, res, _lib.RowMap):
            wrong.append(f"{name}: returns {ret}, bound as {res.__name__}")
        if len(params) != len(args):
            wrong.append(f"{name}: {len(params)} parameters in the header, {len(args)} in the table")
            continue
        wrong += [f"{name}: parameter {i} is {c}, bound as {a.__name__}" for i, (c, a) in enumerate(zip(params, args))
                  if not ctypes_matches(c, a, _lib.RowMap)]
    assert not wrong, "\n".join(wrong)


def test_library_builds_and_exports_every_header_symbol():
    from grafx_amd import _lib
    from grafx_amd.build import LIB, build

    build()
    handle = _lib.lib()
    declared = header_symbols()
    assert declared, "no symbols parsed from the header"
    for name in declared:
        assert hasattr(handle, name), f"{name} declared in include/grafx_amd.h but not exported"
    assert sorted(_lib.SIGNATURES) == declared, "ctypes signature table and header disagree"
    exported = subprocess.run(["nm", "-D", "--defined-only", LIB], capture_output=True, text=True).stdout
    assert set(re.findall(r"\b(gfx_[a-z0-9_]+)\b", exported)) >= set(declared)


def test_size_queries_need_no_gpu():
    from grafx_amd import _lib

    lib = _lib.lib()
    assert lib.gfx_abi_version() == 2 == _lib.ABI_VERSION
    assert lib.gfx_fftconv_nparts(4001) == 1 and lib.gfx_fftconv_nparts(8193) == 1
    assert lib.gfx_fftconv_nparts(8194) == 2 and lib.gfx_fftconv_nparts(60001) == 8
    assert lib.gfx_fir_spectrum_bytes(3, 4001, 0) == 3 * 17 * 256 * 16
    assert lib.gfx_fftconv_workspace_bytes(2, 2, 131072, 131072, 0, 4001, 0) == 0
    assert lib.gfx_fftconv_workspace_bytes(2, 2, 131072, 131072, 0, 60001, 0) == 2 * 2 * (16 + 7) * 17 * 256 * 16
    assert lib.gfx_iir_fsm_plan_bytes(4001) == (8192 + 4096 + 2 * 2052) * 8 and lib.gfx_iir_fsm_plan_bytes(5000) == 0
    assert lib.gfx_istft_basis_bytes(384) == (388 * 384 + 193 * 2 * 208 + 2 * 384) * 4   # full basis, half basis, FFT factors
    # the reverb's impulse-response workspace.  FFT form (n_fft 384, hop 192, schedule AUTO = 0 or FFT = 2): one energy
    # partial per workgroup of 15 blocks of 192 samples; 2880 / 2881 lie either side of a 15-block seam
    def ceil(a, b):
        return -(-a // b)

    for sched in (0, 2):
        for R in (1, 3):
            for ir_len, wgs in ((193, 1), (2880, 1), (2881, 2), (60000, 21)):
                assert ceil(ceil(ir_len, 192), 15) == wgs
                assert lib.gfx_stft_reverb_workspace_bytes(R, ir_len, 384, 192, 1 + ir_len // 192, sched) == R * wgs * 4
    # matrix-core form (schedule GEMM = 1, or any other transform size): the frames, then a partial per 256 samples
    for R in (1, 3):
        for n_fft, hop, T, sched in ((384, 192, 313, 1), (256, 128, 32, 0)):
            want = (R * 2 * T * n_fft + R * ceil(T * n_fft, 256)) * 4
            assert lib.gfx_stft_reverb_workspace_bytes(R, 60000 if T == 313 else 4000, n_fft, hop, T, sched) == want
    for bad in ((0, 400, 384, 192, 3), (1, 0, 384, 192, 3), (1, 400, 0, 192, 3), (1, 400, 384, 192, 0),
                (-1, 400, 384, 192, 3), (1, -400, 384, 192, 3), (1, 400, -384, 192, 3), (1, 400, 384, 192, -3)):
        assert lib.gfx_stft_reverb_workspace_bytes(*bad, 0) == 0
    # the odd-length aliasing: one row per transform needs (3P - 1) / 2 points (25 tiles at P = 135 071), two rows per
    # transform 2P - 1 per pair (35 tiles); the pair form ends at 2^24 points, even lengths do not alias at all
    P = 131072 + 4000 - 1
    assert lib.gfx_odd_alias_workspace_bytes(2, P) == 2 * 25 * 8192 * 8
    # (+ 256: one word per row, rounded up -- the rows' max |z|, from which the second row of a pair is scaled to the first's binade)
    assert lib.gfx_odd_alias_pair_workspace_bytes(2, P) == 35 * 8192 * 8 + 256 == lib.gfx_odd_alias_pair_workspace_bytes(1, P)
    assert lib.gfx_odd_alias_pair_workspace_bytes(3, P) == 2 * 35 * 8192 * 8 + 256
    assert lib.gfx_odd_alias_pair_workspace_bytes(1024, P) == 512 * 35 * 8192 * 8 + 4096
    assert lib.gfx_odd_alias_pair_plan_bytes(P) == (P + (P - 1) + P + 2 * 35 * 8192) * 8
    assert lib.gfx_odd_alias_pair_precise_plan_bytes(P) == 2 * lib.gfx_odd_alias_pair_plan_bytes(P)
    assert lib.gfx_odd_alias_pair_workspace_bytes(2, 258047) == 63 * 8192 * 8 + 256       # the last length of one column pass
    assert lib.gfx_odd_alias_pair_workspace_bytes(2, 258049) == 4 * 16 * 8192 * 8 + 256   # then one outer radix-4 level
    assert lib.gfx_odd_alias_pair_workspace_bytes(2, 480000 + 4000 - 1) == 4 * 30 * 8192 * 8 + 256   # BASELINE configs[1], 4000 taps
    assert lib.gfx_odd_alias_pair_plan_bytes(8388607) > 0 and lib.gfx_odd_alias_pair_plan_bytes(8388609) == 0
    assert lib.gfx_odd_alias_pair_plan_bytes(4000) == 0 and lib.gfx_odd_alias_plan_bytes(8388609) > 0


CZT_ONE_ROW_TILES = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 14, 15, 16, 18, 20, 21, 24, 25, 27, 28, 30, 32)
CZT_PAIR_TILES = CZT_ONE_ROW_TILES + (35, 36, 40, 42, 45, 48, 49, 50, 54, 56, 60, 63)
CZT_SIZE_ROWS = (1, 2, 3, 1024)
CZT_SIZE_ENTRIES = [f"gfx_odd_alias{pair}{precise}_{what}_bytes" for pair in ("", "_pair") for precise in ("", "_precise")
                    for what in ("plan", "workspace")]


def czt_size_lengths():
    """For every supported tile count of each form the largest odd P that fits it and the next odd one (32 and 63 tiles: the
    last lengths before an outer radix-4 level), and the ends of the range: the smallest length, an even one, the last
    lengths of the pair form (2P - 1 <= 2^24) and of the one-row form ((3P - 1) / 2 <= 2^24) and the first beyond each."""
    lengths = {3, 4000, 8388607, 8388609, 11184811, 11184813}
    for C in CZT_ONE_ROW_TILES:              # P + (P + 1) / 2 - 1 <= 8192 C
        P = (2 * 8192 * C + 1) // 3
        P -= 1 - P % 2
        assert P + (P + 1) // 2 - 1 <= 8192 * C < P + 2 + (P + 3) // 2 - 1
        lengths |= {P, P + 2}
    for C in CZT_PAIR_TILES:                 # 2 P - 1 <= 8192 C
        P = (8192 * C + 1) // 2
        P -= 1 - P % 2
        assert 2 * P - 1 <= 8192 * C < 2 * (P + 2) - 1
        lengths |= {P, P + 2}
    return sorted(lengths)


def czt_size_table(lib):
    return {name: [[getattr(lib, name)(P)] if name.endswith("plan_bytes") else [getattr(lib, name)(rows, P) for rows in CZT_SIZE_ROWS]
                   for P in czt_size_lengths()] for name in CZT_SIZE_ENTRIES}


def test_chirp_z_sizes_are_the_recorded_ones():
    """The eight size entries of the odd-length aliasing over every supported tile count of both forms, either side of
    every boundary of the geometry, against the table recorded before the two forms' geometries were folded into one
    function (tests/golden/czt_sizes.json: per entry and length, the plan's bytes or the workspace's for 1, 2, 3, 1024 rows)."""
    import json

    from grafx_amd import _lib

    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "czt_sizes.json")))
    assert golden["lengths"] == czt_size_lengths() and golden["rows"] == list(CZT_SIZE_ROWS)
    assert sorted(golden["bytes"]) == sorted(CZT_SIZE_ENTRIES)
    table = czt_size_table(_lib.lib())
    wrong = [(name, P, got, want) for name in CZT_SIZE_ENTRIES
             for P, got, want in zip(golden["lengths"], table[name], golden["bytes"][name]) if got != want]
    assert not wrong, wrong[:10]
    # the table is not all zeros where a plan exists: both forms accept 3 and refuse an even length
    i3, i4000 = golden["lengths"].index(3), golden["lengths"].index(4000)
    for name in CZT_SIZE_ENTRIES:
        assert all(v > 0 for v in golden["bytes"][name][i3]) and not any(golden["bytes"][name][i4000])


def test_processors_refuse_cpu_tensors_and_missing_library(monkeypatch):
    import torch

    import grafx_amd.processors as P

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        P.StereoGain()(torch.zeros(1, 2, 8), torch.zeros(1, 2))
    from grafx_amd import _lib

    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB", "/nonexistent/libgrafx_amd.so")
    with pytest.raises(ImportError, match="not built"):
        _lib.lib()


def test_library_of_another_abi_version_is_refused(monkeypatch):
    """Entries keep their names across ABI versions, so a library built from another version of the sources must not load."""
    from grafx_amd import _lib

    _lib.lib()                                   # (built, and of this version)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "ABI_VERSION", _lib.ABI_VERSION + 1)
    with pytest.raises(ImportError, match="ABI version 2.*not built"):
        _lib.lib()
    assert _lib._lib is None


def test_plain_c_program_links_and_runs_against_the_library(tmp_path):
    """The boundary is a C ABI: a C translation unit must be able to include the header and link the library."""
    import os
    import subprocess

    from grafx_amd import build

    lib = build.build()
    exe = tmp_path / "abi_smoke"
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    libdir = os.path.dirname(lib)
    cmd = ["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), os.path.join(root, "tests", "c", "abi_smoke.c"),
           "-L", libdir, "-lgrafx_amd", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", str(exe)]
    subprocess.run(cmd, check=True, capture_output=True, text=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True)
    assert "abi_smoke ok" in out.stdout


def test_small_composite_dfts_on_the_host(tmp_path):
    """csrc/small_dft.hpp (the in-register DFTs of 3, 5, 6, 7, 9, ... 30 points behind the chirp-z column passes) is
    __host__ __device__: tests/c/small_dft_host.hip runs every supported size, forward and inverse, float and double,
    against a direct sum in double -- on the CPU, no GPU needed."""
    import os
    import subprocess

    from grafx_amd import build

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = tmp_path / "small_dft_host"
    cmd = [build.HIPCC, "--offload-arch=gfx950", "-std=c++17", "-O1", os.path.join(root, "tests", "c", "small_dft_host.hip"),
           "-o", str(exe)]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "SMALL_DFT_OK" in out.stdout, out.stdout + out.stderr
