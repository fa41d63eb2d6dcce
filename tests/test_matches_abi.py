"""CPU: the threshold-match ABI surface (iris_template_matches, iris_resolver_matches,
iris_resolver_matches_masks) -- the three entry points are exported and named in the header, the Rust
declarations, iris_hip.hpp and the Python mirror; each refuses bad arguments with a message before
it touches a device; and a C++ program using the iris_hip.hpp forms compiles and links
(tests/test_gpu_matches.py runs it)."""
import ctypes
import math
import pathlib
import re
import subprocess

import numpy as np

import iris_hip as ih

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "matches.cpp"
NEW = ["iris_template_matches", "iris_resolver_matches", "iris_resolver_matches_masks"]
E_ARG = -1


def build_cpp_program(outdir):
    """Compiles tests/cpp/matches.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "matches"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def _calls(lib):
    """name -> f(threshold, out, cap, count, parts): the entry point with NULL handles and otherwise
    plausible arguments (one record, one 31-element share array)."""
    rows = np.zeros(31, np.uint16)
    ptrs = (ctypes.c_void_p * 1)(rows.ctypes.data)
    den = rows.ctypes.data_as(ctypes.c_void_p)
    return {
        "iris_template_matches": lambda t, out, cap, cnt, parts=1: lib.iris_template_matches(
            None, None, 0, 1, 0, t, out, cap, cnt),
        "iris_resolver_matches": lambda t, out, cap, cnt, parts=1: lib.iris_resolver_matches(
            None, ptrs, parts, den, 1, 0, t, out, cap, cnt),
        "iris_resolver_matches_masks": lambda t, out, cap, cnt, parts=1: lib.iris_resolver_matches_masks(
            None, None, 0, 1, ptrs, parts, 0, t, out, cap, cnt),
    }, (rows, ptrs)


def test_symbols_exported_and_named_everywhere():
    lib = ih.load_library()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in ih.exported_symbols(), s
        assert re.search(r"\bint " + s + r"\(", header), s
        assert f"pub fn {s}(" in ffi, s
        assert s + "(" in hpp, s
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    assert engines.count("pub fn matches(") == 2
    assert hasattr(ih.TemplateEngine, "matches") and hasattr(ih.MasksEngine, "matches") and hasattr(ih, "resolver_matches")


def test_header_comments_cite_the_reference_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    sec = header[header.index("threshold matching"):header.index("int iris_resolver_matches_masks(")]
    assert "src/main.rs:616-621" in sec and "src/template.rs:43-47" in sec
    assert "no reference counterpart" in sec
    for word in ("batch engines", "host-array forms", "asynchronous pipeline", "device groups"):
        assert word in sec, word
    for s in NEW:  # every entry point's own comment names a reference line
        decl = header.index("int " + s + "(")
        comment = header[header.rindex("/*", 0, decl):decl]
        assert re.search(r"src/(main|template)\.rs:\d+", comment), s


def test_null_handles_are_refused_without_a_gpu():
    lib = ih.load_library()
    calls, _keep = _calls(lib)
    out = (ih.Match * 1)()
    cnt = ctypes.c_uint64(77)
    for name, f in calls.items():
        assert f(0.5, out, 1, ctypes.byref(cnt)) == E_ARG, name
        assert "NULL" in _last_error(lib), name
    assert cnt.value == 77 and out[0].index == 0


def test_value_arguments_are_refused_without_a_gpu():
    lib = ih.load_library()
    calls, _keep = _calls(lib)
    out = (ih.Match * 1)()
    cnt = ctypes.c_uint64(77)
    for name, f in calls.items():
        for nan in (math.nan, -math.nan):
            assert f(nan, out, 1, ctypes.byref(cnt)) == E_ARG, name
            assert "NaN" in _last_error(lib), name
        assert f(0.5, out, 1, None) == E_ARG, name
        assert "count" in _last_error(lib), name
        assert f(0.5, None, 1, ctypes.byref(cnt)) == E_ARG, name
        assert "out is NULL" in _last_error(lib), name
    for name in ("iris_resolver_matches", "iris_resolver_matches_masks"):
        for parts in (0, 9, 2**31):
            assert calls[name](0.5, out, 1, ctypes.byref(cnt), parts) == E_ARG, (name, parts)
            assert "parts" in _last_error(lib), (name, parts)
    assert cnt.value == 77


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()
