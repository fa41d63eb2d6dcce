"""CPU: the pipelined threshold-match ABI surface (iris_template_matches_async,
iris_pending_matches_wait) -- both entry points are exported and named in the header, the Rust
declarations, iris_hip.hpp and the Python mirror, and each refuses bad arguments with a message
before it touches a device.  `out == NULL` with `cap > 0` at the wait needs a pending, so a device:
tests/test_gpu_matches_async.py checks it."""
import ctypes
import math
import pathlib
import re

import iris_hip as ih

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = ["iris_template_matches_async", "iris_pending_matches_wait"]
E_ARG = -1


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def test_symbols_exported_and_named_everywhere():
    lib = ih.load_library()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in ih.exported_symbols(), s
        assert re.search(r"\bint " + s + r"\(", header), s
        assert f"pub fn {s}(" in ffi, s
        assert s + "(" in hpp, s
        assert "ffi::" + s + "(" in engines, s
    assert "typedef iris_pending_t iris_pending_matches_t;" in header
    assert engines.count("pub fn matches_async(") == 1
    assert hasattr(ih.TemplateEngine, "matches_async") and hasattr(ih.PendingMatches, "wait")


def test_header_scope_lists():
    """Threshold matching no longer lists the whole asynchronous pipeline as out of scope, top-k
    still does, and the new section names its reference lines and its contract."""
    header = (ROOT / "include" / "iris_hip.h").read_text()
    decl = header.index("int iris_template_matches_async(")
    comment = header[header.rindex("/*", 0, decl):decl]
    assert "src/lib.rs:42-53" in comment and "src/template.rs:43-47" in comment
    for word in ("byte for byte", "frees the handle", "batch engine is refused", "alive and unmodified"):
        assert word in comment, word
    sec = header[header.index("threshold matching"):header.index("int iris_template_matches(")]
    assert "iris_template_matches_async" in sec
    topk = header[header.index("- top-k"):header.index("int iris_template_topk(")]
    assert "the asynchronous pipeline" in topk


def test_submission_refuses_bad_arguments_without_a_gpu():
    lib = ih.load_library()
    h = ctypes.c_void_p(77)
    f = lib.iris_template_matches_async
    assert f(None, None, 0, 1, 0, 0.5, 1, ctypes.byref(h)) == E_ARG
    assert "NULL" in _last_error(lib)
    for nan in (math.nan, -math.nan):
        assert f(None, None, 0, 1, 0, nan, 1, ctypes.byref(h)) == E_ARG
        assert "NaN" in _last_error(lib)
    assert f(None, None, 0, 1, 0, 0.5, 1, None) == E_ARG
    assert "out is NULL" in _last_error(lib)
    assert h.value == 77


def test_wait_refuses_a_null_pending_without_a_gpu():
    lib = ih.load_library()
    out = (ih.Match * 1)()
    cnt = ctypes.c_uint64(77)
    assert lib.iris_pending_matches_wait(None, out, ctypes.byref(cnt)) == E_ARG
    assert "pending is NULL" in _last_error(lib)
    assert lib.iris_pending_matches_wait(None, None, None) == E_ARG
    assert "pending is NULL" in _last_error(lib)
    assert cnt.value == 77 and out[0].index == 0
