"""CPU: the pipelined top-k ABI surface (iris_template_topk_async, iris_pending_topk_wait) -- both
entry points are exported and named in the header, the Rust declarations, iris_hip.hpp and the
Python mirror, and each refuses bad arguments with a message before it touches a device.
`out == NULL` at the wait needs a pending, so a device: tests/test_gpu_topk_async.py checks it."""
import ctypes
import pathlib
import re

import iris_hip as ih

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = ["iris_template_topk_async", "iris_pending_topk_wait"]
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
    assert "typedef iris_pending_t iris_pending_topk_t;" in header
    assert "typedef iris_pending_t iris_pending_matches_t;" in header
    assert engines.count("pub fn topk_async(") == 1
    assert hasattr(ih.TemplateEngine, "topk_async") and hasattr(ih.PendingTopk, "wait")
    assert "PendingTopk" in ih.__all__


def test_header_comment_and_scope():
    """The new section names its reference lines and its contract, and the top-k scope paragraph
    names the new call while the rest of the asynchronous pipeline stays out."""
    header = (ROOT / "include" / "iris_hip.h").read_text()
    decl = header.index("int iris_template_topk_async(")
    comment = re.sub(r"\s*\n \* ?", " ", header[header.rindex("/*", 0, decl):decl])  # line breaks of the comment out
    for cite in ("src/lib.rs:42-53", "src/template.rs:43-47", "src/main.rs:616-621"):
        assert cite in comment, cite
    for word in ("byte for byte", "frees the handle", "batch engine is refused", "alive and unmodified",
                 "no host copy of its query", "untouched", "iris_pending_topk_t"):
        assert word in comment, word
    topk = header[header.index("- top-k\n"):header.index("int iris_template_topk(")]
    scope = topk[topk.index("Out of scope"):]
    assert "asynchronous pipeline" in scope and "iris_template_topk_async" in scope


def test_submission_refuses_bad_arguments_without_a_gpu():
    lib = ih.load_library()
    h = ctypes.c_void_p(77)
    f = lib.iris_template_topk_async
    assert f(None, None, 0, 1, 0, 4, ctypes.byref(h)) == E_ARG
    assert "NULL" in _last_error(lib)
    for k in (0, 65):  # the value arguments first: refused whatever the handles
        assert f(None, None, 0, 1, 0, k, ctypes.byref(h)) == E_ARG
        assert "IRIS_TOPK_MAX" in _last_error(lib)
    assert f(None, None, 0, 1, 0, 4, None) == E_ARG
    assert "out is NULL" in _last_error(lib)
    assert h.value == 77


def test_wait_refuses_a_null_pending_without_a_gpu():
    lib = ih.load_library()
    out = (ih.Match * 1)()
    cnt = ctypes.c_uint32(77)
    assert lib.iris_pending_topk_wait(None, out, ctypes.byref(cnt)) == E_ARG
    assert "pending is NULL" in _last_error(lib)
    assert lib.iris_pending_topk_wait(None, None, None) == E_ARG
    assert "pending is NULL" in _last_error(lib)
    assert cnt.value == 77 and out[0].index == 0
