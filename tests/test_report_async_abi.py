"""CPU: the ABI surface of the pipelined report (iris_template_report_async,
iris_pending_report_wait) -- both entry points are exported and named in the header (with the
iris_pending_report_t typedef), the Rust declarations and wrappers, iris_hip.hpp and the Python
mirror; the header comment carries its citations and contract words; the scope paragraphs of the
"combined passes" and "histograms" sections name the pipelined form; and, without a device, the
submission refuses bad value arguments with its message before it looks at a handle, leaving *out
untouched, while the wait refuses a NULL pending and leaves the struct untouched."""
import ctypes
import pathlib
import re

import pytest

import iris_hip as ih
import report_fixtures as rf

ROOT = pathlib.Path(__file__).resolve().parents[1]
NEW = ["iris_template_report_async", "iris_pending_report_wait"]
E_ARG = -1
SENTINEL = 0x5A5A5A5A5A5A


def section(header):
    return header[header.index("- pipelined reports\n"):header.index("int iris_pending_report_wait(")]


def test_symbols_exported_and_named_everywhere():
    lib = ih.load_library()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in ih.exported_symbols(), s
        assert re.search(r"\bint " + s + r"\(", header), s
        assert f"pub fn {s}(" in ffi, s
        assert s + "(" in hpp, s
        assert "ffi::" + s + "(" in engines, s
    assert "typedef iris_pending_t iris_pending_report_t;" in header
    assert "pub type IrisPendingReport = IrisPending;" in ffi
    assert "pub fn report_async(" in engines and "pub struct PendingReport" in engines
    assert "class PendingReport" in hpp and "report_async(" in hpp
    assert hasattr(ih.TemplateEngine, "report_async") and hasattr(ih.PendingReport, "wait")
    assert "PendingReport" in ih.__all__
    # the section stands behind "combined passes"
    assert header.index("- combined passes\n") < header.index("- pipelined reports\n") < header.index("- resolver histograms\n")


def test_header_comment_cites_the_reference_and_states_the_contract():
    sec = section((ROOT / "include" / "iris_hip.h").read_text())
    for cite in ("src/lib.rs:42-53", "src/template.rs:43-47", "src/main.rs:616-621"):
        assert cite in sec, cite
    flat = " ".join(sec.replace(" * ", " ").split())
    for words in ("reads only the in scalars", "does not read the array pointers", "writes nothing to the struct",
                  "leaves *out alone", "blocks for THAT pass only", "byte for byte", "entries past the counts are untouched",
                  "neither read nor written", "nothing is written before every selected part has succeeded",
                  "launches nothing", "owns no event or buffers", "The engine may be destroyed before the wait",
                  "must stay alive and unmodified", "Until its wait a pending holds", "report_shared",
                  "parts = IRIS_REPORT_HIST is the pipelined histogram", "Out of scope", "more than one guest per pass",
                  "k > 64"):
        assert words in flat, words


def test_scope_paragraphs_name_the_pipelined_form():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    combined = header[header.index("- combined passes\n"):header.index("#define IRIS_REPORT_MATCHES")]
    hist = header[header.index("- histograms\n"):header.index("#define IRIS_HIST_MAX_BINS")]
    assert "iris_template_report_async" in combined and "iris_template_report_async" in hist
    assert "neither hosts nor is hosted in the sharing ring" not in combined
    assert "parts = IRIS_REPORT_HIST" in hist and "the pipelined and device-group forms" not in hist


def submit_args(parts=7, k=5, nbins=64, threshold=0.3, cap=4):
    r = rf.guard_report()
    r.parts, r.k, r.nbins, r.threshold, r.matches_cap = parts, k, nbins, threshold, cap
    return r


@pytest.mark.parametrize("change, message", [
    (dict(parts=0), "parts must be one or more of"),
    (dict(parts=8), "parts must be one or more of"),
    (dict(k=0), "k must be 1..IRIS_TOPK_MAX"),
    (dict(k=65), "k must be 1..IRIS_TOPK_MAX"),
    (dict(nbins=0), "nbins must be a power of two"),
    (dict(nbins=3), "nbins must be a power of two"),
    (dict(nbins=2048), "nbins must be a power of two"),
    (dict(threshold=float("nan")), "threshold is NaN"),
])
def test_submission_refuses_value_arguments_before_the_handles(change, message):
    """NULL handles throughout: the value argument's message wins, *out stays as it was and the struct
    is not written.  The pointers of the struct hold guard bytes and are never followed."""
    lib = ih.load_library()
    r = submit_args(**change)
    before = bytes(r)
    out = ctypes.c_void_p(SENTINEL)
    assert lib.iris_template_report_async(None, None, 0, 1, 0, ctypes.byref(r), ctypes.byref(out)) == E_ARG
    assert message in lib.iris_last_error().decode()
    assert out.value == SENTINEL and bytes(r) == before


def test_unselected_parts_scalars_are_not_checked():
    """parts = MATCHES with k = 0 and nbins = 3 passes the value checks: the next refusal is the handles'."""
    lib = ih.load_library()
    r = submit_args(parts=rf.MATCHES, k=0, nbins=3)
    out = ctypes.c_void_p(SENTINEL)
    assert lib.iris_template_report_async(None, None, 0, 1, 0, ctypes.byref(r), ctypes.byref(out)) == E_ARG
    assert "NULL argument" in lib.iris_last_error().decode() and out.value == SENTINEL


def test_submission_refuses_null_report_and_null_out():
    lib = ih.load_library()
    out = ctypes.c_void_p(SENTINEL)
    assert lib.iris_template_report_async(None, None, 0, 1, 0, None, ctypes.byref(out)) == E_ARG
    assert "report is NULL" in lib.iris_last_error().decode() and out.value == SENTINEL
    r = submit_args()
    before = bytes(r)
    assert lib.iris_template_report_async(None, None, 0, 1, 0, ctypes.byref(r), None) == E_ARG
    assert "out is NULL" in lib.iris_last_error().decode() and bytes(r) == before
    # a bad value argument wins over out == NULL
    r = submit_args(k=65)
    assert lib.iris_template_report_async(None, None, 0, 1, 0, ctypes.byref(r), None) == E_ARG
    assert "k must be" in lib.iris_last_error().decode()


def test_wait_refuses_a_null_pending():
    lib = ih.load_library()
    r = submit_args()
    before = bytes(r)
    assert lib.iris_pending_report_wait(None, ctypes.byref(r)) == E_ARG
    assert "pending is NULL" in lib.iris_last_error().decode() and bytes(r) == before
