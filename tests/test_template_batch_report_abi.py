"""CPU: the ABI surface of the template batch report (iris_template_batch_report) -- the entry point
is exported and named in the header, the Rust declarations, iris_hip.hpp and the Python mirror, the
ctypes struct and the Rust struct have the layout a C++ compiler gives the header's struct, the
header section states the contract and the scope, and bad value arguments are refused with a message
before a handle is touched, leaving the struct and every array at their guard bytes."""
import ctypes
import pathlib
import re
import subprocess

import pytest

import batch_report_fixtures as bf
import iris_hip as ih
from batch_report_fixtures import ALL, FIELDS, HIST, MATCHES, NAME, TOPK

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "template_batch_report.cpp"
E_ARG = -1

LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "iris_hip.h"
int main() {
    std::printf("sizeof %zu\n", sizeof(iris_batch_report_t));
#define F(f) std::printf(#f " %zu %zu\n", offsetof(iris_batch_report_t, f), sizeof(((iris_batch_report_t *)0)->f))
    F(parts); F(k); F(nbins); F(reserved); F(threshold); F(matches); F(matches_cap); F(matches_counts); F(topk);
    F(topk_counts); F(bins); F(invalid);
    return 0;
}
"""


def build_cpp_program(outdir):
    """Compiles tests/cpp/template_batch_report.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "template_batch_report"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def test_symbol_exported_and_named_everywhere():
    lib = ih.load_library()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    assert hasattr(lib, NAME) and NAME in ih.exported_symbols()
    assert f"ffi::{NAME}(" in engines and NAME + "(" in hpp and "iris_batch_report_t" in hpp
    assert "#[repr(C)]\n#[derive(Clone, Copy, Debug)]\npub struct IrisBatchReport" in ffi
    assert callable(ih.TemplateBatchEngine.report) and "BatchReport" in ih.__all__
    # the Rust struct and the Python mirror list the header's fields in the header's order
    rust = re.search(r"pub struct IrisBatchReport \{(.*?)\}", ffi, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == FIELDS
    assert [f for f, _ in ih.BatchReport._fields_] == FIELDS
    c_struct = re.search(r"typedef struct iris_batch_report \{(.*?)\} iris_batch_report_t;", header, flags=re.S).group(1)
    assert re.findall(r"(\w+);", c_struct) == FIELDS


def test_rust_declares_the_headers_signature():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    c = re.search(r"\bint " + NAME + r"\((.*?)\);", header, flags=re.S).group(1)
    c = re.sub(r"/\*.*?\*/", "", c)
    c_params = [" ".join(p.split()) for p in c.split(",")]
    assert c_params == ["iris_engine_t *engine", "const iris_db_t *db", "uint64_t first", "uint64_t n", "uint64_t index_base",
                        "void *report"]
    rust = re.search(r"pub fn " + NAME + r"\((.*?)\) -> c_int;", ffi, flags=re.S).group(1)
    rust_params = [" ".join(p.split()) for p in rust.split(",") if p.strip()]
    assert rust_params == ["engine: *mut IrisEngine", "db: *const IrisDb", "first: u64", "n: u64", "index_base: u64",
                           "report: *mut c_void"]


def test_header_states_the_contract_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    assert header.index("- resolver reports\n") < header.index("- template batch reports\n") < header.index("- arch plugin\n")
    sec = header[header.index("- template batch reports\n"):header.index("- arch plugin\n")]
    for word in ("BYTE FOR BYTE", "Out of scope", "neither read nor written", "writes nothing", "nothing is launched",
                 "waits once", "iris_template_batch_matches", "iris_template_batch_topk", "iris_template_batch_histogram",
                 "stay untouched", "reserved", "TILES", "masks batch engine", "pipelined", "host-array", "device-group",
                 "per-query thresholds", "search part", "void *"):
        assert word in sec, word
    # the sections of the single-probe reports point here
    combined = header[header.index("- combined passes\n"):header.index("int iris_template_report(")]
    resolver = header[header.index("- resolver reports\n"):header.index("int iris_resolver_report(")]
    assert NAME in combined and NAME in resolver


def test_struct_layout_equals_the_compilers(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(ih.BatchReport)}"
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in lines[1:1 + len(FIELDS)]}
    want = {f: (getattr(ih.BatchReport, f).offset, getattr(ih.BatchReport, f).size) for f in FIELDS}
    assert got == want
    # no implicit padding: the fields tile the struct
    end = 0
    for f in FIELDS:
        assert want[f][0] == end, f
        end += want[f][1]
    assert end == ctypes.sizeof(ih.BatchReport) == 80


def refused(parts, message, **kw):
    """A call with NULL handles that must be refused for its value arguments: IRIS_E_ARG with
    `message`, the struct and the arrays untouched (raw_report checks both)."""
    args = dict(threshold=0.4, cap=4, k=5, nbins=64)
    args.update(kw)
    res = bf.raw_report(None, None, 0, 1, parts, nq=5, expect_rc=E_ARG, **args)
    assert message in res.error, (res.error, message)


def test_bad_parts_and_reserved_are_refused_whatever_the_handles():
    lib = ih.load_library()
    for parts in (0, 8, 15, 1 << 31):
        r = bf.guard_report()
        r.parts = parts
        before = bytes(r)
        assert lib.iris_template_batch_report(None, None, 0, 1, 0, ctypes.byref(r)) == E_ARG, parts
        assert "parts must be one or more" in lib.iris_last_error().decode() and bytes(r) == before
    assert lib.iris_template_batch_report(None, None, 0, 1, 0, None) == E_ARG
    assert "report is NULL" in lib.iris_last_error().decode()
    for parts in bf.MULTI + [MATCHES, TOPK, HIST]:
        refused(parts, "reserved must be 0", reserved=1)
    # parts is looked at first
    r = bf.guard_report()
    r.parts = 0
    assert lib.iris_template_batch_report(None, None, 0, 1, 0, ctypes.byref(r)) == E_ARG
    assert "parts" in lib.iris_last_error().decode()


def test_each_parts_arguments_fall_under_its_siblings_rules():
    for parts in (MATCHES, MATCHES | TOPK, ALL):
        refused(parts, "threshold is NaN", threshold=float("nan"))
    for parts in (TOPK, TOPK | HIST, ALL):
        for k in (0, 65):
            refused(parts, "IRIS_TOPK_MAX", k=k)
    for parts in (HIST, MATCHES | HIST, ALL):
        for nbins in (0, 3, 48, 2048):
            refused(parts, "IRIS_HIST_MAX_BINS", nbins=nbins)


def test_null_pointers_of_selected_parts_are_refused():
    for field, message in (("matches", "out is NULL with cap > 0"), ("matches_counts", "count is NULL"),
                           ("topk", "out is NULL"), ("topk_counts", "count is NULL"), ("bins", "bins is NULL"),
                           ("invalid", "invalid is NULL")):
        refused(ALL, message, null=(field,))
    # matches may be NULL when the cap is 0; with every value argument in order the call fails for its handles
    refused(ALL, "NULL", cap=0)
    refused(ALL, "NULL")


def test_refusals_do_not_apply_to_unselected_parts():
    """Guard bytes in the fields of the other parts (a NaN-like threshold, k and nbins out of range,
    wild pointers) are not looked at: the call fails later, for its handles."""
    for parts in (MATCHES, TOPK, HIST, MATCHES | TOPK, TOPK | HIST, MATCHES | HIST):
        res = bf.raw_report(None, None, 0, 1, parts, nq=5, expect_rc=E_ARG, threshold=0.4, cap=4, k=5, nbins=64)
        for word in ("nbins", "threshold", "IRIS_TOPK_MAX", "bins is NULL", "out is NULL", "count is NULL"):
            assert word not in res.error, (parts, res.error)
        assert "NULL" in res.error


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()


def test_python_mirror_refuses_without_a_device():
    class Handle:
        handle = None

        def __len__(self):
            return 1

    eng = ih.TemplateBatchEngine.__new__(ih.TemplateBatchEngine)
    eng.handle, eng.nq = None, 5
    with pytest.raises(ih.IrisError):  # no part selected
        eng.report(Handle(), 0)
    with pytest.raises(ih.IrisError):
        eng.report(Handle(), bf.TOPK | bf.HIST, k=5, nbins=48)
    with pytest.raises(ih.IrisError):
        eng.report(Handle(), ALL, threshold=0.4, cap=2, k=65, nbins=64)
