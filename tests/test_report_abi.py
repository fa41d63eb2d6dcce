"""CPU: the ABI surface of the combined pass (iris_template_report) -- the entry point is exported and
named in the header, the Rust declarations, iris_hip.hpp and the Python mirror, the three part
constants agree everywhere, the ctypes struct has the layout a C++ compiler gives the header's
struct, bad arguments are refused with a message before a device is touched and leave the struct and
every array alone, and the fixtures of the GPU tests hold what those tests need, by the oracle alone."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
import report_fixtures as rf

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "report.cpp"
NAME = "iris_template_report"
E_ARG = -1
FIELDS = ["parts", "k", "nbins", "topk_count", "threshold", "matches", "matches_cap", "matches_count", "topk", "bins",
          "invalid"]

LAYOUT_PROGRAM = r"""
#include <cstddef>
#include <cstdio>
#include "iris_hip.h"
int main() {
    std::printf("sizeof %zu\n", sizeof(iris_report_t));
#define F(f) std::printf(#f " %zu %zu\n", offsetof(iris_report_t, f), sizeof(((iris_report_t *)0)->f))
    F(parts); F(k); F(nbins); F(topk_count); F(threshold); F(matches); F(matches_cap); F(matches_count); F(topk);
    F(bins); F(invalid);
    std::printf("consts %d %d %d\n", IRIS_REPORT_MATCHES, IRIS_REPORT_TOPK, IRIS_REPORT_HIST);
    return 0;
}
"""


def build_cpp_program(outdir):
    """Compiles tests/cpp/report.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "report"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def test_symbol_exported_and_named_everywhere():
    lib = ih.load_library()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    assert hasattr(lib, NAME) and NAME in ih.exported_symbols()
    assert re.search(r"\bint " + NAME + r"\(", header)
    assert f"pub fn {NAME}(" in ffi and f"ffi::{NAME}(" in engines and NAME + "(" in hpp
    assert "pub struct IrisReport" in ffi and "#[repr(C)]\n#[derive(Clone, Copy, Debug)]\npub struct IrisReport" in ffi
    for name, value in (("MATCHES", 1), ("TOPK", 2), ("HIST", 4)):
        assert re.search(rf"#define IRIS_REPORT_{name} {value}\b", header), name
        assert f"pub const IRIS_REPORT_{name}: u32 = {value};" in ffi, name
        assert getattr(ih, f"REPORT_{name}") == value and getattr(rf, name) == value
    assert callable(ih.TemplateEngine.report)
    # the Rust struct lists the header's fields in the header's order
    rust = re.search(r"pub struct IrisReport \{(.*?)\}", ffi, flags=re.S).group(1)
    assert re.findall(r"pub (\w+):", rust) == FIELDS
    assert [f for f, _ in ih.Report._fields_] == FIELDS


def test_header_states_the_contract_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    assert header.index("- histograms\n") < header.index("- combined passes\n") < header.index("- resolver histograms\n")
    sec = header[header.index("- combined passes\n"):header.index("int " + NAME + "(")]
    assert "src/template.rs:43-47" in sec and "src/main.rs:616-621" in sec
    for word in ("BYTE FOR BYTE", "Out of scope", "neither read nor written", "writes nothing", "nothing is launched",
                 "iris_resolver_report_masks", "waits once"):
        assert word in sec, word


def test_struct_layout_equals_the_compilers(tmp_path):
    src = tmp_path / "layout.cpp"
    src.write_text(LAYOUT_PROGRAM)
    exe = tmp_path / "layout"
    r = subprocess.run(["g++", "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    assert lines[0] == f"sizeof {ctypes.sizeof(ih.Report)}"
    got = {ln.split()[0]: (int(ln.split()[1]), int(ln.split()[2])) for ln in lines[1:1 + len(FIELDS)]}
    want = {f: (getattr(ih.Report, f).offset, getattr(ih.Report, f).size) for f in FIELDS}
    assert got == want
    assert lines[1 + len(FIELDS)] == "consts 1 2 4"
    # no implicit padding: the fields tile the struct
    end = 0
    for f in FIELDS:
        assert want[f][0] == end, f
        end += want[f][1]
    assert end == ctypes.sizeof(ih.Report) == 72


def refused(parts, message, **kw):
    """A call with NULL handles that must be refused for its value arguments: IRIS_E_ARG with
    `message`, the struct and the arrays untouched (raw_report checks both)."""
    args = dict(threshold=0.4, cap=4, k=5, nbins=64)
    args.update(kw)
    res = rf.raw_report(None, None, 0, 1, parts, expect_rc=E_ARG, **args)
    assert message in res.error, (res.error, message)


def test_bad_parts_are_refused_whatever_the_handles():
    lib = ih.load_library()
    for parts in (0, 8, 15, 1 << 31):
        r = rf.guard_report()
        r.parts = parts
        before = bytes(r)
        assert lib.iris_template_report(None, None, 0, 1, 0, ctypes.byref(r)) == E_ARG, parts
        assert "parts" in _last_error(lib) and bytes(r) == before
    assert lib.iris_template_report(None, None, 0, 1, 0, None) == E_ARG and "report is NULL" in _last_error(lib)


def test_each_parts_arguments_fall_under_its_siblings_rules():
    for parts in (rf.MATCHES, rf.MATCHES | rf.TOPK, rf.ALL):
        refused(parts, "threshold is NaN", threshold=float("nan"))
    for parts in (rf.TOPK, rf.TOPK | rf.HIST, rf.ALL):
        for k in (0, 65):
            refused(parts, "IRIS_TOPK_MAX", k=k)
    for parts in (rf.HIST, rf.MATCHES | rf.HIST, rf.ALL):
        for nbins in (0, 48, 2048):
            refused(parts, "IRIS_HIST_MAX_BINS", nbins=nbins)


def test_null_pointers_of_selected_parts_are_refused():
    lib = ih.load_library()

    def call(parts, **null):
        r = rf.guard_report()
        marr, tarr = rf.match_array(4), rf.match_array(5)
        bins = np.full(64, rf.GUARD, np.uint64)
        r.parts, r.threshold, r.matches_cap, r.k, r.nbins = parts, 0.4, 4, 5, 64
        r.matches = None if "matches" in null else ctypes.cast(marr, ctypes.POINTER(ih.Match))
        r.topk = None if "topk" in null else ctypes.cast(tarr, ctypes.POINTER(ih.Match))
        r.bins = None if "bins" in null else bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        before = bytes(r)
        rc = lib.iris_template_report(None, None, 0, 1, 0, ctypes.byref(r))
        assert bytes(r) == before and (bins == np.uint64(rf.GUARD)).all()
        return rc, _last_error(lib)

    assert call(rf.ALL, matches=1) == (E_ARG, "out is NULL with cap > 0")
    rc, msg = call(rf.ALL, topk=1)
    assert rc == E_ARG and "out is NULL" in msg
    rc, msg = call(rf.ALL, bins=1)
    assert rc == E_ARG and "bins is NULL" in msg
    # with every value argument in order the call fails for its handles
    rc, msg = call(rf.ALL)
    assert rc == E_ARG and "NULL" in msg


def test_refusals_do_not_apply_to_unselected_parts():
    """parts = TOPK with nbins = 48 (and a NaN threshold, and NULL arrays of the other parts) is not
    refused for them: it fails later, for the handle."""
    lib = ih.load_library()
    for parts, fields in ((rf.TOPK, dict(k=5)), (rf.HIST, dict(nbins=64)), (rf.MATCHES, dict(threshold=0.4, matches_cap=0))):
        r = ih.Report()
        r.parts, r.k, r.nbins, r.threshold = parts, 0, 48, float("nan")
        tarr = rf.match_array(5)
        bins = np.zeros(64, np.uint64)
        if parts == rf.TOPK:
            r.topk = ctypes.cast(tarr, ctypes.POINTER(ih.Match))
        if parts == rf.HIST:
            r.bins = bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        for f, v in fields.items():
            setattr(r, f, v)
        assert lib.iris_template_report(None, None, 0, 1, 0, ctypes.byref(r)) == E_ARG
        msg = _last_error(lib)
        for word in ("nbins", "threshold", "IRIS_TOPK_MAX", "bins is NULL", "out is NULL"):
            assert word not in msg, (parts, msg)
        assert "NULL" in msg


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()


def test_python_mirror_refuses_without_a_device():
    class Handle:
        handle = None

        def __len__(self):
            return 1

    eng = ih.TemplateEngine.__new__(ih.TemplateEngine)
    eng.handle = None
    with pytest.raises(ih.IrisError):  # no part selected
        eng.report(Handle())
    with pytest.raises(ih.IrisError):
        eng.report(Handle(), nbins=48)


def test_fixtures_are_not_vacuous():
    """By the oracle alone: the small case has a short and a long match list and one invalid record;
    the large case's query 0 has a handful of matches under 0.46 and, under 0.47, more than the 1100
    records of the overflow test's cap and than the 1024 of the first pass's room; its query 3 has no
    valid record; and two of query 0's 70 closest records are at the same distance, so the index
    decides inside a top-k list of 64."""
    c = hf.single_case()
    d = c.dist["gen"]
    assert int((d < 0.48).sum()) == 84 and int((d < 0.5).sum()) == 253 and int(np.isinf(d).sum()) == 1
    assert int(np.isinf(c.dist["edge"]).sum()) == 1
    large = hf.large_case()
    d0 = large.dist(0)
    assert int((d0 < 0.46).sum()) == 12 and int((d0 < 0.47).sum()) == 1373
    assert 1373 > 1100 > 1024
    assert np.isinf(large.dist(3)).all()
    best = np.sort(d0)[:70]
    assert (np.diff(best) == 0).any()
    assert np.count_nonzero(hf.expected(d0, 1024)[0]) > 20
