"""CPU: the ABI surface of the resolver reports (iris_resolver_report, iris_resolver_report_masks) --
both entry points are exported and named in the header, the Rust declarations, iris_hip.hpp and the
Python mirror, the header section states the contract and the scope, bad arguments are refused with
a message before a device is touched and leave the struct and every array at their guard bytes, and
the fixtures of the GPU tests hold what those tests need, by the oracle alone."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
import resolver_hist_fixtures as rhf
import resolver_report_fixtures as rr
from resolver_report_fixtures import ALL, HIST, MATCHES, TOPK

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "resolver_report.cpp"
E_ARG = -1
ABOVE_QUARTER = float(np.nextafter(0.25, np.inf))


def build_cpp_program(outdir):
    """Compiles tests/cpp/resolver_report.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "resolver_report"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def calls(nparts=3):
    """Both entry points with NULL handles and `nparts` (NULL) share arrays."""
    ptrs = [None] * min(max(nparts, 1), 8)
    return [rr.plain_call(None, ptrs, 0, 1, nparts=nparts), rr.masks_call(None, None, 0, 1, ptrs, nparts=nparts)]


def test_symbols_exported_and_named_everywhere():
    lib = ih.load_library()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    for name in rr.NAMES:
        assert hasattr(lib, name) and name in ih.exported_symbols(), name
        assert re.search(r"\bint " + name + r"\(", header), name
        assert f"pub fn {name}(" in ffi and f"ffi::{name}(" in engines and name + "(" in hpp, name
    assert callable(ih.MasksEngine.report) and callable(ih.resolver_report) and "resolver_report" in ih.__all__
    assert "pub fn resolver_report(" in engines and "Report resolver_report(" in hpp


def test_header_states_the_contract_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    assert header.index("- resolver histograms\n") < header.index("- resolver reports\n") < header.index("- arch plugin\n")
    sec = header[header.index("- resolver reports\n"):header.index("- arch plugin\n")]
    for word in ("BYTE FOR BYTE", "Out of scope", "neither read nor written", "writes nothing", "nothing is launched",
                 "waits once", "src/main.rs:597-621", "iris_resolver_matches_masks", "iris_resolver_topk_masks",
                 "iris_resolver_histogram_masks", "iris_resolver_matches ", "iris_resolver_topk ", "iris_resolver_histogram ",
                 "last bin", "invalid", "1..8", "masks batch engine", "iris_resolver_batch_report_masks", "host-array",
                 "pipelined", "device groups", "search part"):
        assert word in sec, word
    # the combined passes section points here and still names the masks form
    combined = header[header.index("- combined passes\n"):header.index("int iris_template_report(")]
    assert "iris_resolver_report_masks" in combined and "resolver reports" in combined and "natural next" not in combined


def test_bad_report_parts_are_refused_whatever_the_handles():
    lib = ih.load_library()
    for call in calls():
        for parts in (0, 8, 15, 1 << 31):
            r = rr.rf.guard_report()
            r.parts = parts
            before = bytes(r)
            assert call(ctypes.byref(r)) == E_ARG, parts
            assert "parts must be one or more" in lib.iris_last_error().decode() and bytes(r) == before
        assert call(None) == E_ARG and "report is NULL" in lib.iris_last_error().decode()


def refused(parts, message, nparts=3, **kw):
    args = dict(threshold=0.4, cap=4, k=5, nbins=64)
    args.update(kw)
    for call in calls(nparts):
        res = rr.raw_report(call, 1, parts, expect_rc=E_ARG, **args)
        assert message in res.error, (res.error, message)


def test_each_parts_arguments_fall_under_its_siblings_rules():
    for parts in (MATCHES, MATCHES | TOPK, ALL):
        refused(parts, "threshold is NaN", threshold=float("nan"))
    for parts in (TOPK, TOPK | HIST, ALL):
        for k in (0, 65):
            refused(parts, "IRIS_TOPK_MAX", k=k)
    for parts in (HIST, MATCHES | HIST, ALL):
        for nbins in (0, 48, 2048):
            refused(parts, "IRIS_HIST_MAX_BINS", nbins=nbins)


def test_share_parts_are_checked_after_the_value_arguments_and_before_the_handles():
    for nparts in (0, 9):
        for parts in rr.SUBSETS:
            refused(parts, "parts must be 1..8", nparts=nparts)
        # a bad value argument is reported first
        refused(ALL, "threshold is NaN", nparts=nparts, threshold=float("nan"))
        refused(TOPK, "IRIS_TOPK_MAX", nparts=nparts, k=0)
        refused(HIST, "IRIS_HIST_MAX_BINS", nparts=nparts, nbins=3)
    # every value in order: the call fails for its handles
    refused(ALL, "NULL")


def test_null_pointers_of_selected_parts_are_refused():
    lib = ih.load_library()

    def run(call, parts, **null):
        r = rr.rf.guard_report()
        marr, tarr = rr.rf.match_array(4), rr.rf.match_array(5)
        bins = np.full(64, rr.GUARD, np.uint64)
        r.parts, r.threshold, r.matches_cap, r.k, r.nbins = parts, 0.4, 4, 5, 64
        r.matches = None if "matches" in null else ctypes.cast(marr, ctypes.POINTER(ih.Match))
        r.topk = None if "topk" in null else ctypes.cast(tarr, ctypes.POINTER(ih.Match))
        r.bins = None if "bins" in null else bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        before = bytes(r)
        rc = call(ctypes.byref(r))
        assert bytes(r) == before and (bins == np.uint64(rr.GUARD)).all()
        return rc, lib.iris_last_error().decode()

    for call in calls():
        assert run(call, ALL, matches=1) == (E_ARG, "out is NULL with cap > 0")
        rc, msg = run(call, ALL, topk=1)
        assert rc == E_ARG and "out is NULL" in msg
        rc, msg = run(call, ALL, bins=1)
        assert rc == E_ARG and "bins is NULL" in msg
        rc, msg = run(call, ALL)
        assert rc == E_ARG and "NULL" in msg


def test_refusals_do_not_apply_to_unselected_parts():
    lib = ih.load_library()
    for call in calls():
        for parts, fields in ((TOPK, dict(k=5)), (HIST, dict(nbins=64)), (MATCHES, dict(threshold=0.4, matches_cap=0))):
            r = ih.Report()
            r.parts, r.k, r.nbins, r.threshold = parts, 0, 48, float("nan")
            tarr = rr.rf.match_array(5)
            bins = np.zeros(64, np.uint64)
            if parts == TOPK:
                r.topk = ctypes.cast(tarr, ctypes.POINTER(ih.Match))
            if parts == HIST:
                r.bins = bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
            for f, v in fields.items():
                setattr(r, f, v)
            assert call(ctypes.byref(r)) == E_ARG
            msg = lib.iris_last_error().decode()
            for word in ("nbins", "threshold", "IRIS_TOPK_MAX", "bins is NULL", "out is NULL", "1..8"):
                assert word not in msg, (parts, msg)
            assert "NULL" in msg


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()


def test_python_mirrors_refuse_without_a_device():
    class Handle:
        handle = None

        def __len__(self):
            return 1

    eng = ih.MasksEngine.__new__(ih.MasksEngine)
    eng.handle = None
    with pytest.raises(ih.IrisError):  # no part selected
        eng.report(Handle(), [0, 0, 0])
    with pytest.raises(ih.IrisError):
        eng.report(Handle(), [0, 0, 0], nbins=48)
    with pytest.raises(ih.IrisError):
        ih.resolver_report(Handle(), [0, 0, 0], 0, 1)
    with pytest.raises(ih.IrisError):
        ih.resolver_report(Handle(), [0, 0, 0], 0, 1, k=65)


def test_fixtures_are_not_vacuous():
    """By the oracle alone, on query 0 and on the garbage slab of the small case and query 0 of the
    large one."""
    c = rhf.small_case()
    for parts in rhf.PARTS:
        e = c.exp[parts][0]
        for t, inside in ((0.25, {0, 32}), (ABOVE_QUARTER, {0, 31, 32, 256})):
            hits = set(int(i) for i in e.hits(t))
            assert inside <= hits and not ({31, 256} - inside) & hits, (parts, t)
        assert e.den[c.ZERO] == 0 and np.isinf(e.dist[c.ZERO]) and c.ZERO not in e.hits(float("inf"))
        g = c.exp[parts][c.GARBAGE]
        assert (g.dist[np.isfinite(g.dist)] > 1.0).any(), parts
        assert hf.expected(g.dist, 64)[0][63] >= 1
        for first, n in ((33, 1), (256, 1)):
            assert len(rr.order(e, first, n)) < 16
        assert len(rr.order(e, 0, c.N)) == c.N - 1
        # equal fractions in different terms, in different tiles: the index decides
        top = rr.order(e, 0, c.N)
        assert list(top[:4]) == [0, 32, 31, 256] and e.dist[31] == e.dist[256] == 0.25
    large = rhf.large_case()
    assert len(large.exp[0].hits(0.5)) > rr.MATCH_FIRST_ROOM
    assert large.exp[0].den[large.ZERO] == 0
