"""CPU: the ABI surface of the masks batch report (iris_resolver_batch_report_masks) -- the entry
point is exported and named in the header, the Rust declarations, iris_hip.hpp and the Python
mirror, the Rust declaration has the header's signature, the header section states the contract and
the scope between its neighbours, and bad value arguments are refused with a message before a handle
is touched, leaving the struct and every array at their guard bytes."""
import ctypes
import pathlib
import re
import subprocess

import pytest

import iris_hip as ih
import masks_batch_report_fixtures as mf
from masks_batch_report_fixtures import ALL, HIST, MATCHES, NAME, TOPK

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "masks_batch_report.cpp"
E_ARG = -1


def build_cpp_program(outdir):
    """Compiles tests/cpp/masks_batch_report.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "masks_batch_report"
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
    assert f"int {NAME}(" in header and f"pub fn {NAME}(" in ffi
    assert f"ffi::{NAME}(" in engines and NAME + "(" in hpp
    assert callable(ih.MasksBatchEngine.report)
    # the call takes the template batch report's struct: no second one anywhere
    assert header.count("typedef struct iris_batch_report {") == 1 and ffi.count("pub struct IrisBatchReport") == 1


def test_rust_declares_the_headers_signature():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    c = re.search(r"\bint " + NAME + r"\((.*?)\);", header, flags=re.S).group(1)
    c = re.sub(r"/\*.*?\*/", "", c)
    c_params = [" ".join(p.split()) for p in c.split(",")]
    assert c_params == ["iris_engine_t *engine", "const iris_db_t *masks_db", "uint64_t first", "uint64_t n",
                        "const uint16_t *const *shares_device", "uint32_t parts", "uint64_t index_base", "void *report"]
    rust = re.search(r"pub fn " + NAME + r"\((.*?)\) -> c_int;", ffi, flags=re.S).group(1)
    rust_params = [" ".join(p.split()) for p in rust.split(",") if p.strip()]
    assert rust_params == ["engine: *mut IrisEngine", "masks_db: *const IrisDb", "first: u64", "n: u64",
                           "shares_device: *const *const u16", "parts: u32", "index_base: u64", "report: *mut c_void"]
    # and the sibling batch calls' leading parameters
    sib = re.search(r"pub fn iris_resolver_batch_histogram_masks\((.*?)\) -> c_int;", ffi, flags=re.S).group(1)
    assert [" ".join(p.split()) for p in sib.split(",") if p.strip()][:6] == rust_params[:6]


def test_header_states_the_contract_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    assert header.index("- template batch reports\n") < header.index("- masks batch reports\n") < header.index("- arch plugin\n")
    sec = header[header.index("- masks batch reports\n"):header.index("- arch plugin\n")]
    for word in ("BYTE FOR BYTE", "Out of scope", "neither read nor written", "writes nothing", "nothing is launched",
                 "waits once", "stay untouched", "reserved", "iris_batch_report_t", "IRIS_REPORT_",
                 "iris_resolver_batch_search_masks", "nq = 1..64", "query-major", "last bin", "den == 0", "invalid",
                 "1..8", "single-query masks engine", "IRIS_E_ARG", "TILES", "LANES", "once more", "matches_cap == 0",
                 "host-array", "pipelined", "device-group", "per-query thresholds", "search part", "distance batch engine",
                 "K-split", "void *") + mf.SIBLINGS:
        assert word in sec, word
    assert sec.count("int iris_") == 1  # the section declares this call alone
    # the neighbouring sections point here and name no follow-up any more
    resolver = header[header.index("- resolver reports\n"):header.index("int iris_resolver_report(")]
    template = header[header.index("- template batch reports\n"):header.index("typedef struct iris_batch_report {")]
    assert NAME in resolver and NAME in template
    assert "next follow-up" not in header


def refused(parts, message, **kw):
    """A call with NULL handles that must be refused for its value arguments: IRIS_E_ARG with
    `message`, the struct and the arrays untouched (raw_report checks both)."""
    args = dict(threshold=0.4, cap=4, k=5, nbins=64, nparts=3)
    args.update(kw)
    res = mf.raw_report(None, None, 0, 1, None, parts, nq=5, expect_rc=E_ARG, **args)
    assert message in res.error, (res.error, message)


def test_bad_parts_and_reserved_are_refused_whatever_the_handles():
    lib = ih.load_library()
    f = getattr(lib, NAME)
    for parts in (0, 8, 15, 1 << 31):
        r = mf.bf.guard_report()
        r.parts = parts
        before = bytes(r)
        assert f(None, None, 0, 1, None, 3, 0, ctypes.byref(r)) == E_ARG, parts
        assert "parts must be one or more" in lib.iris_last_error().decode() and bytes(r) == before
    assert f(None, None, 0, 1, None, 3, 0, None) == E_ARG
    assert "report is NULL" in lib.iris_last_error().decode()
    for parts in mf.MULTI + [MATCHES, TOPK, HIST]:
        refused(parts, "reserved must be 0", reserved=1)
    # the report's parts are looked at before the share parts
    r = mf.bf.guard_report()
    r.parts = 0
    assert f(None, None, 0, 1, None, 0, 0, ctypes.byref(r)) == E_ARG
    assert "parts must be one or more" in lib.iris_last_error().decode()


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


def test_share_parts_come_after_the_report_and_before_the_handles():
    for nparts in (0, 9):
        for parts in mf.MULTI + [MATCHES, TOPK, HIST]:
            refused(parts, "parts must be 1..8", nparts=nparts)
    # a selected part's bad argument wins over a bad number of share parts
    refused(ALL, "IRIS_TOPK_MAX", k=65, nparts=9)
    refused(ALL, "threshold is NaN", threshold=float("nan"), nparts=0)
    # matches may be NULL when the cap is 0; with every value argument in order the call fails for its handles
    refused(ALL, "NULL", cap=0)
    refused(ALL, "NULL")


def test_refusals_do_not_apply_to_unselected_parts():
    """Guard bytes in the fields of the other parts (a NaN-like threshold, k and nbins out of range,
    wild pointers) are not looked at: the call fails later, for its handles."""
    for parts in (MATCHES, TOPK, HIST, MATCHES | TOPK, TOPK | HIST, MATCHES | HIST):
        res = mf.raw_report(None, None, 0, 1, None, parts, nq=5, expect_rc=E_ARG, threshold=0.4, cap=4, k=5, nbins=64, nparts=3)
        for word in ("nbins", "threshold", "IRIS_TOPK_MAX", "bins is NULL", "out is NULL", "count is NULL", "1..8"):
            assert word not in res.error, (parts, res.error)
        assert "NULL" in res.error


def test_single_query_report_names_this_call():
    """iris_resolver_report_masks refuses a batch engine by naming the batched call (the source: the
    refusal itself needs a live engine and runs in the GPU suite)."""
    src = (ROOT / "mpc-iris-code_amd" / "csrc" / "iris_api_select.hip").read_text()
    body = src[src.index("int iris_resolver_report_masks("):src.index("static int batch_report_args(")]
    assert 'CHK(single_masks_args(e, db, "' + NAME + '"));' in body


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()


def test_python_mirror_refuses_without_a_device():
    class Handle:
        handle = None

        def __len__(self):
            return 1

    eng = ih.MasksBatchEngine.__new__(ih.MasksBatchEngine)
    eng.handle, eng.nq = None, 5
    with pytest.raises(ih.IrisError):  # no part selected
        eng.report(Handle(), [0, 0, 0], 0)
    with pytest.raises(ih.IrisError):
        eng.report(Handle(), [0, 0, 0], mf.TOPK | mf.HIST, k=5, nbins=48)
    with pytest.raises(ih.IrisError):
        eng.report(Handle(), [0, 0, 0], ALL, threshold=0.4, cap=2, k=65, nbins=64)
    with pytest.raises(ih.IrisError):  # the share parts
        eng.report(Handle(), [], ALL, threshold=0.4, cap=2, k=5, nbins=64)
