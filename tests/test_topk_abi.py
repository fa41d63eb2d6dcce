"""CPU: the top-k ABI surface (iris_template_topk, iris_resolver_topk, iris_resolver_topk_masks,
iris_topk_merge) -- the four entry points are exported and named in the header, the Rust
declarations, iris_hip.hpp and the Python mirror; each refuses bad arguments with a message before
it touches a device; a C++ program using the iris_hip.hpp forms compiles and links
(tests/test_gpu_topk.py runs it); and the host-only merge equals a numpy restatement of the order
(exact integer cross-products, then the index -- never floats)."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "topk.cpp"
NEW = ["iris_template_topk", "iris_resolver_topk", "iris_resolver_topk_masks", "iris_topk_merge"]
E_ARG = -1
ROT = 31


def build_topk_program(outdir):
    """Compiles tests/cpp/topk.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "topk"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def _calls(lib):
    """name -> f(k, out, count, parts): the entry point with NULL handles and otherwise plausible
    arguments (one record, one 31-element share array)."""
    rows = np.zeros(ROT, np.uint16)
    ptrs = (ctypes.c_void_p * 1)(rows.ctypes.data)
    den = rows.ctypes.data_as(ctypes.c_void_p)
    return {
        "iris_template_topk": lambda k, out, cnt, parts=1: lib.iris_template_topk(None, None, 0, 1, 0, k, out, cnt),
        "iris_resolver_topk": lambda k, out, cnt, parts=1: lib.iris_resolver_topk(None, ptrs, parts, den, 1, 0, k, out,
                                                                                  cnt),
        "iris_resolver_topk_masks": lambda k, out, cnt, parts=1: lib.iris_resolver_topk_masks(None, None, 0, 1, ptrs,
                                                                                              parts, 0, k, out, cnt),
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
    assert re.search(r"#define IRIS_TOPK_MAX 64\b", header) and "pub const IRIS_TOPK_MAX: u32 = 64;" in ffi
    assert ih.TOPK_MAX == 64
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    assert engines.count("pub fn topk(") == 2 and "pub fn resolver_topk(" in engines
    assert engines.count("pub fn matches(") == 2
    assert hasattr(ih.TemplateEngine, "topk") and hasattr(ih.MasksEngine, "topk")
    assert hasattr(ih, "resolver_topk") and hasattr(ih, "merge_topk")
    assert hpp.count("std::vector<Match> topk(") == 2 and "resolver_topk(" in hpp and "topk_merge(" in hpp


def test_header_comments_cite_the_reference_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    sec = header[header.index("- top-k\n"):header.index("int iris_topk_merge(")]
    assert "src/main.rs:616-621" in sec and "src/template.rs:43-47" in sec
    assert "no reference counterpart" in sec
    for word in ("batch engines", "host-array forms", "asynchronous pipeline", "device groups", "k > 64"):
        assert word in sec, word
    for s in NEW:  # every entry point's own comment names a reference line
        decl = header.index("int " + s + "(")
        comment = header[header.rindex("/*", 0, decl):decl]
        assert re.search(r"src/(main|template)\.rs:\d+", comment), s


def test_null_handles_are_refused_without_a_gpu():
    lib = ih.load_library()
    calls, _keep = _calls(lib)
    out = (ih.Match * 1)()
    cnt = ctypes.c_uint32(77)
    for name, f in calls.items():
        assert f(1, out, ctypes.byref(cnt)) == E_ARG, name
        assert "NULL" in _last_error(lib), name
    assert cnt.value == 77 and out[0].index == 0


def test_value_arguments_are_refused_before_the_handles():
    lib = ih.load_library()
    calls, _keep = _calls(lib)
    out = (ih.Match * 1)()
    ctypes.memset(out, 0xA5, ctypes.sizeof(out))
    before = bytes(out)
    cnt = ctypes.c_uint32(77)
    recs = (ih.Match * 1)()
    calls["iris_topk_merge"] = lambda k, o, c, parts=1: lib.iris_topk_merge(recs, 1, k, o, c)
    for name, f in calls.items():
        for k in (0, 65, 2**31):
            assert f(k, out, ctypes.byref(cnt)) == E_ARG, (name, k)
            assert re.search(r"\bk\b", _last_error(lib)), (name, k)
        assert f(1, out, None) == E_ARG, name
        assert "count" in _last_error(lib), name
        assert f(1, None, ctypes.byref(cnt)) == E_ARG, name
        assert "out is NULL" in _last_error(lib), name
    for name in ("iris_resolver_topk", "iris_resolver_topk_masks"):
        for parts in (0, 9, 2**31):
            assert calls[name](1, out, ctypes.byref(cnt), parts) == E_ARG, (name, parts)
            assert "parts" in _last_error(lib), (name, parts)
    assert lib.iris_topk_merge(None, 1, 1, out, ctypes.byref(cnt)) == E_ARG and "records" in _last_error(lib)
    assert cnt.value == 77 and bytes(out) == before


def test_cpp_program_compiles(tmp_path):
    assert build_topk_program(tmp_path).exists()


# ---------------------------------------------------------------- iris_topk_merge against numpy


def make(records):
    """[(num, den, index)] -> Match array (distance = the f64 quotient, rotation = index % 31 - 15)."""
    arr = (ih.Match * max(1, len(records)))()
    for m, (num, den, index) in zip(arr, records):
        m.num, m.den, m.index, m.rotation = int(num), int(den), int(index), int(index) % ROT - 15
        m.distance = float(num) / float(den) if den else float("inf")
    return arr


def np_topk(records, k):
    """Positions of the k first records of the order: exact fraction by integer cross-products (the
    rank of num/den among all the fractions, computed pairwise in int64), then the index."""
    rec = np.asarray(records, np.int64).reshape(-1, 3)
    keep = np.flatnonzero((rec[:, 1] != 0) & (rec[:, 2] != 2**64 - 1))
    num, den, idx = rec[keep, 0], rec[keep, 1], rec[keep, 2]
    # rank[i] = how many records have a strictly smaller fraction: num_j * den_i < num_i * den_j
    rank = (num[None, :] * den[:, None] < num[:, None] * den[None, :]).sum(axis=1)
    order = np.lexsort((idx, rank))
    return keep[order[:k]]


def merge(lib, arr, n, k, room=None):
    out = (ih.Match * (room or k))()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    cnt = ctypes.c_uint32(99)
    rc = lib.iris_topk_merge(arr, n, k, out, ctypes.byref(cnt))
    return rc, cnt.value, out


def check_merge(records, k):
    lib = ih.load_library()
    arr = make(records)
    rc, count, out = merge(lib, arr, len(records), k, room=k + 2)
    assert rc == 0
    want = np_topk(records, k)
    assert count == len(want)
    for j, pos in enumerate(want):
        assert bytes(out[j]) == bytes(arr[int(pos)]), (j, pos)
    assert bytes(out)[count * 32:] == b"\x5a" * ((k + 2 - count) * 32)  # entries past count: untouched
    return [int(p) for p in want]


def test_merge_ties_at_the_cut_and_equal_fractions():
    # 50/100, 100/200 and 1/2 are one fraction: the index alone orders them, whatever (num, den)
    records = [(50, 100, 9), (100, 200, 3), (1, 2, 12), (1, 3, 40), (2, 6, 7), (3, 4, 1), (0, 5, 100), (0, 9, 50)]
    for k in range(1, 9):
        check_merge(records, k)
    assert check_merge(records, 5) == [7, 6, 4, 3, 1]  # 0/9@50, 0/5@100, 2/6@7, 1/3@40, then 100/200@3 of the tie
    # the cut falls inside the tie of three: the lowest indices win
    assert [records[p][2] for p in check_merge(records, 6)][-2:] == [3, 9]
    # large counts: the cross-products need more than 32 bits only past 2^16, but stay exact
    check_merge([(12799, 12800, 1), (6399, 6400, 2), (12798, 12799, 0)], 3)


def test_merge_ignores_empty_records_and_short_inputs():
    lib = ih.load_library()
    records = [(5, 0, 1), (1, 4, 2), (0, 0, 3), (1, 5, 2**64 - 1), (2, 4, 6)]
    arr = make(records)
    arr[3].index = 2**64 - 1
    rc, count, out = merge(lib, arr, 5, 4)
    assert rc == 0 and count == 2 and (out[0].index, out[1].index) == (2, 6)
    assert bytes(out)[64:] == b"\x5a" * 64
    rc, count, out = merge(lib, arr, 0, 4)  # nrecords = 0
    assert rc == 0 and count == 0 and bytes(out) == b"\x5a" * 128
    rc, count, out = merge(lib, None, 0, 4)
    assert rc == 0 and count == 0
    assert ih.merge_topk([], 3) == []
    assert [m.index for m in ih.merge_topk(list(arr), 64)] == [2, 6]


def test_merge_refuses_a_duplicate_index():
    lib = ih.load_library()
    arr = make([(1, 4, 2), (1, 5, 7), (3, 5, 2)])
    rc, count, out = merge(lib, arr, 3, 2)
    assert rc == E_ARG and "same index" in _last_error(lib)
    assert count == 99 and bytes(out) == b"\x5a" * 64
    arr[2].den = 0  # an ignored record's index does not count
    assert merge(lib, arr, 3, 2)[:2] == (0, 2)


@pytest.mark.parametrize("k", [1, 5, 64])
def test_merging_chunk_lists_equals_the_list_of_the_whole(k):
    """Per-chunk top-k lists of a split array, merged, are the top-k of the whole: the lists come
    from the CPU oracle's counts of 300 generated templates (plus exact copies of the query, so
    distance 0 ties cross the chunk borders)."""
    query = oc.gen_templates(99, 0, 1)[0]
    templates = oc.gen_templates(8, 0, 300).copy()
    for i in (3, 99, 100, 250):
        templates[i] = query
    num, den = (np.asarray(a, np.int64) for a in oc.template_counts(query, templates))
    best = []
    for i in range(300):  # best rotation: exact fraction minimum, lowest rotation on ties
        bn, bd = 0, 0
        for r in range(ROT):
            if den[i, r] and (bd == 0 or num[i, r] * bd < bn * den[i, r]):
                bn, bd = int(num[i, r]), int(den[i, r])
        best.append((bn, bd, 1000 + i))
    whole = np_topk(best, k)
    assert [best[p][2] for p in whole[:4]][:min(k, 4)] == [1003, 1099, 1100, 1250][:min(k, 4)]
    lists = []
    for lo, hi in [(0, 100), (100, 101), (101, 300)]:
        lists += [best[lo + int(p)] for p in np_topk(best[lo:hi], k)]
    got = ih.merge_topk(list(make(lists))[:len(lists)], k)
    assert [(m.num, m.den, m.index) for m in got] == [best[p] for p in whole]
