"""CPU: the histogram ABI surface (iris_template_histogram, iris_template_batch_histogram) -- both
entry points are exported and named in the header, the Rust declarations, iris_hip.hpp and the
Python mirror; each refuses bad arguments with a message before it touches a device and leaves its
outputs alone; a C++ program using the iris_hip.hpp forms compiles and links
(tests/test_gpu_template_batch_histogram.py runs it); the single-query fixture of the GPU tests holds
the edge cases it is meant to hold, by the oracle alone; and the header's f64 binning rule equals
the integer rule the device uses."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "histogram.cpp"
NEW = ["iris_template_histogram", "iris_template_batch_histogram"]
E_ARG = -1
GUARD = 0xA5A5A5A5A5A5A5A5


def build_cpp_program(outdir):
    """Compiles tests/cpp/histogram.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "histogram"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def _outputs():
    bins = np.full(2048, GUARD, np.uint64)
    invalid = np.full(4, GUARD, np.uint64)
    return bins, invalid


def _untouched(bins, invalid):
    return (bins == np.uint64(GUARD)).all() and (invalid == np.uint64(GUARD)).all()


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
        assert f"ffi::{s}(" in engines, s
        assert s + "(" in hpp, s
    assert re.search(r"#define IRIS_HIST_MAX_BINS 1024u?\b", header)
    assert "pub const IRIS_HIST_MAX_BINS: u32 = 1024;" in ffi
    assert ih.HIST_MAX_BINS == 1024
    assert callable(ih.TemplateEngine.histogram) and callable(ih.TemplateBatchEngine.histogram)


def test_header_states_the_contract_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    sec = header[header.index("- histograms\n"):header.index("int iris_template_batch_histogram(")]
    assert "src/template.rs:43-47" in sec and "src/main.rs:616-621" in sec
    assert "Out of scope" in sec and "OVERWRITES" in sec
    for word in ("prefix sum", "floor(num * nbins / den)", "sum(bins) + *invalid == n", "power of two"):
        assert word in sec, word


@pytest.mark.parametrize("name", NEW)
def test_bad_nbins_is_refused_whatever_the_handles(name):
    lib = ih.load_library()
    f = getattr(lib, name)
    bins, invalid = _outputs()
    for nbins in (0, 3, 1000, 2048, 2**31):
        assert f(None, None, 0, 1, nbins, bins.ctypes.data, invalid.ctypes.data) == E_ARG, nbins
        assert "IRIS_HIST_MAX_BINS" in _last_error(lib), nbins
    assert _untouched(bins, invalid)


@pytest.mark.parametrize("name", NEW)
def test_null_pointers_and_handles_are_refused_without_a_gpu(name):
    lib = ih.load_library()
    f = getattr(lib, name)
    bins, invalid = _outputs()
    assert f(None, None, 0, 1, 64, None, invalid.ctypes.data) == E_ARG and "bins is NULL" in _last_error(lib)
    assert f(None, None, 0, 1, 64, bins.ctypes.data, None) == E_ARG and "invalid is NULL" in _last_error(lib)
    for nbins in hf.NBINS:
        assert f(None, None, 0, 1, nbins, bins.ctypes.data, invalid.ctypes.data) == E_ARG
        assert "NULL" in _last_error(lib)
        assert f(None, None, 0, 0, nbins, bins.ctypes.data, invalid.ctypes.data) == E_ARG  # n == 0 too
    assert _untouched(bins, invalid)


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()


def test_single_query_fixture_is_not_vacuous():
    """By the oracle alone: at 1024 bins the edge query's histogram has a record in bin 0, one
    exactly on the edge of bin 256 and its neighbour one bit short in bin 255, one at distance 1.0 in
    bin 1023 and one invalid record; the generated records spread over more than 8 bins."""
    c = hf.single_case()
    d = c.dist["edge"]
    bn, bd = hf.best_rotation(c.edge_query, c.templates)
    assert (bn[0], bd[0]) == (0, 12800) and d[0] == 0.0 and hf.bin_of(d[0], 1024) == 0
    assert (bn[31], bd[31]) == (3200, 12800) and d[31] == 0.25 and hf.bin_of(d[31], 1024) == 256
    assert (bn[32], bd[32]) == (3199, 12800) and hf.bin_of(d[32], 1024) == 255
    assert (bn[256], bd[256]) == (12800, 12800) and d[256] == 1.0 and hf.bin_of(d[256], 1024) == 1023
    assert bd[c.ZERO_MASK] == 0 and np.isinf(d[c.ZERO_MASK])
    for key in ("edge", "gen"):
        bins, invalid = hf.expected(c.dist[key], 1024)
        assert invalid == 1 and int(bins.sum()) + invalid == hf.SMALL_N
        generated = np.delete(c.dist[key], list(c.planted))
        assert len(np.unique(hf.bin_of(generated, 1024))) > 8, key
    bins, _ = hf.expected(d, 1024)
    assert bins[0] == 1 and bins[255] == 1 and bins[256] == 1 and bins[1023] == 1
    # the sub-ranges of the GPU tests see different parts of it
    assert hf.expected(d, 1024, 256, 1)[0][1023] == 1 and hf.expected(d, 1024, 5, 200)[1] == 1
    empty, none = hf.expected(d, 1024, 0, 0)
    assert not empty.any() and none == 0


def test_f64_rule_equals_the_integer_rule():
    """min(nbins - 1, floor(d * nbins)) on the oracle's f64 distances equals
    min(nbins - 1, num * nbins // den) on its integer best rotation."""
    c = hf.single_case()
    for key, q in c.queries.items():
        bn, bd = hf.best_rotation(q, c.templates)
        ok = bd != 0
        assert (np.isinf(c.dist[key]) == ~ok).all()
        assert (c.dist[key][ok] == bn[ok] / bd[ok]).all()
        for nbins in hf.NBINS:
            assert (hf.bin_of(c.dist[key][ok], nbins) == np.minimum(nbins - 1, bn[ok] * nbins // bd[ok])).all(), (key, nbins)
    # and on fractions at and next to every bin edge of the finest histogram
    den = np.int64(12800)
    num = np.arange(0, 12801, dtype=np.int64)
    for nbins in hf.NBINS:
        assert (hf.bin_of(num / den, nbins) == np.minimum(nbins - 1, num * nbins // den)).all()
