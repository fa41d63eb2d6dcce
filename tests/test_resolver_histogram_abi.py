"""CPU: the ABI surface of the resolver histograms (iris_resolver_histogram,
iris_resolver_histogram_masks, iris_resolver_batch_histogram_masks) -- the three entry points are
exported and named in the header, the Rust declarations, iris_hip.hpp and the Python mirror; each
refuses bad value arguments with a message before it looks at a handle and leaves its outputs alone;
a C++ program using the iris_hip.hpp forms compiles and links (tests/test_gpu_resolver_histogram.py
runs it); the small fixture of the GPU tests holds the edge cases it is meant to hold, by the oracle
alone; and the header's f64 binning rule equals the integer rule the device uses over the resolver's
whole value range."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
import resolver_hist_fixtures as rf

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "resolver_histogram.cpp"
NEW = ["iris_resolver_histogram", "iris_resolver_histogram_masks", "iris_resolver_batch_histogram_masks"]
E_ARG = -1
GUARD = 0xA5A5A5A5A5A5A5A5


def build_cpp_program(outdir):
    """Compiles tests/cpp/resolver_histogram.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "resolver_histogram"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def _outputs():
    return np.full(2048, GUARD, np.uint64), np.full(4, GUARD, np.uint64)


def _untouched(bins, invalid):
    return (bins == np.uint64(GUARD)).all() and (invalid == np.uint64(GUARD)).all()


def _call(lib, name, nbins, bins, invalid, parts=1, n=1):
    """An entry point with NULL handles and otherwise plausible arguments."""
    rows = np.zeros(31, np.uint16)
    ptrs = (ctypes.c_void_p * 1)(rows.ctypes.data)
    f = getattr(lib, name)
    if name == "iris_resolver_histogram":
        return f(None, ptrs, parts, rows.ctypes.data, n, nbins, bins, invalid)
    return f(None, None, 0, n, ptrs, parts, nbins, bins, invalid)


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
        for doc in ("README.md", "DESIGN.md"):
            assert s in (ROOT / doc).read_text(), (s, doc)
    # the section follows the template histograms
    assert header.index("int iris_resolver_histogram(") > header.index("int iris_template_batch_histogram(")
    assert callable(ih.resolver_histogram) and "resolver_histogram" in ih.__all__
    assert callable(ih.MasksEngine.histogram) and callable(ih.MasksBatchEngine.histogram)


def test_header_states_the_contract_and_the_scope():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    sec = header[header.index("- resolver histograms\n"):header.index("int iris_resolver_batch_histogram_masks(")]
    assert "src/main.rs:597-621" in sec and "src/lib.rs:97-107" in sec
    for word in ("OVERWRITTEN", "prefix sum", "sum(bins) + *invalid == n", "power of two", "32767", "65535", "2^25",
                 "last bin", "byte for byte", "Out of scope"):
        assert word in sec, word
    # the template section no longer names these forms as missing
    old = header[header.index("- histograms\n"):header.index("int iris_template_batch_histogram(")]
    scope = old[old.index("Out of scope"):]
    assert "resolver forms" not in scope and "masks batch form" not in scope and "device-group" in scope
    # the device rule's comment covers the resolver's value range
    dev = (ROOT / "mpc-iris-code_amd" / "csrc" / "iris_device.hpp").read_text()
    rule = dev[dev.index("One record per lane"):dev.index("void hist_count(")]
    assert "32767" in rule and "65535" in rule and "2^25" in rule


@pytest.mark.parametrize("name", NEW)
def test_bad_value_arguments_are_refused_whatever_the_handles(name):
    lib = ih.load_library()
    bins, invalid = _outputs()
    for nbins in (0, 3, 1000, 2048, 2**31):
        assert _call(lib, name, nbins, bins.ctypes.data, invalid.ctypes.data) == E_ARG, nbins
        assert "IRIS_HIST_MAX_BINS" in _last_error(lib), nbins
    assert _call(lib, name, 64, None, invalid.ctypes.data) == E_ARG and "bins is NULL" in _last_error(lib)
    assert _call(lib, name, 64, bins.ctypes.data, None) == E_ARG and "invalid is NULL" in _last_error(lib)
    for parts in (0, 9, 2**31):
        assert _call(lib, name, 64, bins.ctypes.data, invalid.ctypes.data, parts) == E_ARG, parts
        assert "parts" in _last_error(lib), parts
    assert _untouched(bins, invalid)


@pytest.mark.parametrize("name", NEW)
def test_null_handles_are_refused_without_a_gpu(name):
    lib = ih.load_library()
    bins, invalid = _outputs()
    for nbins in hf.NBINS:
        for n in (1, 0):  # n == 0 too: the handles are checked before the range
            assert _call(lib, name, nbins, bins.ctypes.data, invalid.ctypes.data, n=n) == E_ARG, (nbins, n)
            assert "NULL" in _last_error(lib), (nbins, n)
    assert _untouched(bins, invalid)


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()


def test_small_fixture_is_not_vacuous():
    """By the oracle alone, at 1024 bins: in every planted slab a record in bin 0, two exactly on the
    edge of bin 256 and their neighbour one count short in bin 255; one invalid record per slab; the
    garbage slab reaches the last bin through distances above 1; the background spreads over more
    than 8 bins."""
    c = rf.small_case()
    for parts in rf.PARTS:
        for q in range(c.NQ):
            e = c.exp[parts][q]
            bins, invalid = c.want(parts, q, 1024)
            assert invalid == 1 and e.den[c.ZERO] == 0 and np.isinf(e.dist[c.ZERO])
            assert int(bins.sum()) + invalid == c.N
            ok = e.den != 0
            assert len(np.unique(hf.bin_of(e.dist[ok], 1024))) > 8, (parts, q)
            if q == c.GARBAGE:
                over = ok & (e.num > e.den)
                assert over.any() and (e.dist[over] > 1.0).all()
                assert bins[1023] >= over.sum() and (hf.bin_of(e.dist[over], 1024) == 1023).all()
                continue
            assert e.num[0] == 0 and e.dist[0] == 0.0 and bins[0] == 1
            for rec in (31, 256):
                assert 4 * e.num[rec] == e.den[rec] and e.dist[rec] == 0.25 and hf.bin_of(e.dist[rec], 1024) == 256
            assert 4 * (e.num[32] + 1) == e.den[32] and hf.bin_of(e.dist[32], 1024) == 255
            assert bins[256] == 2 and bins[255] == 1
            assert [e.rot[r] + 15 for r in c.PLANTS] == [c.plant_rot[q, r] for r in c.PLANTS]
            # the sub-ranges of the GPU tests see different parts of it
            assert c.want(parts, q, 1024, 256, 1)[0][256] == 1 and c.want(parts, q, 1024, 33, 1)[0].sum() == 1
            assert c.want(parts, q, 1024, 5, 200)[1] == 1
            empty, none = c.want(parts, q, 1024, 0, 0)
            assert not empty.any() and none == 0


def test_f64_rule_equals_the_integer_rule():
    """min(nbins - 1, floor(d * nbins)) on the f64 quotient equals min(nbins - 1, num * nbins // den)
    in integers: on the fixture's own (num, den), and for every den in 1..65535 with num at and beside
    every edge of 1024 bins, num > den included (num <= 32767, so num * nbins < 2^25)."""
    c = rf.small_case()
    for parts in rf.PARTS:
        for e in c.exp[parts]:
            ok = e.den != 0
            assert (e.dist[ok] == e.num[ok] / e.den[ok]).all()
            for nbins in hf.NBINS:
                assert (hf.bin_of(e.dist[ok], nbins) == np.minimum(nbins - 1, e.num[ok] * nbins // e.den[ok])).all()
    den = np.arange(1, 65536, dtype=np.int64)[:, None]
    for nbins in hf.NBINS:  # the edges of each bin count; the integer rule in u32, as on the device
        for j0 in range(0, nbins + 1, 128):
            j = np.arange(j0, min(j0 + 128, nbins + 1), dtype=np.int64)[None, :]
            edge = -((-j * den) // nbins)  # the lowest num in bin j: ceil(j den / nbins)
            num = np.clip(np.concatenate([edge - 1, edge, edge + 1], axis=1), 0, 32767).astype(np.uint32)
            dd = np.broadcast_to(den.astype(np.uint32), num.shape)
            assert int(num.max()) * nbins < 2**25
            want = np.minimum(np.uint32(nbins - 1), num * np.uint32(nbins) // dd)
            assert (hf.bin_of(num / dd, nbins) == want).all(), (j0, nbins)
    # every uneq a u16 sum can decode to, against the largest denominators (distances far above 1)
    num = np.arange(0, 32768, dtype=np.int64)
    for d in (1, 2, 3, 12800, 12801, 32767, 65535):
        for nbins in hf.NBINS:
            assert (hf.bin_of(num / d, nbins) == np.minimum(nbins - 1, num * nbins // d)).all(), (d, nbins)
