"""CPU: the batched MasksEngine's ABI surface -- the four entry points are exported and refuse bad
arguments before they touch a device, IRIS_MASKS_BATCH_MAX agrees between the header, the Rust
declarations and the Python mirror, and a C++ program using iris_hip.hpp's MasksBatchEngine
compiles and links (tests/test_gpu_masks_batch.py runs it)."""
import ctypes
import pathlib
import re
import subprocess

import numpy as np

import iris_hip as ih

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "masks_batch.cpp"
NEW = ["iris_masks_batch_engine_new", "iris_masks_batch_process", "iris_masks_batch_process_device",
       "iris_resolver_batch_search_masks"]
E_ARG = -1


def build_cpp_program(outdir):
    """Compiles tests/cpp/masks_batch.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "masks_batch"
    lib = ROOT / "mpc-iris-code_amd"
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wextra", f"-I{ROOT / 'include'}", str(CPP_SRC), "-o",
                        str(exe), f"-L{lib}", "-liris_hip", f"-Wl,-rpath,{lib}", "-Wl,-rpath-link,/opt/rocm/lib"],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def _last_error(lib):
    return lib.iris_last_error().decode(errors="replace")


def test_symbols_exported():
    lib = ih.load_library()
    for s in NEW:
        assert hasattr(lib, s), s
        assert s in ih.exported_symbols()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    for s in NEW:
        assert re.search(r"\bint " + s + r"\(", header), s


def test_engine_new_refuses_bad_arguments_without_a_gpu():
    lib = ih.load_library()
    q = np.zeros((1, ih.LIMBS), np.uint64)
    h = ctypes.c_void_p()
    qp = q.ctypes.data_as(ctypes.c_void_p)
    assert lib.iris_masks_batch_engine_new(None, qp, 1, ctypes.byref(h)) == E_ARG
    assert "NULL" in _last_error(lib)
    for nq in (0, ih.MASKS_BATCH_MAX + 1):
        assert lib.iris_masks_batch_engine_new(None, qp, nq, ctypes.byref(h)) == E_ARG
        assert "IRIS_MASKS_BATCH_MAX" in _last_error(lib)
    assert not h.value


def test_process_and_resolve_refuse_null_handles_without_a_gpu():
    lib = ih.load_library()
    out = np.zeros(31, np.uint16)
    for f in (lib.iris_masks_batch_process, lib.iris_masks_batch_process_device):
        assert f(None, None, 0, 1, out.ctypes.data_as(ctypes.c_void_p)) == E_ARG
        assert _last_error(lib)
    m = (ih.Match * 1)()
    ptrs = (ctypes.c_void_p * 1)(out.ctypes.data)
    assert lib.iris_resolver_batch_search_masks(None, None, 0, 1, ptrs, 1, 0, None, m) == E_ARG
    assert _last_error(lib)
    assert lib.iris_resolver_batch_search_masks(None, None, 0, 1, ptrs, 1, 0, None, None) == E_ARG


def test_batch_max_agrees_everywhere():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    m = re.search(r"^#define IRIS_MASKS_BATCH_MAX (\d+)", header, re.M)
    assert m and int(m.group(1)) == 64
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    r = re.search(r"pub const IRIS_MASKS_BATCH_MAX: usize = (\d+);", ffi)
    assert r and int(r.group(1)) == int(m.group(1))
    assert ih.MASKS_BATCH_MAX == int(m.group(1))


def test_bindings_name_the_engine():
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    assert "pub struct MasksBatchEngine" in engines
    assert re.search(r"pub fn new\(queries: &\[Bits\]\) -> Self", engines)
    assert re.search(r"pub fn batch_process\(&self, out: &mut \[Vec<\[u16; 31\]>\], db: &Database", engines)
    assert re.search(r"pub fn resolve\(&self, masks: &Database, first: u64, n: u64, shares_device: &\[\*const u16\]\)"
                     r" -> Result<Vec<\(f64, usize\)>>", engines)
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    for s in NEW:
        assert f"pub fn {s}(" in ffi, s
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    assert "class MasksBatchEngine" in hpp and "iris_resolver_batch_search_masks" in hpp
    assert hasattr(ih, "MasksBatchEngine") and hasattr(ih.MasksBatchEngine, "resolve")


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()
