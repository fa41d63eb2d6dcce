"""CPU: the ABI surface of template batch top-k (iris_template_batch_topk) -- the entry point is
exported and named in the header (inside the top-k section), the Rust declarations, iris_hip.hpp,
the Python mirror and the three documents; its header comment cites the reference lines it
generalises and states the byte-for-byte contract; it refuses bad value arguments with a message
before it looks at a handle; the single-query call still refuses a batch engine; and a C++ program
using TemplateBatchEngine::topk compiles and links (tests/test_gpu_template_batch_topk.py runs it)."""
import ctypes
import pathlib
import re
import subprocess

import iris_hip as ih

ROOT = pathlib.Path(__file__).resolve().parents[1]
CPP_SRC = ROOT / "tests" / "cpp" / "template_batch_topk.cpp"
NAME = "iris_template_batch_topk"
E_ARG = -1


def build_cpp_program(outdir):
    """Compiles tests/cpp/template_batch_topk.cpp against the in-tree library -> the binary's path."""
    exe = pathlib.Path(outdir) / "template_batch_topk"
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
    assert hasattr(lib, NAME)
    assert NAME in ih.exported_symbols()
    header = (ROOT / "include" / "iris_hip.h").read_text()
    assert re.search(r"\bint " + NAME + r"\(", header)
    # in the top-k section: after the masks batch form, before the host-only merge
    assert header.index("int iris_resolver_batch_topk_masks(") < header.index("int " + NAME + "(") < header.index(
        "int iris_topk_merge(")
    ffi = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "ffi.rs").read_text()
    assert f"pub fn {NAME}(" in ffi
    engines = (ROOT / "bindings" / "rust" / "src" / "iris_hip" / "engines.rs").read_text()
    assert "pub fn batch_topk(" in engines and "ffi::" + NAME in engines
    impl = engines[engines.index("impl TemplateBatchEngine"):]
    assert "pub fn batch_topk(" in impl and "ffi::" + NAME in impl
    hpp = (ROOT / "include" / "iris_hip.hpp").read_text()
    assert NAME + "(" in hpp
    cls = hpp[hpp.index("class TemplateBatchEngine"):]
    assert re.search(r"std::vector<std::vector<Match>> topk\(", cls[:cls.index("\n};")])
    assert hasattr(ih.TemplateBatchEngine, "topk")
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert NAME in (ROOT / doc).read_text(), doc


def test_header_comment_cites_the_reference_and_the_contract():
    header = (ROOT / "include" / "iris_hip.h").read_text()
    decl = header.index("int " + NAME + "(")
    comment = header[header.rindex("/*", 0, decl):decl]
    for cite in ("src/template.rs:43-47", "src/main.rs:616-621"):
        assert cite in comment, cite
    assert "byte for byte" in comment and "iris_template_topk" in comment
    assert "iris_template_batch_search" in comment and "counts" in comment and "TILES" in comment
    assert "8 G" in comment  # the first pass's geometry: lists per query
    # the scope paragraph of the section: the template batch engine is in, no longer a follow-up
    sec = header[header.index("- top-k\n"):header.index("int iris_template_topk(")]
    scope = sec[sec.index("Out of scope"):]
    assert NAME in scope and "iris_resolver_batch_topk_masks" in scope and "follow-up" not in scope
    for word in ("batch engines", "template", "distance", "host-array forms", "asynchronous pipeline", "device groups",
                 "k > 64"):
        assert word in scope, word
    for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
        assert "template batch engine (a follow-up" not in " ".join((ROOT / doc).read_text().split()), doc


def _call(lib, k, out, counts):
    """The entry point with NULL handles and otherwise plausible arguments."""
    return lib.iris_template_batch_topk(None, None, 0, 1, 0, k, out, counts)


def test_value_arguments_are_refused_before_the_handles():
    lib = ih.load_library()
    out = (ih.Match * 2)()
    ctypes.memset(out, 0x5A, ctypes.sizeof(out))
    before = bytes(out)
    counts = (ctypes.c_uint32 * 2)(77, 78)
    for k in (0, 65, 2**31):
        assert _call(lib, k, out, counts) == E_ARG, k
        assert re.search(r"\bk\b", _last_error(lib)), k
        assert list(counts) == [77, 78] and bytes(out) == before
    assert _call(lib, 1, None, counts) == E_ARG
    assert "out is NULL" in _last_error(lib)
    assert _call(lib, 1, out, None) == E_ARG
    assert "counts" in _last_error(lib)
    assert list(counts) == [77, 78] and bytes(out) == before
    # valid value arguments: the NULL handles are what is refused
    for k in (1, 64):
        assert _call(lib, k, out, counts) == E_ARG
        assert "NULL" in _last_error(lib)
        assert list(counts) == [77, 78] and bytes(out) == before


def test_single_query_call_still_refuses_a_batch_engine():
    """iris_template_topk goes through template_args, which refuses an engine with nq > 0."""
    csrc = ROOT / "mpc-iris-code_amd" / "csrc"
    src = (csrc / "iris_api_select.hip").read_text()
    body = src[src.index("int iris_template_topk("):src.index("int iris_resolver_topk(")]
    assert "CHK(template_args(e, db));" in body
    args = (csrc / "iris_api_search.hip").read_text()
    args = args[args.index("int iris_api::template_args("):]
    assert re.search(r"ARG\(e->kind == IRIS_KIND_TEMPLATES && e->nq == 0,", args[:args.index("}")])


def test_cpp_program_compiles(tmp_path):
    assert build_cpp_program(tmp_path).exists()
