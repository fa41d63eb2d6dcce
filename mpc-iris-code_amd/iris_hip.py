"""iris_hip — Python mirror of the reference's engine API over the C ABI.

Mirrors recmo/mpc-iris-code (v0.8.0) names and argument meaning:

    reference (Rust)                              here
    Bits / EncodedBits / Template (value types)   Bits / EncodedBits / Template
    encode(&Template) -> EncodedBits              encode(template)          src/lib.rs:16-26
    DistanceEngine::new / batch_process           DistanceEngine            src/lib.rs:28-53
    MasksEngine::new / batch_process              MasksEngine               src/lib.rs:55-80
    distances / denominators                      distances / denominators  src/lib.rs:82-94
    decode_distance                               decode_distance           src/lib.rs:97-107
    Template::distance / fraction_hamming         TemplateEngine            src/template.rs:43-64
    arch::dot_bool / arch::dot_u16                dot_bool / dot_u16        src/arch/generic.rs:4-16

Every compute call goes to libiris_hip.so (hand-written gfx950 kernels).  If
the library or a gfx950 device is missing the calls raise — there is no CPU
fallback in this module.
"""
from __future__ import annotations

import ctypes
import math
import os
import pathlib
import threading

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
# IRIS_HIP_LIB points at an alternative in-tree build (kernel experiments under tools/)
LIB_PATH = pathlib.Path(os.environ.get("IRIS_HIP_LIB", HERE / "libiris_hip.so"))


def _load_pycall():
    """The per-call fast path (csrc/iris_pycall.c, built beside the library and linked to it): the
    host-slice engine call without ctypes' per-call marshalling; None where it is not built or a
    non-default library is in use (IRIS_HIP_LIB).  Loaded on the first such call, after
    load_library(), so that importing this module loads no HIP runtime: a process that imports
    torch later (bench.py's ranks) keeps the load order it had without the fast path (torch bundles
    its own libamdhip64.so.7; whichever is mapped first serves both)."""
    global _pycall
    with _lock:
        if _pycall is not _UNLOADED:
            return _pycall
        _pycall = None
        p = HERE / "_iris_pycall.so"
        if "IRIS_HIP_LIB" in os.environ or not p.exists():
            return None
        import importlib.util
        try:
            spec = importlib.util.spec_from_file_location("_iris_pycall", p)
            mod = importlib.util.module_from_spec(spec)
            spec.loader.exec_module(mod)
        except (ImportError, OSError):
            return None
        _pycall = mod
        return mod


_UNLOADED = object()
_pycall = _UNLOADED
_NULL = ctypes.c_void_p()

COLS, ROWS, BITS, LIMBS, ROTATIONS = 200, 64, 12800, 200, 31
KIND_MASKS, KIND_SHARES, KIND_TEMPLATES = 1, 2, 3
LAYOUT_DEFAULT, LAYOUT_LANES, LAYOUT_TILES = 0, 1, 2
DISTANCE_BATCH_MAX = 64  # IRIS_DISTANCE_BATCH_MAX: queries of a DistanceBatchEngine
MASKS_BATCH_MAX = 64  # IRIS_MASKS_BATCH_MAX: queries of a MasksBatchEngine
_REC_DTYPE = {KIND_MASKS: (np.uint64, LIMBS), KIND_SHARES: (np.uint16, BITS), KIND_TEMPLATES: (np.uint64, 2 * LIMBS)}


class IrisError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"iris_hip error {code}: {msg}")
        self.code = code


class Match(ctypes.Structure):
    """iris_match_t: the resolver's (min_distance, min_index) (src/main.rs:581-621)."""

    _fields_ = [("distance", ctypes.c_double), ("index", ctypes.c_uint64), ("num", ctypes.c_uint32),
                ("den", ctypes.c_uint32), ("rotation", ctypes.c_int32), ("reserved", ctypes.c_uint32)]

    def __repr__(self):
        return (f"Match(distance={self.distance!r}, index={self.index}, num={self.num}, den={self.den}, "
                f"rotation={self.rotation})")


REPORT_MATCHES, REPORT_TOPK, REPORT_HIST = 1, 2, 4  # IRIS_REPORT_*


class Report(ctypes.Structure):
    """iris_report_t: the arguments and results of iris_template_report and the resolver reports."""

    _fields_ = [("parts", ctypes.c_uint32), ("k", ctypes.c_uint32), ("nbins", ctypes.c_uint32),
                ("topk_count", ctypes.c_uint32), ("threshold", ctypes.c_double),
                ("matches", ctypes.POINTER(Match)), ("matches_cap", ctypes.c_uint64),
                ("matches_count", ctypes.c_uint64), ("topk", ctypes.POINTER(Match)),
                ("bins", ctypes.POINTER(ctypes.c_uint64)), ("invalid", ctypes.c_uint64)]


class ReportResult:
    """What TemplateEngine.report(), MasksEngine.report() and resolver_report() return; the fields of a part that was not asked for are None."""

    __slots__ = ("matches", "matches_count", "topk", "bins", "invalid")

    def __init__(self):
        self.matches = self.matches_count = self.topk = self.bins = self.invalid = None

    def __repr__(self):
        return (f"ReportResult(matches_count={self.matches_count}, topk={None if self.topk is None else len(self.topk)}, "
                f"bins={None if self.bins is None else len(self.bins)}, invalid={self.invalid})")


class BatchReport(ctypes.Structure):
    """iris_batch_report_t: the arguments of iris_template_batch_report (the results go to its arrays)."""

    _fields_ = [("parts", ctypes.c_uint32), ("k", ctypes.c_uint32), ("nbins", ctypes.c_uint32),
                ("reserved", ctypes.c_uint32), ("threshold", ctypes.c_double),
                ("matches", ctypes.POINTER(Match)), ("matches_cap", ctypes.c_uint64),
                ("matches_counts", ctypes.POINTER(ctypes.c_uint64)), ("topk", ctypes.POINTER(Match)),
                ("topk_counts", ctypes.POINTER(ctypes.c_uint32)), ("bins", ctypes.POINTER(ctypes.c_uint64)),
                ("invalid", ctypes.POINTER(ctypes.c_uint64))]


class BatchReportResult:
    """What TemplateBatchEngine.report() returns, per query; the fields of a part that was not asked
    for are None.  matches[q] and topk[q] are lists of Match that view the arrays the call filled."""

    __slots__ = ("matches", "matches_counts", "topk", "bins", "invalid")

    def __init__(self):
        self.matches = self.matches_counts = self.topk = self.bins = self.invalid = None

    def __repr__(self):
        return (f"BatchReportResult(matches_counts={self.matches_counts}, "
                f"topk={None if self.topk is None else len(self.topk)}, "
                f"bins={None if self.bins is None else self.bins.shape}, invalid={self.invalid})")


def _report(call, owner, threshold, cap, k, nbins, rematch):
    """One report call (iris_template_report, iris_resolver_report, iris_resolver_report_masks):
    fills a Report from the arguments that are not None, runs call(pointer to it) and collects the
    selected parts -> ReportResult.  cap None returns every match: the first call has room for 1024
    records (or what `owner` remembers of its last list) and a longer list comes from
    rematch(count), the sibling call with room for all of them."""
    r = Report()
    res = ReportResult()
    marr = tarr = None  # the arrays the struct points at; the returned records are views into them
    want_all = False
    if threshold is not None:
        r.parts |= REPORT_MATCHES
        r.threshold = float(threshold)
        want_all = cap is None
        room = max(1024, getattr(owner, "_match_room", 0)) if want_all else int(cap)
        r.matches_cap = room
        if room:
            marr = (Match * room)()
            r.matches = marr
    if k is not None:
        r.parts |= REPORT_TOPK
        r.k = int(k)
        tarr = (Match * (max(1, min(int(k), TOPK_MAX)) if int(k) > 0 else 1))()
        r.topk = tarr
    if nbins is not None:
        nb = int(nbins)
        r.parts |= REPORT_HIST
        r.nbins = nb
        res.bins = np.zeros(nb if 0 < nb <= HIST_MAX_BINS else 1, np.uint64)
        r.bins = res.bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    _check(call(ctypes.byref(r)))
    if threshold is not None:
        res.matches_count = int(r.matches_count)
        if want_all and res.matches_count > r.matches_cap:  # the rest of a longer list: the sibling's pass
            res.matches = rematch(res.matches_count)
        else:
            res.matches = [marr[i] for i in range(min(res.matches_count, r.matches_cap))]
        if want_all:
            owner._match_room = min(res.matches_count + res.matches_count // 4, 1 << 22)
    if k is not None:
        res.topk = [tarr[i] for i in range(r.topk_count)]
    if nbins is not None:
        res.invalid = int(r.invalid)
    return res


_lib = None
_lock = threading.Lock()


def load_library(path=None):
    """Load libiris_hip.so (fails loudly when it is absent)."""
    global _lib
    if _lib is not None and path is None:  # per-call fast path: no lock once loaded
        return _lib
    with _lock:
        if _lib is not None and path is None:
            return _lib
        p = pathlib.Path(path) if path else LIB_PATH
        if not p.exists():
            raise IrisError(-4, f"{p} not built: run `make -C {HERE}` (or __graft_entry__.build())")
        lib = ctypes.CDLL(str(p))
        P, u64, i32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int32
        PP = ctypes.POINTER(ctypes.c_void_p)
        sig = {
            "iris_last_error": ([], ctypes.c_char_p),
            "iris_version": ([], ctypes.c_char_p),
            "iris_config": ([P, ctypes.c_char_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
            "iris_device_count": ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
            "iris_device_open": ([ctypes.c_int, PP], ctypes.c_int),
            "iris_device_close": ([P], ctypes.c_int),
            "iris_device_synchronize": ([P], ctypes.c_int),
            "iris_device_stream": ([P, PP], ctypes.c_int),
            "iris_device_memory": ([P, ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)],
                                   ctypes.c_int),
            "iris_template_search_async": ([P, P, u64, u64, u64, PP], ctypes.c_int),
            "iris_pending_wait": ([P, ctypes.POINTER(Match)], ctypes.c_int),
            "iris_device_set_profiling": ([P, ctypes.c_int], ctypes.c_int),
            "iris_device_kernel_stats": ([P, ctypes.c_char_p, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double),
                                          ctypes.POINTER(u64)], ctypes.c_int),
            "iris_device_reset_stats": ([P], ctypes.c_int),
            "iris_device_alloc": ([P, ctypes.c_size_t, PP], ctypes.c_int),
            "iris_device_free": ([P, P], ctypes.c_int),
            "iris_device_drop_resident": ([P], ctypes.c_int),
            "iris_device_drop_resident_range": ([P, P], ctypes.c_int),
            "iris_device_kernel_stats_largest": ([P, ctypes.c_char_p, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double)],
                                                 ctypes.c_int),
            "iris_memcpy_d2h": ([P, P, P, ctypes.c_size_t], ctypes.c_int),
            "iris_db_create": ([P, ctypes.c_int, u64, PP], ctypes.c_int),
            "iris_db_create_ex": ([P, ctypes.c_int, u64, ctypes.c_int, PP], ctypes.c_int),
            "iris_db_layout": ([P, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
            "iris_db_destroy": ([P], ctypes.c_int),
            "iris_db_len": ([P, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_db_capacity": ([P, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_db_kind": ([P, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
            "iris_db_append": ([P, P, u64], ctypes.c_int),
            "iris_db_write": ([P, u64, P, u64], ctypes.c_int),
            "iris_db_read": ([P, u64, u64, P], ctypes.c_int),
            "iris_db_generate": ([P, u64, u64, u64], ctypes.c_int),
            "iris_db_clear": ([P], ctypes.c_int),
            "iris_db_truncate": ([P, u64], ctypes.c_int),
            "iris_memcpy_h2d": ([P, P, P, ctypes.c_size_t], ctypes.c_int),
            "iris_db_load_file": ([P, ctypes.c_char_p, u64, u64, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_db_save_file": ([P, ctypes.c_char_p, u64, u64], ctypes.c_int),
            "iris_templates_read_json": ([ctypes.c_char_p, P, u64, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_templates_write_json": ([ctypes.c_char_p, P, u64], ctypes.c_int),
            "iris_resolver_search_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, P, ctypes.POINTER(Match)],
                                           ctypes.c_int),
            "iris_resolver_search_masks_host": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.POINTER(Match)],
                                                ctypes.c_int),
            "iris_prepare_shares": ([P, u64, u64, u64, P, u64, ctypes.c_uint32, ctypes.c_uint32, P, P], ctypes.c_int),
            "iris_masks_engine_new": ([P, P, PP], ctypes.c_int),
            "iris_distance_engine_new": ([P, P, PP], ctypes.c_int),
            "iris_template_engine_new": ([P, P, PP], ctypes.c_int),
            "iris_engine_destroy": ([P], ctypes.c_int),
            "iris_engine_batch_process": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_engine_batch_process_host": ([P, P, u64, P], ctypes.c_int),
            "iris_engine_batch_process_device": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_template_counts": ([P, P, u64, u64, P, P], ctypes.c_int),
            "iris_template_distances": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_template_search": ([P, P, u64, u64, u64, P, ctypes.POINTER(Match)], ctypes.c_int),
            "iris_template_batch_engine_new": ([P, P, ctypes.c_uint32, PP], ctypes.c_int),
            "iris_template_batch_search": ([P, P, u64, u64, u64, ctypes.POINTER(Match)], ctypes.c_int),
            "iris_distance_batch_engine_new": ([P, P, ctypes.c_uint32, PP], ctypes.c_int),
            "iris_distance_batch_process": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_distance_batch_process_device": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_masks_batch_engine_new": ([P, P, ctypes.c_uint32, PP], ctypes.c_int),
            "iris_masks_batch_process": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_masks_batch_process_device": ([P, P, u64, u64, P], ctypes.c_int),
            "iris_resolver_batch_search_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, P, ctypes.POINTER(Match)],
                                                 ctypes.c_int),
            "iris_resolver_search": ([P, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, P, u64, u64, P,
                                      ctypes.POINTER(Match)], ctypes.c_int),
            "iris_resolver_search_host": ([P, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, P, u64, u64,
                                           ctypes.POINTER(Match)], ctypes.c_int),
            "iris_dot_bool_batch": ([P, P, u64, P, u64, P], ctypes.c_int),
            "iris_dot_u16_batch": ([P, P, u64, P, u64, P], ctypes.c_int),
            "iris_bits_rotated": ([P, i32, P], ctypes.c_int),
            "iris_encoded_rotated": ([P, i32, P], ctypes.c_int),
            "iris_encode": ([P, P], ctypes.c_int),
            "iris_decode_distance": ([P, P, ctypes.POINTER(ctypes.c_double)], ctypes.c_int),
            "iris_match_merge": ([ctypes.POINTER(Match), u64, ctypes.POINTER(Match)], ctypes.c_int),
            "iris_template_matches": ([P, P, u64, u64, u64, ctypes.c_double, ctypes.POINTER(Match), u64,
                                       ctypes.POINTER(u64)], ctypes.c_int),
            "iris_template_matches_async": ([P, P, u64, u64, u64, ctypes.c_double, u64, PP], ctypes.c_int),
            "iris_pending_matches_wait": ([P, ctypes.POINTER(Match), ctypes.POINTER(u64)], ctypes.c_int),
            "iris_resolver_matches": ([P, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, P, u64, u64, ctypes.c_double,
                                       ctypes.POINTER(Match), u64, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_resolver_matches_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.c_double,
                                             ctypes.POINTER(Match), u64, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_resolver_batch_matches_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.c_double,
                                                   ctypes.POINTER(Match), u64, ctypes.POINTER(u64)], ctypes.c_int),
            "iris_template_batch_matches": ([P, P, u64, u64, u64, ctypes.c_double, ctypes.POINTER(Match), u64,
                                             ctypes.POINTER(u64)], ctypes.c_int),
            "iris_template_topk": ([P, P, u64, u64, u64, ctypes.c_uint32, ctypes.POINTER(Match),
                                    ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_template_topk_async": ([P, P, u64, u64, u64, ctypes.c_uint32, PP], ctypes.c_int),
            "iris_pending_topk_wait": ([P, ctypes.POINTER(Match), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_resolver_topk": ([P, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, P, u64, u64, ctypes.c_uint32,
                                    ctypes.POINTER(Match), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_resolver_topk_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.c_uint32,
                                          ctypes.POINTER(Match), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_resolver_batch_topk_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.c_uint32,
                                                ctypes.POINTER(Match), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_template_batch_topk": ([P, P, u64, u64, u64, ctypes.c_uint32, ctypes.POINTER(Match),
                                          ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_topk_merge": ([ctypes.POINTER(Match), u64, ctypes.c_uint32, ctypes.POINTER(Match),
                                 ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_template_histogram": ([P, P, u64, u64, ctypes.c_uint32, P, P], ctypes.c_int),
            "iris_template_batch_histogram": ([P, P, u64, u64, ctypes.c_uint32, P, P], ctypes.c_int),
            "iris_template_report": ([P, P, u64, u64, u64, ctypes.POINTER(Report)], ctypes.c_int),
            "iris_template_report_async": ([P, P, u64, u64, u64, ctypes.POINTER(Report), PP], ctypes.c_int),
            "iris_pending_report_wait": ([P, ctypes.POINTER(Report)], ctypes.c_int),
            "iris_template_batch_report": ([P, P, u64, u64, u64, ctypes.POINTER(BatchReport)], ctypes.c_int),
            "iris_resolver_batch_report_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.POINTER(BatchReport)], ctypes.c_int),
            "iris_resolver_report": ([P, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, P, u64, u64, ctypes.POINTER(Report)],
                                     ctypes.c_int),
            "iris_resolver_report_masks": ([P, P, u64, u64, P, ctypes.c_uint32, u64, ctypes.POINTER(Report)], ctypes.c_int),
            "iris_resolver_histogram": ([P, ctypes.POINTER(ctypes.c_void_p), ctypes.c_uint32, P, u64, ctypes.c_uint32, P, P],
                                        ctypes.c_int),
            "iris_resolver_histogram_masks": ([P, P, u64, u64, P, ctypes.c_uint32, ctypes.c_uint32, P, P], ctypes.c_int),
            "iris_resolver_batch_histogram_masks": ([P, P, u64, u64, P, ctypes.c_uint32, ctypes.c_uint32, P, P], ctypes.c_int),
            "iris_query_table_sizes": ([ctypes.c_int, ctypes.c_uint32, ctypes.POINTER(ctypes.c_size_t),
                                        ctypes.POINTER(ctypes.c_size_t)], ctypes.c_int),
            "iris_engine_query_tables": ([P, P, ctypes.c_size_t, P, ctypes.c_size_t], ctypes.c_int),
            "iris_host_query_tables": ([ctypes.c_int, P, ctypes.c_uint32, P, ctypes.c_size_t, P, ctypes.c_size_t],
                                       ctypes.c_int),
            "iris_db_attach_host": ([P, P, u64, ctypes.c_int], ctypes.c_int),
            "iris_db_detach_host": ([P], ctypes.c_int),
            "iris_group_create": ([ctypes.POINTER(ctypes.c_int), ctypes.c_uint32, PP], ctypes.c_int),
            "iris_group_unique_id": ([P], ctypes.c_int),
            "iris_group_create_rank": ([ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, P, PP], ctypes.c_int),
            "iris_group_destroy": ([P], ctypes.c_int),
            "iris_group_set_timeout": ([P, ctypes.c_uint32], ctypes.c_int),
            "iris_group_info": ([P, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32),
                                 ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_group_device": ([P, ctypes.c_uint32, PP], ctypes.c_int),
            "iris_group_rccl_info": ([P, ctypes.POINTER(ctypes.c_uint32), ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
            "iris_group_db_create": ([P, ctypes.c_int, u64, ctypes.c_int, ctypes.c_uint32, PP], ctypes.c_int),
            "iris_group_db_destroy": ([P], ctypes.c_int),
            "iris_group_db_info": ([P, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_uint32),
                                    ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], ctypes.c_int),
            "iris_group_db_shard": ([P, ctypes.c_uint32, PP, ctypes.POINTER(u64), ctypes.POINTER(u64)], ctypes.c_int),
            "iris_group_db_generate": ([P, u64], ctypes.c_int),
            "iris_group_db_write": ([P, u64, P, u64], ctypes.c_int),
            "iris_group_db_read": ([P, u64, u64, P], ctypes.c_int),
            "iris_group_db_load_file": ([P, ctypes.c_char_p, u64], ctypes.c_int),
            "iris_group_template_search": ([P, P, ctypes.POINTER(Match)], ctypes.c_int),
            "iris_group_template_search_async": ([P, P, PP], ctypes.c_int),
            "iris_group_pending_wait": ([P, ctypes.POINTER(Match)], ctypes.c_int),
            "iris_group_template_batch_search": ([P, P, ctypes.c_uint32, ctypes.POINTER(Match)], ctypes.c_int),
        }
        for name, (args, res) in sig.items():
            if "IRIS_HIP_LIB" in os.environ and not hasattr(lib, name):
                continue  # an older build measured beside this one: it lacks the newer entry points
            f = getattr(lib, name)
            f.argtypes = args
            f.restype = res
        if path is None:
            _lib = lib
        return lib


def exported_symbols():
    return [
        "iris_last_error", "iris_version", "iris_config", "iris_device_count", "iris_device_open", "iris_device_close",
        "iris_device_synchronize", "iris_device_stream", "iris_device_set_profiling", "iris_device_kernel_stats",
        "iris_device_reset_stats", "iris_device_alloc", "iris_device_free", "iris_device_drop_resident",
        "iris_device_drop_resident_range", "iris_device_kernel_stats_largest",
        "iris_memcpy_d2h", "iris_db_create",
        "iris_db_create_ex", "iris_db_layout",
        "iris_db_destroy", "iris_db_len", "iris_db_capacity", "iris_db_kind", "iris_db_append", "iris_db_write",
        "iris_db_read", "iris_db_generate", "iris_db_clear", "iris_masks_engine_new", "iris_distance_engine_new",
        "iris_template_engine_new", "iris_engine_destroy", "iris_engine_batch_process",
        "iris_engine_batch_process_host", "iris_engine_batch_process_device", "iris_template_counts", "iris_template_distances", "iris_template_search",
        "iris_template_batch_engine_new", "iris_template_batch_search", "iris_resolver_search",
        "iris_resolver_search_host", "iris_dot_bool_batch", "iris_dot_u16_batch", "iris_bits_rotated", "iris_encoded_rotated", "iris_encode",
        "iris_decode_distance", "iris_match_merge", "iris_db_load_file", "iris_db_save_file",
        "iris_templates_read_json", "iris_templates_write_json", "iris_prepare_shares",
        "iris_db_truncate", "iris_memcpy_h2d", "iris_resolver_search_masks", "iris_resolver_search_masks_host",
        "iris_query_table_sizes", "iris_engine_query_tables", "iris_host_query_tables", "iris_device_memory",
        "iris_template_search_async", "iris_pending_wait",
        "iris_db_attach_host", "iris_db_detach_host",
        "iris_group_create", "iris_group_unique_id", "iris_group_create_rank", "iris_group_destroy", "iris_group_set_timeout", "iris_group_info",
        "iris_group_device", "iris_group_rccl_info", "iris_group_db_create", "iris_group_db_destroy", "iris_group_db_info",
        "iris_group_db_shard", "iris_group_db_generate", "iris_group_db_write", "iris_group_db_read",
        "iris_group_db_load_file", "iris_group_template_search", "iris_group_template_search_async",
        "iris_group_pending_wait", "iris_group_template_batch_search",
        "iris_distance_batch_engine_new", "iris_distance_batch_process", "iris_distance_batch_process_device",
        "iris_masks_batch_engine_new", "iris_masks_batch_process", "iris_masks_batch_process_device",
        "iris_resolver_batch_search_masks",
        "iris_template_matches", "iris_resolver_matches", "iris_resolver_matches_masks",
        "iris_resolver_batch_matches_masks", "iris_template_batch_matches",
        "iris_template_matches_async", "iris_pending_matches_wait",
        "iris_template_topk_async", "iris_pending_topk_wait",
        "iris_template_topk", "iris_resolver_topk", "iris_resolver_topk_masks", "iris_topk_merge",
        "iris_resolver_batch_topk_masks", "iris_template_batch_topk",
        "iris_template_histogram", "iris_template_batch_histogram",
        "iris_resolver_histogram", "iris_resolver_histogram_masks", "iris_resolver_batch_histogram_masks",
        "iris_template_report_async", "iris_pending_report_wait",
        "iris_template_report", "iris_resolver_report", "iris_resolver_report_masks", "iris_template_batch_report", "iris_resolver_batch_report_masks",
    ]


def query_table_sizes(kind, nq=0):
    """(table bytes, fragment bytes) of an engine's rotated-query tables."""
    tb, fb = ctypes.c_size_t(), ctypes.c_size_t()
    _check(load_library().iris_query_table_sizes(int(kind), int(nq), ctypes.byref(tb), ctypes.byref(fb)))
    return tb.value, fb.value


def host_query_tables(kind, query, nq=0):
    """The rotated-query table and MFMA fragments of `query` built by the host reference
    builders (CPU only) -> (table uint8 array, fragments uint8 array)."""
    tb, fb = query_table_sizes(kind, nq)
    q = np.ascontiguousarray(query)
    tab, frag = np.zeros(tb, np.uint8), np.zeros(fb, np.uint8)
    _check(load_library().iris_host_query_tables(int(kind), _ptr(q), int(nq), _ptr(tab) if tb else None, tb,
                                                 _ptr(frag), fb))
    return tab, frag


def read_templates_json(path):
    """JSON array of {"pattern": hex, "mask": hex} (src/bits.rs:74-93) -> uint64 [n, 400]
    (pattern limbs then mask limbs, the Template byte layout)."""
    lib = load_library()
    n = ctypes.c_uint64(0)
    _check(lib.iris_templates_read_json(os.fsencode(path), None, 0, ctypes.byref(n)))
    out = np.zeros((n.value, 2 * LIMBS), np.uint64)
    if n.value:
        _check(lib.iris_templates_read_json(os.fsencode(path), _ptr(out), n.value, ctypes.byref(n)))
    return out


def write_templates_json(path, templates):
    """Inverse of read_templates_json (compact JSON, lowercase hex)."""
    a = np.ascontiguousarray(np.asarray(templates, np.uint64).reshape(-1, 2 * LIMBS))
    _check(load_library().iris_templates_write_json(os.fsencode(path), _ptr(a), a.shape[0]))


def prepare_shares(templates, shares, masks=None, key=None, nonce=0, first=0, n=None, index_base=0, rounds=12):
    """`prepare` on the device (src/main.rs:333-361): appends EncodedBits::share(len(shares))
    of encode(templates[first:first+n]) to the share Databases and, optionally, the masks to
    a masks Database.  key: 32 bytes (default: os.urandom, a CSPRNG).  rounds: ChaCha8/12/20;
    12 is the reference's generator (rand 0.8.5 thread_rng = ChaCha12).  Returns the key."""
    if key is None:
        key = os.urandom(32)
    key = bytes(key)
    if len(key) != 32:
        raise ValueError("key must be 32 bytes")
    if n is None:
        n = len(templates) - int(first)
    kbuf = (ctypes.c_uint8 * 32).from_buffer_copy(key)
    arr = (ctypes.c_void_p * len(shares))(*[s.handle for s in shares])
    _check(load_library().iris_prepare_shares(templates.handle, int(first), int(n), int(index_base), kbuf,
                                              int(nonce), int(rounds), len(shares), arr,
                                              masks.handle if masks is not None else None))
    return key


def _check(rc):
    if rc != 0:
        raise IrisError(rc, load_library().iris_last_error().decode(errors="replace"))


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


# ====================================================================== value types


def _collect_matches(call, cap, out, owner=None):
    """Runs one iris_*_matches call -> (list[Match], count).  call(out_ptr, cap, count_ref) -> rc.
    out: a (Match * cap) ctypes array filled in place (entries past the matches stay untouched), or
    None.  cap=None asks for every match: a first call with room for 1024 -- or for a quarter more
    than `owner`'s last such call reported, so a caller with a steady list length makes one call --
    and one more with room for the reported count if there are more; cap=0 with out=None only counts."""
    count = ctypes.c_uint64()
    if out is not None:
        cap = len(out) if cap is None else int(cap)
        if cap > len(out):
            raise IrisError(-1, "cap exceeds len(out)")
        _check(call(out, cap, ctypes.byref(count)))
        return [out[i] for i in range(min(cap, count.value))], count.value
    want_all = cap is None
    cap = max(1024, getattr(owner, "_match_room", 0)) if want_all else int(cap)
    buf = (Match * cap)() if cap else None
    _check(call(buf, cap, ctypes.byref(count)))
    if want_all and count.value > cap:
        cap = count.value
        buf = (Match * cap)()
        _check(call(buf, cap, ctypes.byref(count)))
    if want_all and owner is not None:
        owner._match_room = min(count.value + count.value // 4, 1 << 22)
    return [buf[i] for i in range(min(cap, count.value))], count.value


class Bits:
    """12 800-bit vector, `[u64; 200]` (src/bits.rs:13-15)."""

    __slots__ = ("limbs",)

    def __init__(self, limbs=None):
        self.limbs = np.zeros(LIMBS, np.uint64) if limbs is None else _c(limbs, np.uint64).reshape(LIMBS).copy()

    @classmethod
    def random(cls, rng):
        return cls(rng.integers(0, 2**64, LIMBS, dtype=np.uint64))

    def __getitem__(self, i):  # Index<usize> (src/bits.rs:44-57)
        if not 0 <= i < BITS:
            raise IndexError(i)
        return bool((int(self.limbs[i // 64]) >> (i % 64)) & 1)

    def __eq__(self, other):
        return isinstance(other, Bits) and bool((self.limbs == other.limbs).all())

    def rotated(self, amount):
        out = np.empty(LIMBS, np.uint64)
        _check(load_library().iris_bits_rotated(_ptr(self.limbs), int(amount), _ptr(out)))
        return Bits(out)

    def count_ones(self):
        return int(np.unpackbits(self.limbs.view(np.uint8)).sum())

    def __and__(self, other):
        return Bits(self.limbs & other.limbs)

    def __or__(self, other):
        return Bits(self.limbs | other.limbs)

    def __xor__(self, other):
        return Bits(self.limbs ^ other.limbs)

    def __invert__(self):
        return Bits(~self.limbs)

    def dot(self, other):  # Bits::dot -> arch::dot_bool (src/bits.rs:35-37)
        return dot_bool(self, other)

    def to_hex(self):  # serde: hex of the LE bytes (src/bits.rs:74-81)
        return self.limbs.astype("<u8").tobytes().hex()

    @classmethod
    def from_hex(cls, s):
        b = bytes.fromhex(s)
        if len(b) != 1600:
            raise ValueError("expected 1600 bytes")
        return cls(np.frombuffer(b, "<u8"))


class EncodedBits:
    """`[u16; 12800]` ring vector (src/encoded_bits.rs:13-15)."""

    __slots__ = ("values",)

    def __init__(self, values=None):
        self.values = np.zeros(BITS, np.uint16) if values is None else _c(values, np.uint16).reshape(BITS).copy()

    @classmethod
    def random(cls, rng):
        return cls(rng.integers(0, 2**16, BITS, dtype=np.uint16))

    @classmethod
    def from_bits(cls, bits):  # From<&Bits> (src/encoded_bits.rs:75-79)
        return cls(np.unpackbits(bits.limbs.view(np.uint8), bitorder="little").astype(np.uint16))

    def __eq__(self, other):
        return isinstance(other, EncodedBits) and bool((self.values == other.values).all())

    def rotated(self, amount):
        out = np.empty(BITS, np.uint16)
        _check(load_library().iris_encoded_rotated(_ptr(self.values), int(amount), _ptr(out)))
        return EncodedBits(out)

    def sum(self):
        return int(self.values.astype(np.uint64).sum() & 0xFFFF)

    def __add__(self, other):
        return EncodedBits(self.values + other.values)

    def __sub__(self, other):
        return EncodedBits(self.values - other.values)

    def __mul__(self, other):
        return EncodedBits(self.values * other.values)

    def __neg__(self):
        return EncodedBits(np.uint16(0) - self.values)

    def dot(self, other):  # EncodedBits::dot -> arch::dot_u16 (src/encoded_bits.rs:64-66)
        return dot_u16(self, other)

    def share(self, n, rng):
        """n additive shares mod 2^16 (src/encoded_bits.rs:23-38); host-side offline prep."""
        assert n > 0
        shares = [EncodedBits.random(rng) for _ in range(n - 1)]
        acc = np.zeros(BITS, np.uint16)
        for s in shares:
            acc = acc + s.values
        shares.append(EncodedBits(self.values - acc))
        return shares


class Template:
    """`#[repr(C)] { pattern: Bits, mask: Bits }` (src/template.rs:11-29)."""

    __slots__ = ("pattern", "mask")

    def __init__(self, pattern=None, mask=None):
        self.pattern = pattern if isinstance(pattern, Bits) else Bits(pattern)
        self.mask = mask if isinstance(mask, Bits) else Bits(mask)

    @classmethod
    def random(cls, rng):
        return cls(Bits.random(rng), Bits.random(rng))

    @classmethod
    def from_array(cls, a):
        a = _c(a, np.uint64).reshape(2 * LIMBS)
        return cls(a[:LIMBS], a[LIMBS:])

    def to_array(self):
        return np.concatenate([self.pattern.limbs, self.mask.limbs])

    def rotated(self, amount):
        return Template(self.pattern.rotated(amount), self.mask.rotated(amount))

    def __eq__(self, other):
        return isinstance(other, Template) and self.pattern == other.pattern and self.mask == other.mask

    def distance(self, other, device=None):
        """Template::distance (src/template.rs:43-47), on the GPU."""
        dev = device or default_device()
        with TemplateEngine(dev, self) as eng:
            return float(eng.distances_host(other.to_array()[None, :])[0])


def encode(template):
    """encode(&Template) -> EncodedBits (src/lib.rs:16-26)."""
    t = template.to_array() if isinstance(template, Template) else _c(template, np.uint64)
    out = np.empty(BITS, np.uint16)
    _check(load_library().iris_encode(_ptr(_c(t, np.uint64)), _ptr(out)))
    return EncodedBits(out)


def decode_distance(distances, denominators):
    """decode_distance(&[u16;31], &[u16;31]) -> f64 (src/lib.rs:97-107)."""
    out = ctypes.c_double()
    _check(load_library().iris_decode_distance(_ptr(_c(distances, np.uint16)), _ptr(_c(denominators, np.uint16)),
                                               ctypes.byref(out)))
    return out.value


TOPK_MAX = 64  # IRIS_TOPK_MAX
HIST_MAX_BINS = 1024  # IRIS_HIST_MAX_BINS


def _collect_topk(call, k):
    """Runs call(out, count) on a k-entry array -> the listed entries as a list of Match."""
    room = max(1, min(int(k), TOPK_MAX)) if int(k) > 0 else 1
    arr = (Match * room)()
    cnt = ctypes.c_uint32(0)
    _check(call(arr, ctypes.byref(cnt)))
    return [_copy_match(arr[i]) for i in range(cnt.value)]


def _copy_match(m):
    c = Match()
    ctypes.memmove(ctypes.byref(c), ctypes.byref(m), ctypes.sizeof(Match))
    return c


def merge_topk(matches, k):
    """Merges top-k lists that carry global indices (shards, chunks, GPUs) into the k best, best
    first (iris_topk_merge; host only) -> list[Match]."""
    matches = list(matches)
    arr = (Match * max(1, len(matches)))(*matches)
    return _collect_topk(lambda o, cnt: load_library().iris_topk_merge(arr, len(matches), int(k), o, cnt), k)


def merge_matches(matches):
    """Cross-shard argmin merge (src/main.rs:616-621 semantics)."""
    arr = (Match * max(1, len(matches)))(*matches) if matches else (Match * 1)()
    out = Match()
    _check(load_library().iris_match_merge(arr, len(matches), ctypes.byref(out)))
    return out


# ====================================================================== devices / databases


class Device:
    """One HIP device (gfx950) and its stream."""

    def __init__(self, ordinal=0):
        lib = load_library()
        h = ctypes.c_void_p()
        _check(lib.iris_device_open(int(ordinal), ctypes.byref(h)))
        self.handle = h
        self.ordinal = ordinal

    @staticmethod
    def count():
        n = ctypes.c_int()
        _check(load_library().iris_device_count(ctypes.byref(n)))
        return n.value

    def close(self):
        if self.handle:
            load_library().iris_device_close(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        _check(load_library().iris_device_synchronize(self.handle))

    def config(self):
        """The environment knobs this device read when it opened (iris_config), as a dict."""
        return config(self)

    def memory(self):
        """(free, total) device memory in bytes."""
        f, t = ctypes.c_size_t(), ctypes.c_size_t()
        _check(load_library().iris_device_memory(self.handle, ctypes.byref(f), ctypes.byref(t)))
        return f.value, t.value

    def resident(self):
        """(count, bytes) of the record-file copies this device keeps resident for host-slice calls."""
        c, b = self.config()["resident"].split("/")
        return int(c), int(b)

    def drop_resident(self):
        """Frees the device's resident record-file copies (iris_device_drop_resident)."""
        _check(load_library().iris_device_drop_resident(self.handle))

    def drop_resident_range(self, array):
        """Frees the resident copy of the file mapping that holds `array`'s first byte
        (iris_device_drop_resident_range): after changing the file through a writable mapping."""
        a = np.asarray(array)
        _check(load_library().iris_device_drop_resident_range(self.handle, ctypes.c_void_p(a.ctypes.data)))

    def stream(self):
        s = ctypes.c_void_p()
        _check(load_library().iris_device_stream(self.handle, ctypes.byref(s)))
        return s.value

    def set_profiling(self, enabled=True):
        _check(load_library().iris_device_set_profiling(self.handle, 1 if enabled else 0))

    def reset_stats(self):
        _check(load_library().iris_device_reset_stats(self.handle))

    def kernel_stats(self, name):
        """-> (launches, total_ms, items) recorded with HIP events on the device stream."""
        l, ms, it = ctypes.c_uint64(), ctypes.c_double(), ctypes.c_uint64()
        _check(load_library().iris_device_kernel_stats(self.handle, name.encode(), ctypes.byref(l), ctypes.byref(ms),
                                                        ctypes.byref(it)))
        return l.value, ms.value, it.value

    def kernel_stats_largest(self, name):
        """-> (items, ms) of the largest launch of the kernel family since the last reset."""
        it, ms = ctypes.c_uint64(), ctypes.c_double()
        _check(load_library().iris_device_kernel_stats_largest(self.handle, name.encode(), ctypes.byref(it),
                                                                ctypes.byref(ms)))
        return it.value, ms.value

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        _check(load_library().iris_device_alloc(self.handle, int(nbytes), ctypes.byref(p)))
        return p.value

    def free(self, ptr):
        _check(load_library().iris_device_free(self.handle, ctypes.c_void_p(ptr)))

    def d2h(self, host_array, device_ptr):
        _check(load_library().iris_memcpy_d2h(self.handle, _ptr(host_array), ctypes.c_void_p(device_ptr),
                                               host_array.nbytes))

    def h2d(self, device_ptr, host_array):
        a = np.ascontiguousarray(host_array)
        _check(load_library().iris_memcpy_h2d(self.handle, ctypes.c_void_p(device_ptr), _ptr(a), a.nbytes))


def config(device=None):
    """iris_config as a dict: the knobs of `device`, or (None) those a device opened now would get.
    Test-only hooks set without IRIS_TEST_HOOKS=1 appear under "ignored" (a list)."""
    lib = load_library()
    h = device.handle if device is not None else None
    need = ctypes.c_size_t()
    _check(lib.iris_config(h, None, 0, ctypes.byref(need)))
    buf = ctypes.create_string_buffer(need.value + 1)
    _check(lib.iris_config(h, buf, len(buf), None))
    out = {}
    for kv in buf.value.decode().split():
        k, v = kv.split("=", 1)
        out[k] = v.split(",") if k == "ignored" else v
    return out


_default = None


def default_device():
    global _default
    if _default is None:
        _default = Device(0)
    return _default


def _records(kind, records):
    dt, width = _REC_DTYPE[kind]
    if isinstance(records, (Bits, EncodedBits, Template)):
        records = [records]
    if isinstance(records, (list, tuple)):
        rows = []
        for r in records:
            if isinstance(r, Bits):
                rows.append(r.limbs)
            elif isinstance(r, EncodedBits):
                rows.append(r.values)
            elif isinstance(r, Template):
                rows.append(r.to_array())
            else:
                rows.append(np.asarray(r))
        records = np.stack(rows) if rows else np.zeros((0, width), dt)
    a = _c(records, dt)
    if a.ndim == 1:
        a = a.reshape(1, -1)
    if a.shape[-1] != width:
        raise IrisError(-1, f"records must have {width} {np.dtype(dt).name} per row, got shape {a.shape}")
    return a


class Database:
    """Device-resident database (replaces the reference's mmap'd share/masks files)."""

    def __init__(self, device, kind, capacity, layout=LAYOUT_DEFAULT):
        self.device = device
        self.kind = kind
        h = ctypes.c_void_p()
        _check(load_library().iris_db_create_ex(device.handle, int(kind), int(capacity), int(layout),
                                                ctypes.byref(h)))
        self.handle = h

    @property
    def layout(self):
        v = ctypes.c_int()
        _check(load_library().iris_db_layout(self.handle, ctypes.byref(v)))
        return v.value

    def close(self):
        if self.handle:
            self._release_attached()
            load_library().iris_db_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _release_attached(self):
        # every change of the records ends the attachment in the library: the host array is
        # writable again (if it was before attach_host)
        a = getattr(self, "_attached", None)
        if a is not None and getattr(self, "_attached_writable", False):
            a.setflags(write=True)
        self._attached = None

    def __len__(self):
        n = ctypes.c_uint64()
        _check(load_library().iris_db_len(self.handle, ctypes.byref(n)))
        return n.value

    @property
    def capacity(self):
        n = ctypes.c_uint64()
        _check(load_library().iris_db_capacity(self.handle, ctypes.byref(n)))
        return n.value

    def append(self, records):
        a = _records(self.kind, records)
        self._release_attached()
        _check(load_library().iris_db_append(self.handle, _ptr(a), a.shape[0]))

    def write(self, index, records):
        a = _records(self.kind, records)
        self._release_attached()
        _check(load_library().iris_db_write(self.handle, int(index), _ptr(a), a.shape[0]))

    def read(self, first, n):
        dt, width = _REC_DTYPE[self.kind]
        out = np.empty((n, width), dt)
        _check(load_library().iris_db_read(self.handle, int(first), int(n), _ptr(out)))
        return out

    def generate(self, n, seed, global_index0=None):
        """Append n synthetic records; generator index defaults to the DB position."""
        g0 = len(self) if global_index0 is None else global_index0
        self._release_attached()
        _check(load_library().iris_db_generate(self.handle, int(n), int(seed), int(g0)))

    def clear(self):
        self._release_attached()
        _check(load_library().iris_db_clear(self.handle))

    def truncate(self, n):
        if int(n) != len(self):
            self._release_attached()
        _check(load_library().iris_db_truncate(self.handle, int(n)))

    def load_file(self, path, first=0, count=None):
        """Appends records [first, first+count) of a raw record file (.masks / .share-i /
        raw templates; src/main.rs:386-400,455-469).  Returns the number appended."""
        got = ctypes.c_uint64(0)
        cnt = (1 << 64) - 1 if count is None else int(count)
        self._release_attached()
        _check(load_library().iris_db_load_file(self.handle, os.fsencode(path), int(first), cnt,
                                                ctypes.byref(got)))
        return got.value

    def save_file(self, path, first=0, n=None):
        """Writes records [first, first+n) to a raw record file."""
        if n is None:
            n = len(self) - int(first)
        _check(load_library().iris_db_save_file(self.handle, os.fsencode(path), int(first), int(n)))

    def attach_host(self, host, upload=True):
        """Declares this database the resident copy of the host record array `host` (e.g. a
        memory-mapped record file, src/main.rs:389-391,458-460): upload=True fills the (empty)
        database from it; upload=False checks it already holds them.  Engine batch_process
        calls on slices (numpy views) of `host` then run on the device copy without an
        upload.  Keeps a reference to `host` while attached and makes that array read-only
        until the attachment ends (detach_host, or any write to the database): the device copy
        would not see a change (other views of the same memory are not locked -- the rows must
        stay unchanged while attached, as include/iris_hip.h says)."""
        a = host if isinstance(host, np.ndarray) else np.asarray(host)
        dt, width = _REC_DTYPE[self.kind]
        if a.dtype != dt or a.ndim != 2 or a.shape[1] != width or not a.flags["C_CONTIGUOUS"]:
            raise IrisError(-1, f"host must be a C-contiguous [n, {width}] {np.dtype(dt).name} array")
        self._release_attached()
        _check(load_library().iris_db_attach_host(self.handle, _ptr(a), a.shape[0], 1 if upload else 0))
        self._attached = a
        self._attached_writable = bool(a.flags.writeable)
        if self._attached_writable:
            a.setflags(write=False)

    def detach_host(self):
        _check(load_library().iris_db_detach_host(self.handle))
        self._release_attached()


# ====================================================================== engines


class _Engine:
    kind = 0

    def close(self):
        if getattr(self, "handle", None):
            load_library().iris_engine_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def query_tables(self):
        """The engine's device-built rotated-query table and MFMA fragments, copied to
        the host -> (table uint8 array, fragments uint8 array)."""
        tb, fb = query_table_sizes(self.kind, getattr(self, "nq", 0))
        tab, frag = np.zeros(tb, np.uint8), np.zeros(fb, np.uint8)
        _check(load_library().iris_engine_query_tables(self.handle, _ptr(tab) if tb else None, tb, _ptr(frag), fb))
        return tab, frag

    def batch_process(self, out, db, first=0, n=None):
        """batch_process(&self, out: &mut [[u16;31]], db: &[T]) (src/lib.rs:42-52, 69-79).

        `db` is a Database (records [first, first+n)) or a host array / list of records.
        `out` is a [n, 31] uint16 array (filled in place)."""
        lib = load_library()
        if out.dtype != np.uint16 or not out.flags.c_contiguous or out.ndim != 2 or out.shape[1] != ROTATIONS:
            raise IrisError(-1, "out must be a C-contiguous [n, 31] uint16 array")
        dt, width = _REC_DTYPE[self.kind]
        if (isinstance(db, np.ndarray) and db.dtype == dt and db.ndim == 2 and db.shape[1] == width
                and db.flags.c_contiguous and out.shape[0] == db.shape[0]):
            # the chunk walk's call (a contiguous slice of the caller's record array): passed as is,
            # with none of the conversions below, through the buffer protocol where the fast path
            # is built (csrc/iris_pycall.c), else ctypes
            pc = _pycall if _pycall is not _UNLOADED else _load_pycall()
            if pc is not None:
                rc = pc.batch_process_host((self.handle or _NULL).value or 0, db, out, db.itemsize * width)
            else:
                rc = lib.iris_engine_batch_process_host(self.handle, db.ctypes.data, db.shape[0], out.ctypes.data)
            if rc:
                _check(rc)
            return out
        if isinstance(db, Database):
            n = (len(db) - first) if n is None else n
            if out.shape[0] != n:  # assert_eq!(out.len(), db.len()) (src/lib.rs:43,70)
                raise IrisError(-1, f"assertion `out.len() == db.len()` failed: {out.shape[0]} != {n}")
            _check(lib.iris_engine_batch_process(self.handle, db.handle, int(first), int(n), _ptr(out)))
        else:
            a = _records(self.kind, db)  # a contiguous view of the caller's array is passed as is
            if out.shape[0] != a.shape[0]:
                raise IrisError(-1, f"assertion `out.len() == db.len()` failed: {out.shape[0]} != {a.shape[0]}")
            _check(lib.iris_engine_batch_process_host(self.handle, _ptr(a), a.shape[0], _ptr(out)))
        return out


def _batch_process_device(self, db, out_device_ptr, first=0, n=None):
    """Results stay on the GPU: out_device_ptr is a device array of n*31 u16."""
    n = (len(db) - first) if n is None else n
    rc = load_library().iris_engine_batch_process_device(self.handle, db.handle, int(first), int(n), int(out_device_ptr))
    if rc:
        _check(rc)


_Engine.batch_process_device = _batch_process_device


class MasksEngine(_Engine):
    """MasksEngine (src/lib.rs:55-80): out[k] = dot_bool(rot(query, k-15), entry)."""

    kind = KIND_MASKS

    def __init__(self, device, query):
        self.device = device
        q = query.limbs if isinstance(query, Bits) else _c(query, np.uint64)
        h = ctypes.c_void_p()
        _check(load_library().iris_masks_engine_new(device.handle, _ptr(_c(q, np.uint64)), ctypes.byref(h)))
        self.handle = h

    def resolve(self, db, shares, first=0, n=None, index_base=0, dist_out_device=None):
        """The resolver step with this engine's denominators computed on the fly
        (src/main.rs:510-519 + 597-621): shares = the participants' [n,31] u16 outputs,
        host arrays or device pointers.  Host arrays (and no dist_out_device) go through
        iris_resolver_search_masks_host: summed on the host, the sum uploaded.  -> Match."""
        if n is None:
            n = len(db) - int(first)
        dev = self.device
        if dist_out_device is None and shares and not any(isinstance(a, int) for a in shares):
            arrs = [_c(a, np.uint16) for a in shares]
            for a in arrs:
                if a.shape != (n, ROTATIONS):
                    raise IrisError(-1, "shares must be [n, 31] uint16")
            ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
            m = Match()
            _check(load_library().iris_resolver_search_masks_host(self.handle, db.handle, int(first), int(n), ptrs,
                                                                  len(arrs), int(index_base), ctypes.byref(m)))
            return m
        tmp = []
        try:
            ptrs = []
            for a in shares:
                if isinstance(a, int):
                    ptrs.append(a)
                    continue
                a = _c(a, np.uint16)
                if a.shape != (n, ROTATIONS):
                    raise IrisError(-1, "shares must be [n, 31] uint16")
                p = dev.alloc(max(a.nbytes, 16))
                tmp.append(p)
                dev.h2d(p, a)
                ptrs.append(p)
            arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
            m = Match()
            _check(load_library().iris_resolver_search_masks(self.handle, db.handle, int(first), int(n), arr,
                                                             len(ptrs), int(index_base),
                                                             ctypes.c_void_p(dist_out_device or 0), ctypes.byref(m)))
            return m
        finally:
            for p in tmp:
                dev.free(p)


    def matches(self, db, shares, threshold, first=0, n=None, index_base=0, cap=None, out=None):
        """Every record of the resolver step whose decoded distance is below `threshold`
        (iris_resolver_matches_masks; the threshold has no reference counterpart): shares = the
        participants' [n,31] u16 outputs, host arrays (uploaded for the call) or device pointers.
        Indices are index_base + row.  -> (list[Match] in ascending index order, count); cap / out
        as in TemplateEngine.matches."""
        if n is None:
            n = len(db) - int(first)
        dev = self.device
        tmp = []
        try:
            ptrs = []
            for a in shares:
                if isinstance(a, int):
                    ptrs.append(a)
                    continue
                a = _c(a, np.uint16)
                if a.shape != (n, ROTATIONS):
                    raise IrisError(-1, "shares must be [n, 31] uint16")
                p = dev.alloc(max(a.nbytes, 16))
                tmp.append(p)
                dev.h2d(p, a)
                ptrs.append(p)
            arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
            f = load_library().iris_resolver_matches_masks
            return _collect_matches(lambda o, c, cnt: f(self.handle, db.handle, int(first), int(n), arr, len(ptrs),
                                                        int(index_base), float(threshold), o, c, cnt), cap, out, self)
        finally:
            for p in tmp:
                dev.free(p)


    def topk(self, db, shares, k, first=0, n=None, index_base=0):
        """The k closest records of the resolver step, best first (iris_resolver_topk_masks; k has
        no reference counterpart): shares as in matches().  Indices are index_base + row.
        -> list[Match] of min(k, rows with a valid rotation) entries."""
        if n is None:
            n = len(db) - int(first)
        dev = self.device
        tmp = []
        try:
            ptrs = []
            for a in shares:
                if isinstance(a, int):
                    ptrs.append(a)
                    continue
                a = _c(a, np.uint16)
                if a.shape != (n, ROTATIONS):
                    raise IrisError(-1, "shares must be [n, 31] uint16")
                p = dev.alloc(max(a.nbytes, 16))
                tmp.append(p)
                dev.h2d(p, a)
                ptrs.append(p)
            arr = (ctypes.c_void_p * len(ptrs))(*ptrs)
            f = load_library().iris_resolver_topk_masks
            return _collect_topk(lambda o, cnt: f(self.handle, db.handle, int(first), int(n), arr, len(ptrs),
                                                  int(index_base), int(k), o, cnt), k)
        finally:
            for p in tmp:
                dev.free(p)

    def histogram(self, db, share_ptrs, nbins, first=0, n=None):
        """The distance distribution of the resolver step in one masks pass
        (iris_resolver_histogram_masks; no reference counterpart): share_ptrs are the participants'
        device arrays of n*31 u16.  -> (bins: np.ndarray[nbins] of uint64, invalid: int).  A row is
        counted in bin min(nbins - 1, floor(distance * nbins)) -- a distance above 1 (garbage shares)
        in the last -- one without a valid rotation in `invalid` alone; nbins is a power of two up
        to HIST_MAX_BINS.  The prefix sum of j bins is matches(j / nbins, cap=0)'s total."""
        n = (len(db) - int(first)) if n is None else n
        nb = int(nbins)
        ptrs = [int(p) for p in share_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        bins = np.zeros(nb if 0 < nb <= HIST_MAX_BINS else 1, np.uint64)
        invalid = ctypes.c_uint64(0)
        _check(load_library().iris_resolver_histogram_masks(self.handle, db.handle, int(first), int(n), arr, len(ptrs), nb,
                                                            _ptr(bins), ctypes.addressof(invalid)))
        return bins, int(invalid.value)

    def report(self, db, share_ptrs, threshold=None, cap=None, k=None, nbins=None, first=0, n=None, index_base=0):
        """Several of matches(), topk() and histogram() of the resolver step from ONE masks pass
        (iris_resolver_report_masks; no reference counterpart) -> ReportResult, shaped like
        TemplateEngine.report: `threshold` (with `cap`) asks for .matches and .matches_count, `k` for
        .topk, `nbins` for .bins and .invalid; each is exactly what the sibling method returns.
        share_ptrs are the participants' device arrays of n*31 u16."""
        n = (len(db) - int(first)) if n is None else n
        ptrs = [int(p) for p in share_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        f = load_library().iris_resolver_report_masks
        return _report(lambda r: f(self.handle, db.handle, int(first), int(n), arr, len(ptrs), int(index_base), r), self,
                       threshold, cap, k, nbins,
                       lambda count: self.matches(db, ptrs, threshold, first, n, index_base, cap=count)[0])


class DistanceEngine(_Engine):
    """DistanceEngine (src/lib.rs:28-53): out[k] = dot_u16(rot(query, k-15), entry)."""

    kind = KIND_SHARES

    def __init__(self, device, query):
        self.device = device
        q = query.values if isinstance(query, EncodedBits) else _c(query, np.uint16)
        h = ctypes.c_void_p()
        _check(load_library().iris_distance_engine_new(device.handle, _ptr(_c(q, np.uint16)), ctypes.byref(h)))
        self.handle = h


class TemplateEngine(_Engine):
    """Masked fractional Hamming of one query Template against a Template DB
    (src/template.rs:43-64): counts per rotation, distances, fused argmin."""

    kind = KIND_TEMPLATES

    def __init__(self, device, query):
        self.device = device
        q = query.to_array() if isinstance(query, Template) else _c(query, np.uint64)
        h = ctypes.c_void_p()
        _check(load_library().iris_template_engine_new(device.handle, _ptr(_c(q, np.uint64)), ctypes.byref(h)))
        self.handle = h
        self._query = _c(q, np.uint64).copy()  # PendingMatches: a cap=None list longer than its room

    def counts(self, db, first=0, n=None):
        """-> (num [n,31] u16, den [n,31] u16)."""
        n = (len(db) - first) if n is None else n
        num = np.empty((n, ROTATIONS), np.uint16)
        den = np.empty((n, ROTATIONS), np.uint16)
        _check(load_library().iris_template_counts(self.handle, db.handle, int(first), int(n), _ptr(num), _ptr(den)))
        return num, den

    def distances(self, db, first=0, n=None):
        """Template::distance(query, db[i]) for every i -> [n] f64."""
        n = (len(db) - first) if n is None else n
        out = np.empty(n, np.float64)
        _check(load_library().iris_template_distances(self.handle, db.handle, int(first), int(n), _ptr(out)))
        return out

    def distances_host(self, records, layout=LAYOUT_DEFAULT):
        a = _records(KIND_TEMPLATES, records)
        with Database(self.device, KIND_TEMPLATES, max(1, a.shape[0]), layout) as db:
            db.append(a)
            return self.distances(db)

    def search_async(self, db, first=0, n=None, index_base=0):
        """Enqueue the fused min/argmin and return at once -> PendingSearch (wait() -> Match)."""
        n = (len(db) - first) if n is None else n
        h = ctypes.c_void_p()
        _check(load_library().iris_template_search_async(self.handle, db.handle, int(first), int(n),
                                                         int(index_base), ctypes.byref(h)))
        return PendingSearch(h)

    def search(self, db, first=0, n=None, index_base=0, dist_out_device=None):
        """Fused min/argmin (src/main.rs:581-621) -> Match."""
        n = (len(db) - first) if n is None else n
        m = Match()
        rc = load_library().iris_template_search(self.handle, db.handle, int(first), int(n), int(index_base),
                                                 dist_out_device or None, ctypes.byref(m))
        if rc:
            _check(rc)
        return m


    def matches(self, db, threshold, first=0, n=None, index_base=0, cap=None, out=None):
        """Every record whose distance is below `threshold`, in one database pass
        (iris_template_matches; the threshold has no reference counterpart) -> (list[Match] in
        ascending index order, count).  cap=None returns them all; with a cap the list holds the
        min(count, cap) lowest indices and count is still the total; cap=0 only counts.  out: a
        (Match * cap) ctypes array to fill in place."""
        n = (len(db) - first) if n is None else n
        f = load_library().iris_template_matches
        return _collect_matches(lambda o, c, cnt: f(self.handle, db.handle, int(first), int(n), int(index_base),
                                                    float(threshold), o, c, cnt), cap, out, self)

    def matches_async(self, db, threshold, first=0, n=None, index_base=0, cap=None):
        """Enqueue matches() and return at once (iris_template_matches_async) -> PendingMatches,
        whose wait() returns what matches() with the same arguments returns.  The engine may be
        closed before the wait; the database stays alive and unmodified until it.  cap=None asks
        for every match: the pending holds room as matches() would on its first call, and a longer
        list is fetched by one blocking matches() at the wait."""
        n = (len(db) - first) if n is None else n
        want_all = cap is None
        cap = max(1024, getattr(self, "_match_room", 0)) if want_all else int(cap)
        h = ctypes.c_void_p()
        _check(load_library().iris_template_matches_async(self.handle, db.handle, int(first), int(n), int(index_base),
                                                          float(threshold), cap, ctypes.byref(h)))
        again = None
        if want_all:
            device, q, args = self.device, self._query, (db, threshold, first, n, index_base)

            def again(count):
                with TemplateEngine(device, q) as e:
                    return e.matches(*args, cap=count)
        return PendingMatches(h, cap, again)

    def topk(self, db, k, first=0, n=None, index_base=0):
        """The k closest records of the range, best first, in one database pass
        (iris_template_topk; k = 1..TOPK_MAX has no reference counterpart) -> list[Match] of
        min(k, records with a valid rotation) entries; [0] is search()'s result."""
        n = (len(db) - first) if n is None else n
        f = load_library().iris_template_topk
        return _collect_topk(lambda o, cnt: f(self.handle, db.handle, int(first), int(n), int(index_base), int(k),
                                              o, cnt), k)

    def histogram(self, db, nbins, first=0, n=None):
        """The distribution of the range's distances in one database pass (iris_template_histogram;
        no reference counterpart) -> (np.ndarray[nbins] of uint64, invalid).  A record is counted in
        bin min(nbins - 1, floor(distance * nbins)) of its best rotation's distance, a record
        without a valid rotation in `invalid` alone; nbins is a power of two up to HIST_MAX_BINS.
        The prefix sum of j bins is matches(j / nbins, cap=0)'s total.  Histograms of chunks add."""
        n = (len(db) - first) if n is None else n
        nb = int(nbins)
        bins = np.zeros(nb if 0 < nb <= HIST_MAX_BINS else 1, np.uint64)
        invalid = ctypes.c_uint64()
        _check(load_library().iris_template_histogram(self.handle, db.handle, int(first), int(n), nb, _ptr(bins),
                                                      ctypes.byref(invalid)))
        return bins, int(invalid.value)

    def report(self, db, threshold=None, cap=None, k=None, nbins=None, first=0, n=None, index_base=0):
        """Several of matches(), topk() and histogram() from ONE read of the range
        (iris_template_report; no reference counterpart) -> ReportResult.  A part is asked for by
        its argument: `threshold` (with `cap` as in matches(): None returns every match, 0 only
        counts) fills .matches and .matches_count, `k` fills .topk, `nbins` fills .bins and
        .invalid; each is exactly what the sibling method returns, the others stay None.  At least
        one part must be asked for."""
        n = (len(db) - first) if n is None else n
        f = load_library().iris_template_report
        return _report(lambda r: f(self.handle, db.handle, int(first), int(n), int(index_base), r), self, threshold, cap, k, nbins,
                       lambda count: self.matches(db, threshold, first, n, index_base, cap=count)[0])

    def report_async(self, db, threshold=None, cap=None, k=None, nbins=None, first=0, n=None, index_base=0):
        """Enqueue report() and return at once (iris_template_report_async) -> PendingReport, whose
        wait() returns the ReportResult that report() with the same arguments returns.  A report
        pass that is still streaming the database also computes the one submitted after it,
        whatever parts and arguments the two ask for; `nbins` alone is the pipelined histogram.
        The engine may be closed before the wait; the database stays alive and unmodified until it.
        cap None returns every match: the pass has room for 1024 records (or what the engine
        remembers of its last list), and a longer list comes from matches() at the wait -- the
        one case in which the engine must still be open then."""
        n = (len(db) - first) if n is None else n
        r = Report()  # the in scalars only: the submission reads no pointer
        room = None
        if threshold is not None:
            r.parts |= REPORT_MATCHES
            r.threshold = float(threshold)
            room = max(1024, getattr(self, "_match_room", 0)) if cap is None else int(cap)
            r.matches_cap = room
        if k is not None:
            r.parts |= REPORT_TOPK
            r.k = int(k)
        if nbins is not None:
            r.parts |= REPORT_HIST
            r.nbins = int(nbins)
        h = ctypes.c_void_p()
        _check(load_library().iris_template_report_async(self.handle, db.handle, int(first), int(n), int(index_base),
                                                         ctypes.byref(r), ctypes.byref(h)))
        rematch = None
        if threshold is not None and cap is None:
            rematch = lambda count: self.matches(db, threshold, first, n, index_base, cap=count)[0]
        return PendingReport(h, self, threshold, room, k, nbins, rematch)

    def topk_async(self, db, k, first=0, n=None, index_base=0):
        """Enqueue topk() and return at once (iris_template_topk_async) -> PendingTopk, whose
        wait() returns what topk() with the same arguments returns.  The engine may be closed
        before the wait; the database stays alive and unmodified until it."""
        n = (len(db) - first) if n is None else n
        h = ctypes.c_void_p()
        _check(load_library().iris_template_topk_async(self.handle, db.handle, int(first), int(n), int(index_base),
                                                       int(k), ctypes.byref(h)))
        return PendingTopk(h, int(k))


class PendingReport:
    """An enqueued report pass (TemplateEngine.report_async); wait() -> ReportResult, once."""

    def __init__(self, handle, owner, threshold, room, k, nbins, rematch):
        self.handle = handle
        self._args = (owner, threshold, room, k, nbins, rematch)

    def wait(self):
        if self.handle is None:
            raise IrisError(-1, "PendingReport.wait called twice")
        h, self.handle = self.handle, None
        owner, threshold, room, k, nbins, rematch = self._args
        f = load_library().iris_pending_report_wait
        res = _report(lambda r: f(h, r), owner, threshold, room, k, nbins, rematch)
        if rematch is not None:  # cap None: every match, as report() returns them
            if res.matches_count > room:
                res.matches = rematch(res.matches_count)
            owner._match_room = min(res.matches_count + res.matches_count // 4, 1 << 22)
        return res

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                load_library().iris_pending_report_wait(self.handle, None)  # refused, and the handle freed
            except Exception:
                pass


class PendingTopk:
    """An enqueued top-k pass (TemplateEngine.topk_async); wait() -> list[Match], once."""

    def __init__(self, handle, k):
        self.handle = handle
        self.k = k

    def wait(self):
        if self.handle is None:
            raise IrisError(-1, "PendingTopk.wait called twice")
        h, self.handle = self.handle, None
        f = load_library().iris_pending_topk_wait
        return _collect_topk(lambda o, cnt: f(h, o, cnt), self.k)

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                load_library().iris_pending_topk_wait(self.handle, None, ctypes.byref(ctypes.c_uint32()))
            except Exception:
                pass


class PendingSearch:
    """An enqueued search (TemplateEngine.search_async); wait() -> Match, once."""

    def __init__(self, handle):
        self.handle = handle

    def wait(self):
        if self.handle is None:
            raise IrisError(-1, "PendingSearch.wait called twice")
        m = Match()
        h, self.handle = self.handle, None
        _check(load_library().iris_pending_wait(h, ctypes.byref(m)))
        return m

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                load_library().iris_pending_wait(self.handle, None)
            except Exception:
                pass


class PendingMatches:
    """An enqueued threshold-match pass (TemplateEngine.matches_async); wait() -> (list[Match],
    count), once."""

    def __init__(self, handle, cap, again=None):
        self.handle = handle
        self.cap = cap
        self._again = again

    def wait(self):
        if self.handle is None:
            raise IrisError(-1, "PendingMatches.wait called twice")
        buf = (Match * self.cap)() if self.cap else None
        count = ctypes.c_uint64()
        h, self.handle = self.handle, None
        _check(load_library().iris_pending_matches_wait(h, buf, ctypes.byref(count)))
        if self._again is not None and count.value > self.cap:
            return self._again(count.value)
        return [buf[i] for i in range(min(self.cap, count.value))], count.value

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                load_library().iris_pending_matches_wait(self.handle, None, ctypes.byref(ctypes.c_uint64()))
            except Exception:
                pass


class TemplateBatchEngine(_Engine):
    """Many query Templates against one template DB in one pass (configs[2])."""

    kind = KIND_TEMPLATES

    def __init__(self, device, queries):
        self.device = device
        q = _records(KIND_TEMPLATES, queries)
        self.nq = q.shape[0]
        h = ctypes.c_void_p()
        _check(load_library().iris_template_batch_engine_new(device.handle, _ptr(q), self.nq, ctypes.byref(h)))
        self.handle = h

    def search(self, db, first=0, n=None, index_base=0):
        n = (len(db) - first) if n is None else n
        out = (Match * self.nq)()
        _check(load_library().iris_template_batch_search(self.handle, db.handle, int(first), int(n), int(index_base),
                                                         out))
        return list(out)

    def matches(self, db, threshold, first=0, n=None, index_base=0, cap=None, out=None):
        """Every query's records whose distance is below `threshold`, in one pass over the
        templates (iris_template_batch_matches; the threshold has no reference counterpart).
        -> (lists, counts): lists[q] is the list[Match] TemplateEngine(queries[q]).matches gives
        over the same range (ascending index, index_base + first + i), counts[q] its exact total.
        cap is per query: None asks for every match (room for min(1024, max(16, 65536 // nq)) a
        query first -- 64 at 1024 queries, 2 MB of Match -- then once more with room for the longest
        reported list); 0 with out=None only counts.  out: a (Match * (nq * cap)) ctypes array
        filled in place, query-major (entries past a query's list stay untouched); cap defaults to
        len(out) // nq."""
        n = (len(db) - first) if n is None else n
        counts = (ctypes.c_uint64 * self.nq)()
        f = load_library().iris_template_batch_matches

        def call(buf, room):
            _check(f(self.handle, db.handle, int(first), int(n), int(index_base), float(threshold), buf, room, counts))

        want_all = out is None and cap is None
        if out is not None:
            cap = len(out) // self.nq if cap is None else int(cap)
            if self.nq * cap > len(out):
                raise IrisError(-1, "nq * cap exceeds len(out)")
            buf = out
        else:
            cap = min(1024, max(16, 65536 // self.nq)) if want_all else int(cap)
            buf = (Match * (self.nq * cap))() if cap else None
        call(buf, cap)
        if want_all and max(counts) > cap:
            cap = max(counts)
            buf = (Match * (self.nq * cap))()
            call(buf, cap)
        totals = [int(c) for c in counts]
        return [[buf[q * cap + j] for j in range(min(cap, totals[q]))] for q in range(self.nq)], totals

    def topk(self, db, k, first=0, n=None, index_base=0):
        """Every query's k closest records, best first, in one pass over the templates
        (iris_template_batch_topk; k = 1..TOPK_MAX has no reference counterpart).  -> list of nq
        lists: entry q is the list[Match] TemplateEngine(queries[q]).topk gives over the same range
        (indices index_base + first + i)."""
        n = (len(db) - first) if n is None else n
        room = max(1, min(int(k), TOPK_MAX)) if int(k) > 0 else 1
        out = (Match * (self.nq * room))()
        counts = (ctypes.c_uint32 * self.nq)()
        _check(load_library().iris_template_batch_topk(self.handle, db.handle, int(first), int(n), int(index_base),
                                                       int(k), out, counts))
        return [[_copy_match(out[q * room + j]) for j in range(counts[q])] for q in range(self.nq)]

    def histogram(self, db, nbins, first=0, n=None):
        """Every query's distance histogram in one pass over the templates
        (iris_template_batch_histogram) -> (np.ndarray[nq, nbins] of uint64, np.ndarray[nq] of
        uint64): row q and entry q are what TemplateEngine(queries[q]).histogram gives over the
        same range."""
        n = (len(db) - first) if n is None else n
        nb = int(nbins)
        bins = np.zeros((self.nq, nb if 0 < nb <= HIST_MAX_BINS else 1), np.uint64)
        invalid = np.zeros(self.nq, np.uint64)
        _check(load_library().iris_template_batch_histogram(self.handle, db.handle, int(first), int(n), nb, _ptr(bins),
                                                            _ptr(invalid)))
        return bins, invalid

    def report(self, db, parts, threshold=0.0, cap=0, k=0, nbins=0, first=0, n=None, index_base=0):
        """Several of matches(), topk() and histogram() for every query from ONE pass over the
        templates (iris_template_batch_report; no reference counterpart) -> BatchReportResult.
        parts: REPORT_MATCHES | REPORT_TOPK | REPORT_HIST; threshold and cap (records per query; 0
        only counts) serve the matches part, k the top-k part, nbins the histogram part.  Each part
        is byte for byte what the sibling method's call writes: matches[q] the min(count, cap)
        lowest indices, matches_counts[q] the exact total, topk[q] best first, bins[q] and
        invalid[q] query q's histogram.  The records are views of the arrays the call filled."""
        n = (len(db) - first) if n is None else n
        f = load_library().iris_template_batch_report
        return _batch_report(self.nq, parts, threshold, cap, k, nbins, lambda r: f(
            self.handle, db.handle, int(first), int(n), int(index_base), ctypes.byref(r)))


def _batch_report(nq, parts, threshold, cap, k, nbins, call):
    """One batch report call (iris_template_batch_report, iris_resolver_batch_report_masks): the
    iris_batch_report_t and the arrays of the selected parts for nq queries, call(struct) -> rc,
    then the BatchReportResult whose records are views of the arrays the call filled."""
    parts = int(parts)
    r = BatchReport()
    res = BatchReportResult()
    r.parts = parts
    marr = mcounts = tarr = tcounts = None
    room = 1
    if parts & REPORT_MATCHES:
        r.threshold = float(threshold)
        r.matches_cap = int(cap)
        if int(cap):
            marr = (Match * (nq * int(cap)))()
            r.matches = marr
        mcounts = (ctypes.c_uint64 * nq)()
        r.matches_counts = mcounts
    if parts & REPORT_TOPK:
        r.k = int(k)
        room = max(1, min(int(k), TOPK_MAX)) if int(k) > 0 else 1
        tarr = (Match * (nq * room))()
        tcounts = (ctypes.c_uint32 * nq)()
        r.topk = tarr
        r.topk_counts = tcounts
    if parts & REPORT_HIST:
        nb = int(nbins)
        r.nbins = nb
        res.bins = np.zeros((nq, nb if 0 < nb <= HIST_MAX_BINS else 1), np.uint64)
        res.invalid = np.zeros(nq, np.uint64)
        r.bins = res.bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        r.invalid = res.invalid.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    _check(call(r))
    if parts & REPORT_MATCHES:
        c = int(cap)
        res.matches_counts = [int(x) for x in mcounts]
        res.matches = [[marr[q * c + j] for j in range(min(c, res.matches_counts[q]))] for q in range(nq)]
    if parts & REPORT_TOPK:
        res.topk = [[tarr[q * room + j] for j in range(tcounts[q])] for q in range(nq)]
    return res


class DistanceBatchEngine(_Engine):
    """nq DistanceEngines at once (iris_distance_batch_engine_new): one pass over a share database
    answers every query; out[q] is what DistanceEngine(queries[q]).batch_process writes."""

    kind = KIND_SHARES

    def __init__(self, device, queries):
        self.device = device
        q = _records(KIND_SHARES, queries)
        self.nq = q.shape[0]
        h = ctypes.c_void_p()
        _check(load_library().iris_distance_batch_engine_new(device.handle, _ptr(q), self.nq, ctypes.byref(h)))
        self.handle = h

    def query_tables(self):
        raise IrisError(-1, "a distance batch engine holds one DistanceEngine's tables per query")

    def batch_process(self, out, db, first=0, n=None):
        """`db` is a share Database (records [first, first+n)); `out` a C-contiguous [nq, n, 31]
        uint16 array, filled in place: out[q, i, k] = dot_u16(rot(queries[q], k-15), db[first+i])."""
        n = (len(db) - first) if n is None else n
        if (not isinstance(out, np.ndarray) or out.dtype != np.uint16 or not out.flags.c_contiguous or out.ndim != 3
                or out.shape[0] != self.nq or out.shape[2] != ROTATIONS):
            raise IrisError(-1, f"out must be a C-contiguous [{self.nq}, n, 31] uint16 array")
        if out.shape[1] != n:  # assert_eq!(out.len(), db.len()) (src/lib.rs:43), per query
            raise IrisError(-1, f"assertion `out.len() == db.len()` failed: {out.shape[1]} != {n}")
        _check(load_library().iris_distance_batch_process(self.handle, db.handle, int(first), int(n), _ptr(out)))
        return out

    def batch_process_device(self, db, out_device_ptr, first=0, n=None):
        """Results stay on the GPU: out_device_ptr is a device array of nq*n*31 u16 (query-major)."""
        n = (len(db) - first) if n is None else n
        rc = load_library().iris_distance_batch_process_device(self.handle, db.handle, int(first), int(n),
                                                               int(out_device_ptr))
        if rc:
            _check(rc)


class MasksBatchEngine(_Engine):
    """nq MasksEngines at once (iris_masks_batch_engine_new): one pass over a masks database answers
    every query; out[q] is what MasksEngine(masks[q]).batch_process writes, and resolve() is the
    resolver step of every query against the participants' DistanceBatchEngine outputs."""

    kind = KIND_MASKS

    def __init__(self, device, masks):
        self.device = device
        q = _records(KIND_MASKS, masks)
        self.nq = q.shape[0]
        h = ctypes.c_void_p()
        _check(load_library().iris_masks_batch_engine_new(device.handle, _ptr(q), self.nq, ctypes.byref(h)))
        self.handle = h

    def query_tables(self):
        raise IrisError(-1, "a masks batch engine holds one MasksEngine's tables per query")

    def batch_process(self, out, db, first=0, n=None):
        """`db` is a masks Database (records [first, first+n)); `out` a C-contiguous [nq, n, 31]
        uint16 array, filled in place: out[q, i, k] = dot_bool(rot(masks[q], k-15), db[first+i])."""
        n = (len(db) - first) if n is None else n
        if (not isinstance(out, np.ndarray) or out.dtype != np.uint16 or not out.flags.c_contiguous or out.ndim != 3
                or out.shape[0] != self.nq or out.shape[2] != ROTATIONS):
            raise IrisError(-1, f"out must be a C-contiguous [{self.nq}, n, 31] uint16 array")
        if out.shape[1] != n:  # assert_eq!(out.len(), db.len()) (src/lib.rs:70), per query
            raise IrisError(-1, f"assertion `out.len() == db.len()` failed: {out.shape[1]} != {n}")
        _check(load_library().iris_masks_batch_process(self.handle, db.handle, int(first), int(n), _ptr(out)))
        return out

    def batch_process_device(self, db, out_device_ptr, first=0, n=None):
        """Results stay on the GPU: out_device_ptr is a device array of nq*n*31 u16 (query-major)."""
        n = (len(db) - first) if n is None else n
        rc = load_library().iris_masks_batch_process_device(self.handle, db.handle, int(first), int(n),
                                                            int(out_device_ptr))
        if rc:
            _check(rc)

    def resolve(self, db, shares_device_ptrs, first=0, n=None, index_base=0, dist_out=None):
        """The resolver step of every query in one pass over masks records [first, first+n):
        shares_device_ptrs[p] is participant p's device array of nq*n*31 u16, query-major (what
        DistanceBatchEngine.batch_process_device wrote over the same records); dist_out: None or
        a device array of nq*n doubles (query-major).  -> list of nq Match."""
        n = (len(db) - first) if n is None else n
        ptrs = [int(p) for p in shares_device_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        out = (Match * self.nq)()
        _check(load_library().iris_resolver_batch_search_masks(self.handle, db.handle, int(first), int(n), arr,
                                                               len(ptrs), int(index_base),
                                                               ctypes.c_void_p(dist_out or 0), out))
        return list(out)

    def matches(self, db, shares_device_ptrs, threshold, first=0, n=None, index_base=0, cap=None, out=None):
        """Every query's records of that resolver step whose decoded distance is below `threshold`,
        in one pass over the masks (iris_resolver_batch_matches_masks; the threshold has no
        reference counterpart): shares_device_ptrs as in resolve().  -> (lists, counts): lists[q]
        is the list[Match] MasksEngine(masks[q]).matches gives on slab q of every part (ascending
        index, index_base + row), counts[q] its exact total.  cap is per query: None asks for every
        match (room for 1024 a query, then once more with room for the longest reported list); 0
        with out=None only counts.  out: a (Match * (nq * cap)) ctypes array filled in place,
        query-major (entries past a query's list stay untouched); cap defaults to len(out) // nq."""
        n = (len(db) - first) if n is None else n
        ptrs = [int(p) for p in shares_device_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        counts = (ctypes.c_uint64 * self.nq)()
        f = load_library().iris_resolver_batch_matches_masks

        def call(buf, room):
            _check(f(self.handle, db.handle, int(first), int(n), arr, len(ptrs), int(index_base), float(threshold),
                     buf, room, counts))

        want_all = out is None and cap is None
        if out is not None:
            cap = len(out) // self.nq if cap is None else int(cap)
            if self.nq * cap > len(out):
                raise IrisError(-1, "nq * cap exceeds len(out)")
            buf = out
        else:
            cap = 1024 if want_all else int(cap)
            buf = (Match * (self.nq * cap))() if cap else None
        call(buf, cap)
        if want_all and max(counts) > cap:
            cap = max(counts)
            buf = (Match * (self.nq * cap))()
            call(buf, cap)
        totals = [int(c) for c in counts]
        return [[buf[q * cap + j] for j in range(min(cap, totals[q]))] for q in range(self.nq)], totals

    def topk(self, db, shares_device_ptrs, k, first=0, n=None, index_base=0):
        """Every query's k closest records of that resolver step, best first, in one pass over the
        masks (iris_resolver_batch_topk_masks; k = 1..TOPK_MAX has no reference counterpart):
        shares_device_ptrs as in resolve().  -> list of nq lists: entry q is the list[Match]
        MasksEngine(masks[q]).topk gives on slab q of every part (indices index_base + row)."""
        n = (len(db) - first) if n is None else n
        ptrs = [int(p) for p in shares_device_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        room = max(1, min(int(k), TOPK_MAX)) if int(k) > 0 else 1
        out = (Match * (self.nq * room))()
        counts = (ctypes.c_uint32 * self.nq)()
        _check(load_library().iris_resolver_batch_topk_masks(self.handle, db.handle, int(first), int(n), arr, len(ptrs),
                                                             int(index_base), int(k), out, counts))
        return [[_copy_match(out[q * room + j]) for j in range(counts[q])] for q in range(self.nq)]

    def histogram(self, db, shares_device_ptrs, nbins, first=0, n=None):
        """Every query's distance histogram of that resolver step, up to 4 queries a masks pass
        (iris_resolver_batch_histogram_masks): shares_device_ptrs as in resolve().
        -> (np.ndarray[nq, nbins] of uint64, np.ndarray[nq] of uint64): row q and entry q are what
        MasksEngine(masks[q]).histogram gives on slab q of every part."""
        n = (len(db) - first) if n is None else n
        nb = int(nbins)
        ptrs = [int(p) for p in shares_device_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        bins = np.zeros((self.nq, nb if 0 < nb <= HIST_MAX_BINS else 1), np.uint64)
        invalid = np.zeros(self.nq, np.uint64)
        _check(load_library().iris_resolver_batch_histogram_masks(self.handle, db.handle, int(first), int(n), arr, len(ptrs),
                                                                  nb, _ptr(bins), _ptr(invalid)))
        return bins, invalid

    def report(self, db, shares_device_ptrs, parts, threshold=0.0, cap=0, k=0, nbins=0, first=0, n=None, index_base=0):
        """Several of matches(), topk() and histogram() for every query from ONE pass over the
        masks and the share slabs (iris_resolver_batch_report_masks; no reference counterpart)
        -> BatchReportResult, as TemplateBatchEngine.report returns it.  shares_device_ptrs as in
        resolve(); parts: REPORT_MATCHES | REPORT_TOPK | REPORT_HIST; threshold and cap (records
        per query; 0 only counts) serve the matches part, k the top-k part, nbins the histogram
        part.  Each part is byte for byte what the sibling method's call writes; topk[q][0] at
        k = 1 is resolve()'s entry q."""
        n = (len(db) - first) if n is None else n
        ptrs = [int(p) for p in shares_device_ptrs]
        arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
        f = load_library().iris_resolver_batch_report_masks
        return _batch_report(self.nq, parts, threshold, cap, k, nbins, lambda r: f(
            self.handle, db.handle, int(first), int(n), arr, len(ptrs), int(index_base), ctypes.byref(r)))


# ====================================================================== device groups


class Group:
    """Devices searched together (include/iris_hip.h "device groups"): a sharded template
    database, per-shard winners all-gathered over RCCL and merged on every device.
    Group(ordinals) drives several devices from this process (ncclCommInitAll);
    Group.rank(ordinal, nranks, rank, uid) is one device of a multi-process group whose
    128-byte id comes from Group.unique_id() on rank 0."""

    def __init__(self, ordinals=(0,), _handle=None):
        if _handle is not None:
            self.handle = _handle
        else:
            ords = (ctypes.c_int * len(ordinals))(*[int(o) for o in ordinals])
            h = ctypes.c_void_p()
            _check(load_library().iris_group_create(ords, len(ordinals), ctypes.byref(h)))
            self.handle = h
        l, r, f = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(load_library().iris_group_info(self.handle, ctypes.byref(l), ctypes.byref(r), ctypes.byref(f)))
        self.local_devices, self.ranks, self.first_rank = l.value, r.value, f.value
        # what RCCL reports: its communicators' rank count and every rank's device PCI bus id
        cr = ctypes.c_uint32()
        ids = ctypes.create_string_buffer(32 * self.ranks)
        _check(load_library().iris_group_rccl_info(self.handle, ctypes.byref(cr), ids, len(ids)))
        self.rccl_nranks = cr.value
        self.rccl_devices = [ids.raw[32 * k:32 * (k + 1)].split(b"\0", 1)[0].decode() for k in range(self.ranks)]
        self.devices = []
        for i in range(self.local_devices):
            d = ctypes.c_void_p()
            _check(load_library().iris_group_device(self.handle, i, ctypes.byref(d)))
            self.devices.append(_BorrowedDevice(d))

    @staticmethod
    def unique_id():
        buf = (ctypes.c_uint8 * 128)()
        _check(load_library().iris_group_unique_id(buf))
        return bytes(buf)

    @classmethod
    def rank(cls, ordinal, nranks, rank, uid):
        if len(uid) != 128:
            raise ValueError("the group id is 128 bytes")
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(bytes(uid))
        h = ctypes.c_void_p()
        _check(load_library().iris_group_create_rank(int(ordinal), int(nranks), int(rank), buf, ctypes.byref(h)))
        return cls(_handle=h)

    def set_timeout(self, ms):
        """Bound (ms) of the exchange waits of later calls; 0 = automatic (iris_group_set_timeout)."""
        _check(load_library().iris_group_set_timeout(self.handle, int(ms)))

    def close(self):
        if getattr(self, "handle", None):
            load_library().iris_group_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BorrowedDevice(Device):
    """A group's device handle (owned by the group: close() does nothing)."""

    def __init__(self, handle):
        self.handle = handle
        self.ordinal = None

    def close(self):
        self.handle = None


class _BorrowedDatabase(Database):
    """A group shard's database (owned by the group database: close() does nothing)."""

    def __init__(self, handle, device, kind):
        self.handle = handle
        self.device = device
        self.kind = kind

    def close(self):
        self.handle = None


class GroupDatabase:
    """`total` records of `kind` in S = ranks x shards_per_device contiguous shards over a
    Group; every record starts empty (never a candidate)."""

    def __init__(self, group, kind, total, layout=LAYOUT_DEFAULT, shards_per_device=1):
        self.group = group
        self.kind = kind
        h = ctypes.c_void_p()
        _check(load_library().iris_group_db_create(group.handle, int(kind), int(total), int(layout),
                                                   int(shards_per_device), ctypes.byref(h)))
        self.handle = h
        t, S, f, l = ctypes.c_uint64(), ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        _check(load_library().iris_group_db_info(h, ctypes.byref(t), ctypes.byref(S), ctypes.byref(f),
                                                 ctypes.byref(l)))
        self.total, self.shards, self.first_shard, self.local_shards = t.value, S.value, f.value, l.value

    def shard(self, i):
        """-> (first global index, count) of local shard i."""
        f, c = ctypes.c_uint64(), ctypes.c_uint64()
        _check(load_library().iris_group_db_shard(self.handle, int(i), None, ctypes.byref(f), ctypes.byref(c)))
        return f.value, c.value

    def shard_db(self, i):
        """Local shard i as a Database (borrowed: owned by this group database), e.g. for a
        local search with no exchange; its record j is global record shard(i)[0] + j."""
        h = ctypes.c_void_p()
        _check(load_library().iris_group_db_shard(self.handle, int(i), ctypes.byref(h), None, None))
        spd = self.local_shards // self.group.local_devices
        return _BorrowedDatabase(h, self.group.devices[int(i) // spd], self.kind)

    def close(self):
        if getattr(self, "handle", None):
            load_library().iris_group_db_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return self.total

    def generate(self, seed):
        _check(load_library().iris_group_db_generate(self.handle, int(seed)))

    def write(self, index, records):
        a = _records(self.kind, records)
        _check(load_library().iris_group_db_write(self.handle, int(index), _ptr(a), a.shape[0]))

    def read(self, index, n):
        dt, width = _REC_DTYPE[self.kind]
        out = np.empty((n, width), dt)
        _check(load_library().iris_group_db_read(self.handle, int(index), int(n), _ptr(out)))
        return out

    def load_file(self, path, first=0):
        _check(load_library().iris_group_db_load_file(self.handle, os.fsencode(path), int(first)))

    def search(self, query):
        """Global (min distance, lowest index) of one query Template -> Match."""
        q = query.to_array() if isinstance(query, Template) else _c(query, np.uint64)
        m = Match()
        _check(load_library().iris_group_template_search(self.handle, _ptr(_c(q, np.uint64)), ctypes.byref(m)))
        return m

    def search_async(self, query):
        q = query.to_array() if isinstance(query, Template) else _c(query, np.uint64)
        h = ctypes.c_void_p()
        _check(load_library().iris_group_template_search_async(self.handle, _ptr(_c(q, np.uint64)), ctypes.byref(h)))
        return GroupPendingSearch(h)

    def batch_search(self, queries):
        q = _records(KIND_TEMPLATES, queries)
        out = (Match * q.shape[0])()
        _check(load_library().iris_group_template_batch_search(self.handle, _ptr(q), q.shape[0], out))
        return list(out)


class GroupPendingSearch:
    """An enqueued group search; wait() -> Match, once."""

    def __init__(self, handle):
        self.handle = handle

    def wait(self):
        if self.handle is None:
            raise IrisError(-1, "GroupPendingSearch.wait called twice")
        m = Match()
        h, self.handle = self.handle, None
        _check(load_library().iris_group_pending_wait(h, ctypes.byref(m)))
        return m

    def __del__(self):
        if getattr(self, "handle", None) is not None:
            try:
                load_library().iris_group_pending_wait(self.handle, None)
            except Exception:
                pass


def distances(query, entry, device=None):
    """distances(&EncodedBits, &EncodedBits) -> [u16; 31] (src/lib.rs:82-87)."""
    dev = device or default_device()
    out = np.empty((1, ROTATIONS), np.uint16)
    with DistanceEngine(dev, query) as eng:
        eng.batch_process(out, [entry])
    return out[0]


def denominators(query, entry, device=None):
    """denominators(&Bits, &Bits) -> [u16; 31] (src/lib.rs:89-94)."""
    dev = device or default_device()
    out = np.empty((1, ROTATIONS), np.uint16)
    with MasksEngine(dev, query) as eng:
        eng.batch_process(out, [entry])
    return out[0]


# ====================================================================== resolver


def resolver_search(shares, denominators, index_base=0, device=None):
    """The resolver's aggregation (src/main.rs:597-621) on the GPU: wrapping sum
    of the participants' [n,31] u16 shares, decode_distance with the [n,31]
    denominators, min over rotations, strict-< lowest-index argmin -> Match."""
    dev = device or default_device()
    arrs = [_c(s, np.uint16) for s in shares]
    den = _c(denominators, np.uint16)
    n = den.shape[0]
    for a in arrs:
        if a.shape != (n, ROTATIONS):
            raise IrisError(-1, "shares and denominators must all be [n, 31] uint16")
    ptrs = (ctypes.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    m = Match()
    _check(load_library().iris_resolver_search_host(dev.handle, ptrs, len(arrs), _ptr(den), n, int(index_base),
                                                    ctypes.byref(m)))
    return m


def resolver_search_device(device, share_ptrs, denoms_ptr, n, index_base=0, dist_out_device=None):
    """Device-resident form: share_ptrs / denoms_ptr are device arrays of n*31 u16."""
    ptrs = (ctypes.c_void_p * len(share_ptrs))(*share_ptrs)
    m = Match()
    _check(load_library().iris_resolver_search(device.handle, ptrs, len(share_ptrs), ctypes.c_void_p(denoms_ptr), int(n),
                                               int(index_base), ctypes.c_void_p(dist_out_device or 0),
                                               ctypes.byref(m)))
    return m


def resolver_matches(device, share_ptrs, denoms_ptr, n, threshold, index_base=0, cap=None, out=None):
    """Every row of the resolver's aggregation whose decoded distance is below `threshold`
    (iris_resolver_matches; device arrays of n*31 u16; indices are index_base + row) ->
    (list[Match] in ascending index order, count); cap / out as in TemplateEngine.matches."""
    ptrs = (ctypes.c_void_p * len(share_ptrs))(*share_ptrs)
    f = load_library().iris_resolver_matches
    return _collect_matches(lambda o, c, cnt: f(device.handle, ptrs, len(share_ptrs), ctypes.c_void_p(denoms_ptr), int(n),
                                                int(index_base), float(threshold), o, c, cnt), cap, out, device)


def resolver_topk(device, share_ptrs, denoms_ptr, n, k, index_base=0):
    """The k closest rows of the resolver's aggregation, best first (iris_resolver_topk; device
    arrays of n*31 u16; indices are index_base + row) -> list[Match]."""
    ptrs = (ctypes.c_void_p * len(share_ptrs))(*share_ptrs)
    f = load_library().iris_resolver_topk
    return _collect_topk(lambda o, cnt: f(device.handle, ptrs, len(share_ptrs), ctypes.c_void_p(denoms_ptr), int(n),
                                          int(index_base), int(k), o, cnt), k)


def resolver_histogram(device, share_ptrs, denoms_ptr, n, nbins):
    """The distance distribution of the resolver's aggregation (iris_resolver_histogram; device
    arrays of n*31 u16) -> (bins: np.ndarray[nbins] of uint64, invalid: int); nbins is a power of
    two up to HIST_MAX_BINS, a distance above 1 joins the last bin."""
    ptrs = (ctypes.c_void_p * max(len(share_ptrs), 1))(*share_ptrs)
    nb = int(nbins)
    bins = np.zeros(nb if 0 < nb <= HIST_MAX_BINS else 1, np.uint64)
    invalid = ctypes.c_uint64(0)
    _check(load_library().iris_resolver_histogram(device.handle, ptrs, len(share_ptrs), ctypes.c_void_p(denoms_ptr), int(n),
                                                  nb, _ptr(bins), ctypes.addressof(invalid)))
    return bins, int(invalid.value)


def resolver_report(device, share_ptrs, denoms_ptr, n, threshold=None, cap=None, k=None, nbins=None, index_base=0):
    """Several of resolver_matches(), resolver_topk() and resolver_histogram() from ONE read of the
    share rows (iris_resolver_report; device arrays of n*31 u16) -> ReportResult, shaped like
    TemplateEngine.report: a part is asked for by its argument and is exactly what the sibling
    function returns."""
    ptrs = (ctypes.c_void_p * max(len(share_ptrs), 1))(*share_ptrs)
    f = load_library().iris_resolver_report
    return _report(lambda r: f(device.handle, ptrs, len(share_ptrs), ctypes.c_void_p(denoms_ptr), int(n), int(index_base), r),
                   device, threshold, cap, k, nbins,
                   lambda count: resolver_matches(device, share_ptrs, denoms_ptr, n, threshold, index_base, cap=count)[0])


# ====================================================================== arch plugin


def dot_bool_batch(a, b, device=None):
    """out[j, i] = dot_bool(a[i], b[j]) (src/arch/generic.rs:4-9)."""
    dev = device or default_device()
    a = _records(KIND_MASKS, a)
    b = _records(KIND_MASKS, b)
    out = np.empty((b.shape[0], a.shape[0]), np.uint16)
    _check(load_library().iris_dot_bool_batch(dev.handle, _ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out)))
    return out


def dot_u16_batch(a, b, device=None):
    """out[j, i] = dot_u16(a[i], b[j]) (src/arch/generic.rs:11-16)."""
    dev = device or default_device()
    a = _records(KIND_SHARES, a)
    b = _records(KIND_SHARES, b)
    out = np.empty((b.shape[0], a.shape[0]), np.uint16)
    _check(load_library().iris_dot_u16_batch(dev.handle, _ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out)))
    return out


def dot_bool(a, b, device=None):
    return int(dot_bool_batch([a], [b], device)[0, 0])


def dot_u16(a, b, device=None):
    return int(dot_u16_batch([a], [b], device)[0, 0])


def f64_bits(x):
    return int(np.float64(x).view(np.uint64))


__all__ = [
    "Bits", "EncodedBits", "Template", "encode", "decode_distance", "resolver_search", "resolver_search_device", "distances", "denominators", "MasksEngine",
    "DistanceEngine", "TemplateEngine", "TemplateBatchEngine", "Device", "Database", "Match", "merge_matches", "merge_topk", "resolver_topk", "resolver_histogram", "resolver_report", "TOPK_MAX", "HIST_MAX_BINS", "Report", "ReportResult", "BatchReport", "BatchReportResult", "REPORT_MATCHES", "REPORT_TOPK", "REPORT_HIST", "dot_bool", "dot_u16",
    "Group", "GroupDatabase", "GroupPendingSearch", "PendingMatches", "PendingReport", "PendingTopk",
    "dot_bool_batch", "dot_u16_batch", "IrisError", "load_library", "KIND_MASKS", "KIND_SHARES", "KIND_TEMPLATES",
    "LAYOUT_DEFAULT", "LAYOUT_LANES", "LAYOUT_TILES", "config",
    "ROTATIONS", "BITS", "LIMBS", "COLS", "ROWS",
]
