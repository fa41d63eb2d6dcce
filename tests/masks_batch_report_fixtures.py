"""Shared by the masks batch report tests (test_masks_batch_report_abi.py,
test_gpu_masks_batch_report.py): the raw call of iris_resolver_batch_report_masks into guarded
arrays, as batch_report_fixtures.raw_report makes the template call, and the check of every selected
part of every query against the CPU oracle alone (resolver_report_fixtures.check per query: an
Expected of test_gpu_matches.resolver_expected).  A resolver call numbers its rows from index_base:
Match.index = index_base + (record - first)."""
import ctypes

import numpy as np

import batch_report_fixtures as bf
import iris_hip as ih
import report_fixtures as rf
import resolver_report_fixtures as rrf
from batch_report_fixtures import SIZE, WORD
from report_fixtures import ALL, GUARD32, GUARD_BYTE, HIST, MATCHES, PAD, TOPK  # noqa: F401

NAME = "iris_resolver_batch_report_masks"
MULTI = [MATCHES | TOPK, MATCHES | HIST, TOPK | HIST, ALL]
SIBLINGS = ("iris_resolver_batch_matches_masks", "iris_resolver_batch_topk_masks", "iris_resolver_batch_histogram_masks")


def share_array(ptrs):
    """The `shares_device` argument of device pointers ptrs (None: NULL)."""
    return (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None


def raw_report(eng, db, first, n, ptrs, parts, nq=None, threshold=None, cap=None, k=None, nbins=None, index_base=0,
               expect_rc=0, null=(), reserved=0, nparts=None):
    """iris_resolver_batch_report_masks through ctypes.  The fields of unselected parts hold guard
    bytes (their pointers too), every array has guard records or words behind it, and all of them
    are checked after the call; a refused call must leave the struct, the arrays and the count
    arrays at their guard bytes.  eng / db None are NULL handles, ptrs None a NULL share array;
    null: names of pointer fields of selected parts handed in as NULL."""
    lib = ih.load_library()
    nq = eng.nq if nq is None else nq
    r = bf.guard_report()
    r.parts, r.reserved = parts, reserved
    marr = mcounts = tarr = tcounts = bins = invalid = None
    if parts & MATCHES:
        marr = rf.match_array(nq * cap)
        mcounts = np.full(nq + PAD, WORD, np.uint64)
        r.threshold, r.matches_cap = threshold, cap
        r.matches = ctypes.cast(marr, ctypes.POINTER(ih.Match)) if cap and "matches" not in null else None
        r.matches_counts = None if "matches_counts" in null else mcounts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    if parts & TOPK:
        tarr = rf.match_array(nq * max(k, 1))
        tcounts = np.full(nq + PAD, GUARD32, np.uint32)
        r.k = k
        r.topk = None if "topk" in null else ctypes.cast(tarr, ctypes.POINTER(ih.Match))
        r.topk_counts = None if "topk_counts" in null else tcounts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    if parts & HIST:
        bins = np.full(nq * max(nbins, 1) + PAD, WORD, np.uint64)
        invalid = np.full(nq + PAD, WORD, np.uint64)
        r.nbins = nbins
        r.bins = None if "bins" in null else bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
        r.invalid = None if "invalid" in null else invalid.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    before = bytes(r)
    nparts = (len(ptrs) if ptrs is not None else 0) if nparts is None else nparts
    rc = lib.iris_resolver_batch_report_masks(eng.handle if eng is not None else None, db.handle if db is not None else None,
                                              first, n, share_array(ptrs), nparts, index_base, ctypes.byref(r))
    out = bf.Result()
    out.rc, out.error = rc, lib.iris_last_error().decode(errors="replace")
    assert rc == expect_rc, (rc, out.error)
    assert bytes(r) == before, "the struct has no out fields: the call wrote it"
    if rc != 0:  # a refused call writes nothing
        for arr in (marr, tarr):
            assert arr is None or bytes(arr) == bytes([GUARD_BYTE]) * ctypes.sizeof(arr)
        for arr in (mcounts, bins, invalid):
            assert arr is None or (arr == WORD).all()
        assert tcounts is None or (tcounts == GUARD32).all()
        return out
    out.matches = out.matches_counts = out.topk = out.topk_counts = out.bins = out.invalid = None
    out.matches_bytes = out.topk_bytes = None
    if parts & MATCHES:
        assert (mcounts[nq:] == WORD).all(), "words past matches_counts[nq - 1] were written"
        out.matches_counts = [int(c) for c in mcounts[:nq]]
        raw = bytes(marr)
        out.matches, out.matches_bytes = [], []
        for q in range(nq):
            took = min(out.matches_counts[q], cap)
            lo, hi = q * cap * SIZE, (q + 1) * cap * SIZE
            assert raw[lo + took * SIZE:hi] == bytes([GUARD_BYTE]) * (hi - lo - took * SIZE), (q, "entries past the list")
            out.matches_bytes.append(raw[lo:lo + took * SIZE])
            out.matches.append([ih._copy_match(marr[q * cap + i]) for i in range(took)])
        assert raw[nq * cap * SIZE:] == bytes([GUARD_BYTE]) * (PAD * SIZE), "records past the last list were written"
    if parts & TOPK:
        assert (tcounts[nq:] == GUARD32).all(), "words past topk_counts[nq - 1] were written"
        out.topk_counts = [int(c) for c in tcounts[:nq]]
        raw = bytes(tarr)
        out.topk, out.topk_bytes = [], []
        for q in range(nq):
            took = out.topk_counts[q]
            assert took <= k
            lo, hi = q * k * SIZE, (q + 1) * k * SIZE
            assert raw[lo + took * SIZE:hi] == bytes([GUARD_BYTE]) * (hi - lo - took * SIZE), (q, "entries past the list")
            out.topk_bytes.append(raw[lo:lo + took * SIZE])
            out.topk.append([ih._copy_match(tarr[q * k + i]) for i in range(took)])
        assert raw[nq * k * SIZE:] == bytes([GUARD_BYTE]) * (PAD * SIZE), "records past the last list were written"
    if parts & HIST:
        assert (bins[nq * nbins:] == WORD).all() and (invalid[nq:] == WORD).all(), "words past the rows were written"
        out.bins = bins[:nq * nbins].reshape(nq, nbins).copy()
        out.invalid = [int(v) for v in invalid[:nq]]
    return out


def query_view(res, q, parts):
    """Query q of a raw_report result as the result of a single-query report (rrf.check's input)."""
    one = rf.Result()
    one.matches = one.matches_count = one.topk = one.topk_count = one.bins = one.invalid = None
    if parts & MATCHES:
        one.matches, one.matches_count = res.matches[q], res.matches_counts[q]
    if parts & TOPK:
        one.topk, one.topk_count = res.topk[q], res.topk_counts[q]
    if parts & HIST:
        one.bins, one.invalid = res.bins[q], res.invalid[q]
    return one


def check(exps, res, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0):
    """Every selected part of every query against the oracle's Expected of that query."""
    for q, e in enumerate(exps):
        rrf.check(e, query_view(res, q, parts), parts, first, n, threshold, cap, k, nbins, base)
    if not parts & MATCHES:
        assert res.matches is None and res.matches_counts is None
    if not parts & TOPK:
        assert res.topk is None and res.topk_counts is None
    if not parts & HIST:
        assert res.bins is None and res.invalid is None


def same(a, b, parts):
    """The selected parts of two raw_report results, byte for byte."""
    if parts & MATCHES:
        assert a.matches_counts == b.matches_counts and a.matches_bytes == b.matches_bytes
    if parts & TOPK:
        assert a.topk_counts == b.topk_counts and a.topk_bytes == b.topk_bytes
    if parts & HIST:
        assert a.bins.tobytes() == b.bins.tobytes() and a.invalid == b.invalid


def siblings(eng, db, first, n, ptrs, base, threshold, cap, k, nbins):
    """The three sibling batch calls, raw, as one result in raw_report's form (no guard checks)."""
    lib = ih.load_library()
    nq, arr = eng.nq, share_array(ptrs)
    marr = (ih.Match * max(nq * cap, 1))()
    mcounts = (ctypes.c_uint64 * nq)()
    assert lib.iris_resolver_batch_matches_masks(eng.handle, db.handle, first, n, arr, len(ptrs), base, threshold,
                                                 marr if cap else None, cap, mcounts) == 0
    tarr = (ih.Match * (nq * k))()
    tcounts = (ctypes.c_uint32 * nq)()
    assert lib.iris_resolver_batch_topk_masks(eng.handle, db.handle, first, n, arr, len(ptrs), base, k, tarr, tcounts) == 0
    bins = np.zeros((nq, nbins), np.uint64)
    invalid = np.zeros(nq, np.uint64)
    assert lib.iris_resolver_batch_histogram_masks(eng.handle, db.handle, first, n, arr, len(ptrs), nbins,
                                                   bins.ctypes.data_as(ctypes.c_void_p),
                                                   invalid.ctypes.data_as(ctypes.c_void_p)) == 0
    mraw, traw = bytes(marr), bytes(tarr)
    out = bf.Result()
    out.matches_counts = [int(c) for c in mcounts]
    out.matches_bytes = [mraw[q * cap * SIZE:(q * cap + min(int(mcounts[q]), cap)) * SIZE] for q in range(nq)]
    out.topk_counts = [int(c) for c in tcounts]
    out.topk_bytes = [traw[q * k * SIZE:(q * k + int(tcounts[q])) * SIZE] for q in range(nq)]
    out.bins, out.invalid = bins, [int(v) for v in invalid]
    return out
