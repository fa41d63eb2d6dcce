"""Shared by the template batch report tests (test_template_batch_report_abi.py,
test_gpu_template_batch_report.py): the raw call of iris_template_batch_report into guarded arrays,
and the check of every selected part against the CPU oracle alone (report_fixtures.check_list and
order, hist_fixtures.expected; per query an Expected of test_gpu_template_batch_matches or a
SparseExpected of report_fixtures)."""
import ctypes

import numpy as np

import hist_fixtures as hf
import iris_hip as ih
import report_fixtures as rf
from report_fixtures import ALL, GUARD, GUARD32, GUARD_BYTE, HIST, MATCHES, PAD, TOPK  # noqa: F401

NAME = "iris_template_batch_report"
MULTI = [MATCHES | TOPK, MATCHES | HIST, TOPK | HIST, ALL]
FIELDS = ["parts", "k", "nbins", "reserved", "threshold", "matches", "matches_cap", "matches_counts", "topk",
          "topk_counts", "bins", "invalid"]
WORD = np.uint64(GUARD)
SIZE = ctypes.sizeof(ih.Match)


def guard_report():
    """An iris_batch_report_t whose every field holds guard bytes."""
    r = ih.BatchReport()
    ctypes.memset(ctypes.byref(r), GUARD_BYTE, ctypes.sizeof(r))
    return r


class Result:
    """One raw call: rc, error, and for each selected part its per-query outputs (None otherwise)."""


def raw_report(eng, db, first, n, parts, nq=None, threshold=None, cap=None, k=None, nbins=None, index_base=0,
               expect_rc=0, null=(), reserved=0):
    """iris_template_batch_report through ctypes.  The fields of unselected parts hold guard bytes
    (their pointers too), every array has guard records or words behind it, and all of them are
    checked after the call; a refused call must leave the struct, the arrays and the count arrays
    at their guard bytes.  null: names of pointer fields of selected parts handed in as NULL."""
    lib = ih.load_library()
    nq = eng.nq if nq is None else nq
    r = guard_report()
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
    rc = lib.iris_template_batch_report(eng.handle if eng is not None else None, db.handle if db is not None else None,
                                        first, n, index_base, ctypes.byref(r))
    out = Result()
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


def check(exps, res, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0):
    """Every selected part of a raw_report result, per query, against the oracle's Expected of that
    query: the count, the lowest-index prefix in ascending order, the top-k in (exact fraction,
    index) order, the bins against np.bincount of the binned distances, sum(bins) + invalid == n,
    and the prefix sums of the bins against the match totals at threshold j / nbins."""
    for q, e in enumerate(exps):
        if parts & MATCHES:
            hits = e.hits(threshold, first, n)
            assert res.matches_counts[q] == len(hits), (q, res.matches_counts[q], len(hits))
            rf.check_list(e, res.matches[q], hits[:cap], base)
        if parts & TOPK:
            rf.check_list(e, res.topk[q], rf.order(e, first, n)[:k], base)
        if parts & HIST:
            want, want_invalid = hf.expected(e.dist, nbins, first, n)
            assert (res.bins[q] == want).all() and res.invalid[q] == want_invalid, q
            assert int(res.bins[q].sum()) + res.invalid[q] == n, q
            prefix = np.concatenate([[0], np.cumsum(res.bins[q])])
            for j in sorted({0, 1, nbins // 2, nbins - 1} & set(range(nbins))):
                assert prefix[j] == len(e.hits(j / nbins, first, n)), (q, j)
    if not parts & MATCHES:
        assert res.matches is None and res.matches_counts is None
    if not parts & TOPK:
        assert res.topk is None and res.topk_counts is None
    if not parts & HIST:
        assert res.bins is None and res.invalid is None
