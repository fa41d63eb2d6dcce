"""Shared by the resolver report tests (test_resolver_report_abi.py, test_gpu_resolver_report.py):
the raw calls of iris_resolver_report and iris_resolver_report_masks into guarded arrays, and the
expected parts of a call from the CPU oracle alone.

Expected results of (threshold, k, nbins) over rows [first, first + n) of an oracle Expected
(test_gpu_matches.resolver_expected: per record the best rotation's uneq, den, k and f64 distance):
  matches   the records with a valid rotation whose f64 distance is below the threshold, ascending;
  top-k     the k first records with a valid rotation by exact fraction, then index -- order() sorts
            by the f64 distance and then proves, in integers, that this is the exact fraction order;
  histogram hist_fixtures.expected on the distances (a distance above 1 joins the last bin).
A resolver call numbers its rows from index_base: Match.index = index_base + (record - first)."""
import ctypes

import numpy as np

import hist_fixtures as hf
import iris_hip as ih
import report_fixtures as rf
from report_fixtures import ALL, GUARD, GUARD32, GUARD_BYTE, HIST, MATCHES, PAD, SUBSETS, TOPK  # noqa: F401

ROT = 31
NAMES = ("iris_resolver_report", "iris_resolver_report_masks")
MATCH_FIRST_ROOM = 1024  # kMatchFirstRoom: the records the first pass has room for under a smaller cap


def masks_call(eng, db, first, n, ptrs, index_base=0, nparts=None):
    """-> call(report pointer) of iris_resolver_report_masks; eng / db None are NULL handles."""
    lib = ih.load_library()
    arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    nparts = (len(ptrs) if ptrs is not None else 0) if nparts is None else nparts
    return lambda r: lib.iris_resolver_report_masks(eng.handle if eng is not None else None,
                                                    db.handle if db is not None else None, first, n, arr, nparts,
                                                    index_base, r)


def plain_call(device, ptrs, den_ptr, n, index_base=0, nparts=None):
    """-> call(report pointer) of iris_resolver_report; device None is a NULL handle."""
    lib = ih.load_library()
    arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs) if ptrs is not None else None
    nparts = (len(ptrs) if ptrs is not None else 0) if nparts is None else nparts
    return lambda r: lib.iris_resolver_report(device.handle if device is not None else None, arr, nparts,
                                              ctypes.c_void_p(den_ptr) if den_ptr else None, n, index_base, r)


def raw_report(call, n, parts, threshold=None, cap=None, k=None, nbins=None, fill=GUARD_BYTE, expect_rc=0):
    """One resolver report call through ctypes, as report_fixtures.raw_report makes the template
    call: the fields of unselected parts hold guard bytes (their pointers too), every array has guard
    words behind it, and both are checked after the call.  cap=None: room for every row."""
    lib = ih.load_library()
    r = rf.guard_report()
    r.parts = parts
    marr = tarr = bins = None
    if parts & MATCHES:
        cap = n if cap is None else cap
        marr = rf.match_array(cap, fill)
        r.threshold, r.matches_cap = threshold, cap
        r.matches = ctypes.cast(marr, ctypes.POINTER(ih.Match)) if cap else None
    if parts & TOPK:
        tarr = rf.match_array(k, fill)
        r.k, r.topk = k, ctypes.cast(tarr, ctypes.POINTER(ih.Match))
    word = np.uint8(fill).astype(np.uint64) * np.uint64(0x0101010101010101)
    if parts & HIST:
        bins = np.full(nbins + 3, word, np.uint64)
        r.nbins, r.bins = nbins, bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    before = bytes(r)
    rc = call(ctypes.byref(r))
    out = rf.Result()
    out.rc, out.error = rc, lib.iris_last_error().decode(errors="replace")
    assert rc == expect_rc, (rc, out.error)
    size = ctypes.sizeof(ih.Match)
    if rc != 0:  # a refused call writes nothing
        assert bytes(r) == before, "a refused call wrote the struct"
        assert marr is None or bytes(marr) == bytes([fill]) * ctypes.sizeof(marr)
        assert tarr is None or bytes(tarr) == bytes([fill]) * ctypes.sizeof(tarr)
        assert bins is None or (bins == word).all()
        return out
    # the in fields and the fields of unselected parts are as they were
    assert r.parts == parts
    if parts & MATCHES:
        assert r.matches_cap == cap and rf.bits_of(r.threshold) == rf.bits_of(threshold)
    else:
        assert r.matches_count == GUARD and r.matches_cap == GUARD and rf.bits_of(r.threshold) == np.uint64(GUARD)
        assert ctypes.cast(r.matches, ctypes.c_void_p).value == GUARD
    if parts & TOPK:
        assert r.k == k
    else:
        assert r.topk_count == GUARD32 and r.k == GUARD32 and ctypes.cast(r.topk, ctypes.c_void_p).value == GUARD
    if parts & HIST:
        assert r.nbins == nbins
    else:
        assert r.invalid == GUARD and r.nbins == GUARD32 and ctypes.cast(r.bins, ctypes.c_void_p).value == GUARD
    out.matches = out.matches_count = out.topk = out.topk_count = out.bins = out.invalid = None
    out.matches_bytes = out.topk_bytes = None
    if parts & MATCHES:
        out.matches_count = int(r.matches_count)
        took = min(out.matches_count, cap)
        raw = bytes(marr)
        assert raw[took * size:] == bytes([fill]) * (len(raw) - took * size), "records past the list were written"
        out.matches_bytes = raw[:took * size]
        out.matches = [ih._copy_match(marr[i]) for i in range(took)]
    if parts & TOPK:
        out.topk_count = int(r.topk_count)
        assert out.topk_count <= k
        raw = bytes(tarr)
        assert raw[k * size:] == bytes([fill]) * (PAD * size), "records past the k entries were written"
        out.topk_bytes = raw[:out.topk_count * size]
        out.topk = [ih._copy_match(tarr[i]) for i in range(out.topk_count)]
    if parts & HIST:
        assert (bins[nbins:] == word).all(), "words past the bins were written"
        out.bins, out.invalid = bins[:nbins].copy(), int(r.invalid)
    return out


def order(e, first, n):
    """The records of [first, first + n) with a valid rotation, best first: exact fraction, then index.
    Sorted by (f64 distance, index); the integer cross products of neighbours then prove that equal
    distances are equal fractions and smaller distances smaller fractions (terms below 2^16)."""
    idx = np.arange(first, first + n)
    idx = idx[e.den[idx] != 0]
    idx = idx[np.lexsort((idx, e.dist[idx]))]
    a, b = idx[:-1], idx[1:]
    left, right = e.num[a] * e.den[b], e.num[b] * e.den[a]
    assert (left <= right).all() and ((left == right) == (e.dist[a] == e.dist[b])).all()
    assert (a[left == right] < b[left == right]).all()
    return idx


def check(e, res, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0):
    """Every selected part of a raw_report result against the oracle's Expected e."""
    if parts & MATCHES:
        hits = e.hits(threshold, first, n)
        assert res.matches_count == len(hits), (res.matches_count, len(hits))
        rf.check_list(e, res.matches, hits if cap is None else hits[:cap], base - first)
        assert [m.index for m in res.matches] == sorted(m.index for m in res.matches)
    else:
        assert res.matches is None and res.matches_count is None
    if parts & TOPK:
        rf.check_list(e, res.topk, order(e, first, n)[:k], base - first)
    else:
        assert res.topk is None
    if parts & HIST:
        want, want_invalid = hf.expected(e.dist, nbins, first, n)
        assert (res.bins == want).all() and res.invalid == want_invalid
        assert int(res.bins.sum()) + res.invalid == n
    else:
        assert res.bins is None and res.invalid is None
