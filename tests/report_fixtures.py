"""Shared by the report tests (test_report_abi.py, test_gpu_report.py): the raw call of
iris_template_report into guarded arrays, and the expected lists of a call from the CPU oracle alone.

Expected results of (threshold, k, nbins) over records [first, first + n) of an oracle Expected
(test_gpu_matches.Expected: per record the best rotation's num, den, k and f64 distance):
  matches   the records with a valid rotation whose f64 distance is below the threshold, ascending;
  top-k     the k first records with a valid rotation in the order (distance, index) -- distinct
            fractions of terms up to 12800 have distinct f64 quotients and equal ones equal
            quotients, so that is the exact fraction order;
  histogram hist_fixtures.expected on the distances."""
import ctypes

import numpy as np

import hist_fixtures as hf
import iris_hip as ih

MATCHES, TOPK, HIST = 1, 2, 4
ALL = MATCHES | TOPK | HIST
SUBSETS = [1, 2, 3, 4, 5, 6, 7]
GUARD = 0xA5A5A5A5A5A5A5A5
GUARD32 = 0xA5A5A5A5
GUARD_BYTE = 0xA5
PAD = 2  # guard records behind each list


def bits_of(x):
    return np.asarray(x, np.float64).view(np.uint64)


def guard_ptr(ctype):
    return ctypes.cast(ctypes.c_void_p(GUARD), ctypes.POINTER(ctype))


def match_array(count, fill=GUARD_BYTE):
    arr = (ih.Match * (count + PAD))()
    ctypes.memset(arr, fill, ctypes.sizeof(arr))
    return arr


def guard_report():
    """An iris_report_t whose every field holds guard bytes."""
    r = ih.Report()
    ctypes.memset(ctypes.byref(r), GUARD_BYTE, ctypes.sizeof(r))
    return r


class Result:
    """One raw call: rc, and for each selected part its outputs (None otherwise)."""


def raw_report(eng, db, first, n, parts, threshold=None, cap=None, k=None, nbins=None, index_base=0, fill=GUARD_BYTE,
               expect_rc=0):
    """iris_template_report through ctypes: the fields of unselected parts hold guard bytes (their
    pointers too), every array has guard words behind it, and both are checked after the call.
    cap=None: room for every record of the range."""
    lib = ih.load_library()
    r = guard_report()
    r.parts = parts
    marr = tarr = bins = None
    if parts & MATCHES:
        cap = n if cap is None else cap
        marr = match_array(cap, fill)
        r.threshold, r.matches_cap = threshold, cap
        r.matches = ctypes.cast(marr, ctypes.POINTER(ih.Match)) if cap else None
    if parts & TOPK:
        tarr = match_array(k, fill)
        r.k, r.topk = k, ctypes.cast(tarr, ctypes.POINTER(ih.Match))
    if parts & HIST:
        bins = np.full(nbins + 3, np.uint8(fill).astype(np.uint64) * np.uint64(0x0101010101010101), np.uint64)
        r.nbins, r.bins = nbins, bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    before = bytes(r)
    rc = lib.iris_template_report(eng.handle if eng is not None else None, db.handle if db is not None else None,
                                  first, n, index_base, ctypes.byref(r))
    out = Result()
    out.rc, out.error = rc, lib.iris_last_error().decode(errors="replace")
    assert rc == expect_rc, (rc, out.error)
    word = np.uint8(fill).astype(np.uint64) * np.uint64(0x0101010101010101)
    size = ctypes.sizeof(ih.Match)
    if rc != 0:  # a refused call writes nothing
        assert bytes(r) == before, "a refused call wrote the struct"
        assert marr is None or bytes(marr) == bytes([fill]) * ctypes.sizeof(marr)
        assert tarr is None or bytes(tarr) == bytes([fill]) * ctypes.sizeof(tarr)
        assert bins is None or (bins == word).all()
        return out
    # the in fields and the fields of unselected parts are as they were
    assert (r.parts, r.matches_cap if parts & MATCHES else None) == (parts, cap if parts & MATCHES else None)
    if not parts & MATCHES:
        assert r.matches_count == GUARD and r.matches_cap == GUARD and bits_of(r.threshold) == np.uint64(GUARD)
        assert ctypes.cast(r.matches, ctypes.c_void_p).value == GUARD
    if not parts & TOPK:
        assert r.topk_count == GUARD32 and r.k == GUARD32 and ctypes.cast(r.topk, ctypes.c_void_p).value == GUARD
    if not parts & HIST:
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
    """The records of [first, first + n) with a valid rotation, best first: distance, then index."""
    idx = np.arange(first, first + n)
    idx = idx[np.isfinite(e.dist[idx])]
    return idx[np.lexsort((idx, e.dist[idx]))]


def check_list(e, got, want, base):
    """A list of Match against record indices `want` of e: index, f64 bits, num, den, rotation."""
    assert len(got) == len(want), (len(got), len(want))
    for m, i in zip(got, want):
        i = int(i)
        assert m.index == base + i, (m, i)
        assert bits_of(m.distance) == bits_of(e.dist[i]), (m, i)
        assert (m.num, m.den, m.rotation, m.reserved) == (e.num[i], e.den[i], e.rot[i], 0), (m, i)


def check(e, res, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0):
    """Every selected part of a raw_report result against the oracle's Expected e."""
    if parts & MATCHES:
        hits = e.hits(threshold, first, n)
        assert res.matches_count == len(hits), (res.matches_count, len(hits))
        check_list(e, res.matches, hits if cap is None else hits[:cap], base)
    else:
        assert res.matches is None and res.matches_count is None
    if parts & TOPK:
        check_list(e, res.topk, order(e, first, n)[:k], base)
    else:
        assert res.topk is None
    if parts & HIST:
        want, want_invalid = hf.expected(e.dist, nbins, first, n)
        assert (res.bins == want).all() and res.invalid == want_invalid
        assert int(res.bins.sum()) + res.invalid == n
    else:
        assert res.bins is None and res.invalid is None


class SparseExpected:
    """Expected of a large database from its cached oracle distances: num, den and rotation are
    computed by the oracle for the records a list names, when it names them."""

    def __init__(self, query, templates, dist):
        self.query, self.templates, self.dist = query, templates, dist
        self.num, self.den, self.rot = _Lazy(self, 0), _Lazy(self, 1), _Lazy(self, 2)
        self._known = {}

    def hits(self, threshold, first=0, n=None):
        n = len(self.dist) - first if n is None else n
        idx = np.arange(first, first + n)
        return idx[np.isfinite(self.dist[idx]) & (self.dist[idx] < threshold)]

    def record(self, i):
        if i not in self._known:
            from oracle import oracle_c as oc
            from test_gpu_matches import Expected
            x = Expected(*oc.template_counts(self.query, self.templates[i:i + 1]))
            self._known[i] = (int(x.num[0]), int(x.den[0]), int(x.rot[0]))
        return self._known[i]


class _Lazy:
    def __init__(self, owner, field):
        self.owner, self.field = owner, field

    def __getitem__(self, i):
        return self.owner.record(int(i))[self.field]
