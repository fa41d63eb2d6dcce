"""The life of a pending handle: what iris_template_search_async,
iris_template_matches_async and iris_template_topk_async share from submission to wait -- the
refusal of a wait of the wrong kind, the pools of pinned slots and device buffers past their first
block, the three kinds in one pipeline, and the release of a handle whose wait was refused for an
argument.  Every result equals the blocking call's for the same arguments field by field (the
distance as its f64 bit pattern).

One range of 64 records throughout, so no pass takes a place in the sharing ring; eight queries,
each a perturbed copy of a record of its own.  The file's 7 tests take about 2 s on an MI355X."""
import ctypes

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc

gpu = pytest.mark.gpu
N = 64
E_ARG = -1
SENTINEL = (0xABCDEF, 77, 78, 79, -5.0)
CALLS = {"search": ("iris_template_search_async", "iris_pending_wait"),
         "matches": ("iris_template_matches_async", "iris_pending_matches_wait"),
         "topk": ("iris_template_topk_async", "iris_pending_topk_wait")}
THRESHOLDS = [0.01, 0.3, 0.46, 0.49, 0.7]
CAPS = [4, 0, 64, 1, 9]
KS = [64, 1, 7, 64, 1, 16]


def fields(m):
    return (int(np.float64(m.distance).view(np.uint64)), m.index, m.num, m.den, m.rotation)


def rebased(ms, by):
    return [(d, i + by, num, den, rot) for d, i, num, den, rot in ms]


@pytest.fixture(scope="module")
def recs():
    return oc.gen_templates(9494, 0, N)


@pytest.fixture(scope="module")
def queries(recs):
    qs = []
    for i in range(8):
        q = recs[7 * i + 2].copy()
        q[1 + i] ^= np.uint64(0x00FF00FF00FF00FF)
        qs.append(q)
    return qs


class Blocking:
    """The blocking calls' results at index_base 0, computed once per argument set."""

    def __init__(self, engines, db):
        self.engines, self.db, self.memo = engines, db, {}

    def _get(self, key, call):
        if key not in self.memo:
            self.memo[key] = call()
        return self.memo[key]

    def search(self, qi, base=0):
        m = self._get(("s", qi), lambda: fields(self.engines[qi].search(self.db, 0, N)))
        return rebased([m], base)[0]

    def matches(self, qi, thr, cap, base=0):
        ms, count = self._get(("m", qi, thr, cap), lambda: self.engines[qi].matches(self.db, thr, 0, N, cap=cap))
        return rebased([fields(m) for m in ms], base), count

    def topk(self, qi, k, base=0):
        ms = self._get(("t", qi, k), lambda: [fields(m) for m in self.engines[qi].topk(self.db, k, 0, N)])
        return rebased(ms, base)


def got_matches(res):
    return [fields(m) for m in res[0]], res[1]


def sentinels(count):
    out = (ih.Match * count)()
    for m in out:
        m.index, m.num, m.den, m.rotation, m.distance = SENTINEL
    return out


def untouched(out):
    return all((m.index, m.num, m.den, m.rotation, m.distance) == SENTINEL for m in out)


def raw_submit(lib, kind, e, db, arg=None, base=0):
    h = ctypes.c_void_p()
    if kind == "search":
        rc = lib.iris_template_search_async(e.handle, db.handle, 0, N, base, ctypes.byref(h))
    elif kind == "matches":
        rc = lib.iris_template_matches_async(e.handle, db.handle, 0, N, base, arg[0], arg[1], ctypes.byref(h))
    else:
        rc = lib.iris_template_topk_async(e.handle, db.handle, 0, N, base, arg, ctypes.byref(h))
    assert rc == 0 and h.value
    return h


def raw_wait(lib, kind, h, out, count):
    if kind == "search":
        return lib.iris_pending_wait(h, out)
    f = lib.iris_pending_matches_wait if kind == "matches" else lib.iris_pending_topk_wait
    return f(h, out, ctypes.byref(count) if count is not None else None)


@gpu
def test_wrong_kind_waits_leave_the_handle_alive(device, recs, queries):
    """One pending of each kind; each handle goes to both waits that do not serve it -- refused with
    a message that names the submission and the wait that does, nothing written -- and then to its
    own, which returns what the blocking call returns."""
    lib = ih.load_library()
    with ih.Database(device, ih.KIND_TEMPLATES, N) as db, ih.TemplateEngine(device, queries[0]) as e:
        db.append(recs)
        want = Blocking([e], db)
        args = {"search": None, "matches": (0.49, 4), "topk": 4}
        hs = {kind: raw_submit(lib, kind, e, db, args[kind], base=3) for kind in CALLS}
        for kind, h in hs.items():
            for wait in CALLS:
                if wait == kind:
                    continue
                out = sentinels(4)
                count = None if wait == "search" else (ctypes.c_uint64 if wait == "matches" else ctypes.c_uint32)(77)
                assert raw_wait(lib, wait, h, out, count) == E_ARG
                assert lib.iris_last_error().decode() == "pending of %s: %s waits for it" % CALLS[kind]
                assert untouched(out) and (count is None or count.value == 77)
        m = ih.Match()
        assert lib.iris_pending_wait(hs["search"], ctypes.byref(m)) == 0
        assert fields(m) == want.search(0, 3)
        out, c64 = sentinels(4), ctypes.c_uint64(77)
        assert raw_wait(lib, "matches", hs["matches"], out, c64) == 0
        wl, wc = want.matches(0, 0.49, 4, 3)
        assert ([fields(x) for x in out[:len(wl)]], c64.value) == (wl, wc) and untouched(out[len(wl):])
        out, c32 = sentinels(4), ctypes.c_uint32(77)
        assert raw_wait(lib, "topk", hs["topk"], out, c32) == 0
        assert c32.value == 4 and [fields(x) for x in out] == want.topk(0, 4, 3)


@gpu
@pytest.mark.parametrize("layout", ["tiles", "lanes"])
def test_pools_past_one_block(layout, recs, queries):
    """257 searches (a block of result slots is 256), 65 match handles (64) and 33 top-k handles
    (32) outstanding at once on a device of their own, waited for in submission order.  A top-k
    handle of k = 1 is returned first: its buffer is the smallest there is, 4096 bytes, and the
    k = 64 submissions after it (on the LANES database 4 lists and a spare one, 7680 bytes) find
    it too small and take a pair that has no buffer yet; after the waits three more find buffers
    of both sizes."""
    with ih.Device(0) as dev, ih.Database(dev, ih.KIND_TEMPLATES, N, getattr(ih, "LAYOUT_" + layout.upper())) as db:
        db.append(recs)
        engines = [ih.TemplateEngine(dev, q) for q in queries]
        try:
            want = Blocking(engines, db)
            assert [fields(m) for m in engines[3].topk_async(db, 1, 0, N).wait()] == want.topk(3, 1)
            pend = []
            for i in range(257):
                pend.append(("s", i % 8, None, engines[i % 8].search_async(db, 0, N, index_base=i)))
            for i in range(65):
                arg = (THRESHOLDS[i % 5], CAPS[i // 5 % 5])
                pend.append(("m", i % 8, arg, engines[i % 8].matches_async(db, arg[0], 0, N, index_base=i, cap=arg[1])))
            for i in range(33):
                pend.append(("t", i % 8, KS[i % 6], engines[i % 8].topk_async(db, KS[i % 6], 0, N, index_base=i)))
            for j, k in enumerate([64, 1, 64]):
                pend.append(("t", j, k, None))
            bases = list(range(257)) + list(range(65)) + list(range(33)) + [0, 0, 0]
            for (kind, qi, arg, p), base in zip(pend, bases):
                if kind == "s":
                    assert fields(p.wait()) == want.search(qi, base)
                elif kind == "m":
                    assert got_matches(p.wait()) == want.matches(qi, arg[0], arg[1], base)
                else:
                    p = p or engines[qi].topk_async(db, arg, 0, N)
                    assert [fields(m) for m in p.wait()] == want.topk(qi, arg, base)
            assert len({want.search(qi) for qi in range(8)}) == 8  # eight different winners
            assert {want.matches(qi, 0.01, 4)[1] for qi in range(8)} == {1} and want.matches(0, 0.7, 4)[1] == N
        finally:
            for e in engines:
                e.close()


@gpu
def test_mixed_kinds_in_one_pipeline(device, recs, queries):
    """search, matches, top-k, matches, top-k, search submitted with nothing waited for, every
    engine destroyed at once, and waited for in reverse order."""
    plan = [("s", 0, None), ("m", 1, (0.49, 9)), ("t", 2, 64), ("m", 3, (0.01, 1)), ("t", 4, 1), ("s", 5, None)]
    with ih.Database(device, ih.KIND_TEMPLATES, N) as db:
        db.append(recs)
        pend = []
        for i, (kind, qi, arg) in enumerate(plan):
            with ih.TemplateEngine(device, queries[qi]) as e:
                pend.append(e.search_async(db, 0, N, index_base=i) if kind == "s" else
                            e.matches_async(db, arg[0], 0, N, index_base=i, cap=arg[1]) if kind == "m" else
                            e.topk_async(db, arg, 0, N, index_base=i))
        got = {i: pend[i].wait() for i in reversed(range(len(plan)))}
        engines = [ih.TemplateEngine(device, q) for q in queries]
        try:
            want = Blocking(engines, db)
            for i, (kind, qi, arg) in enumerate(plan):
                if kind == "s":
                    assert fields(got[i]) == want.search(qi, i)
                elif kind == "m":
                    assert got_matches(got[i]) == want.matches(qi, arg[0], arg[1], i)
                else:
                    assert [fields(m) for m in got[i]] == want.topk(qi, arg, i)
        finally:
            for e in engines:
                e.close()


@gpu
@pytest.mark.parametrize("kind", ["matches", "topk"])
def test_release_after_an_argument_error(kind, recs, queries):
    """A wait refused for `count == NULL` still consumes its handle: the same query submitted again
    on the same device gives the blocking call's result, and the device -- every other handle
    destroyed -- closes, its holds released one for one."""
    lib = ih.load_library()
    dev = ih.Device(0)
    with ih.Database(dev, ih.KIND_TEMPLATES, N) as db, ih.TemplateEngine(dev, queries[6]) as e:
        db.append(recs)
        arg = (0.49, 4) if kind == "matches" else 5
        h = raw_submit(lib, kind, e, db, arg)
        out = sentinels(5)
        assert raw_wait(lib, kind, h, out, None) == E_ARG
        assert lib.iris_last_error().decode() == "count is NULL" and untouched(out)
        want = Blocking({6: e}, db)
        if kind == "matches":
            assert got_matches(e.matches_async(db, 0.49, 0, N, cap=4).wait()) == want.matches(6, 0.49, 4)
        else:
            assert [fields(m) for m in e.topk_async(db, 5, 0, N).wait()] == want.topk(6, 5)
    assert lib.iris_device_close(dev.handle) == 0
    dev.handle = None
