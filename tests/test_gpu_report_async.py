"""Pipelined reports (iris_template_report_async): a report pass that is still
streaming the database also feeds the sinks of the report pass submitted after it -- its match
list, its k closest records, its histogram, whichever of them it asks for -- workgroup by workgroup.
Whatever is shared, every result equals the blocking report() of the same query on the same device
field by field (distances as f64 bit patterns; the arrays byte for byte, their guard bytes past the
counts and those of unselected parts included) and, once per test, the CPU oracle: distances sorted
by (distance, index), the threshold filter, floor(d * nbins) bins.

The fixtures are tests/test_gpu_search_share.py's: 86 tiles of generated records, four generated
queries, near() records at distance 0.0017 to 0.0028 of their query while no generated record is
closer than 0.4576 to any of them.  The forced tests pin the 4-tiles-per-wave form on small ranges
and hold every pass back behind a 2-ms spin, so the next registration lands before the pass starts
and every workgroup carries the guest: `report_shared` (registrations, tile groups carried) is then
exact, and the histogram's sum shows that every record was counted once.
The file's 46 tests take 3.7 s together on an MI355X."""
import ctypes

import numpy as np
import pytest

import iris_hip as ih
import report_fixtures as rf
from oracle import oracle_c as oc
from test_gpu_search_share import FORCED, NDB, TILE, grid_of, near, queries, recs, span  # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
BASE = 3
M, T, H, ALL = rf.MATCHES, rf.TOPK, rf.HIST, rf.ALL
WORD = np.uint64(rf.GUARD)
BIG_TILES = 16 * 17 + 3  # 18 workgroups, 72 lists: two merge levels (kTopkFanIn = 64)
BIG_NDB = (BIG_TILES + 3) * TILE
MSIZE = ctypes.sizeof(ih.Match)


class Spec:
    """The in scalars of one report: parts, threshold, matches_cap, k, nbins."""

    def __init__(self, parts, thr=0.3, cap=8, k=5, nbins=64):
        self.parts, self.thr, self.cap, self.k, self.nbins = parts, thr, cap, k, nbins

    def __repr__(self):
        return f"Spec({self.parts}, {self.thr}, {self.cap}, {self.k}, {self.nbins})"


HOST = Spec(ALL, 0.3, 8, 5, 64)
GUEST = Spec(ALL, 0.01, 8, 64, 1024)


def struct_of(spec, arrays=True):
    """A guard-filled iris_report_t with spec's in scalars; arrays: guarded arrays of the selected
    parts (else their pointers keep the guard value: the submission must not read them)."""
    r = rf.guard_report()
    r.parts = spec.parts
    marr = tarr = bins = None
    if spec.parts & M:
        r.threshold, r.matches_cap = spec.thr, spec.cap
        if arrays:
            marr = rf.match_array(spec.cap)
            r.matches = ctypes.cast(marr, ctypes.POINTER(ih.Match)) if spec.cap else None
    if spec.parts & T:
        r.k = spec.k
        if arrays:
            tarr = rf.match_array(spec.k)
            r.topk = ctypes.cast(tarr, ctypes.POINTER(ih.Match))
    if spec.parts & H:
        r.nbins = spec.nbins
        if arrays:
            bins = np.full(spec.nbins + 3, WORD, np.uint64)
            r.bins = bins.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    return r, (marr, tarr, bins)


def mfields(m):
    return (int(np.float64(m.distance).view(np.uint64)), m.index, m.num, m.den, m.rotation, m.reserved)


def harvest(r, arrs, spec):
    """What a successful call left -> a dict two calls are compared by.  Checks on the way that the
    fields of unselected parts and everything past the counts still hold guard bytes."""
    marr, tarr, bins = arrs
    out = {"parts": r.parts}
    assert r.parts == spec.parts
    if spec.parts & M:
        assert r.matches_cap == spec.cap and rf.bits_of(r.threshold) == rf.bits_of(spec.thr)
        took = min(int(r.matches_count), spec.cap)
        raw = bytes(marr)
        assert raw[took * MSIZE:] == bytes([rf.GUARD_BYTE]) * (len(raw) - took * MSIZE), "records past the list were written"
        out["matches_count"], out["matches"] = int(r.matches_count), [mfields(marr[i]) for i in range(took)]
        out["matches_bytes"] = raw
    else:
        assert r.matches_count == rf.GUARD and r.matches_cap == rf.GUARD and rf.bits_of(r.threshold) == WORD
        assert ctypes.cast(r.matches, ctypes.c_void_p).value == rf.GUARD
    if spec.parts & T:
        assert r.k == spec.k and r.topk_count <= spec.k
        raw = bytes(tarr)
        assert raw[r.topk_count * MSIZE:] == bytes([rf.GUARD_BYTE]) * (len(raw) - r.topk_count * MSIZE), \
            "records past the count were written"
        out["topk"], out["topk_bytes"] = [mfields(tarr[i]) for i in range(r.topk_count)], raw
    else:
        assert r.topk_count == rf.GUARD32 and r.k == rf.GUARD32 and ctypes.cast(r.topk, ctypes.c_void_p).value == rf.GUARD
    if spec.parts & H:
        assert r.nbins == spec.nbins and (bins[spec.nbins:] == WORD).all(), "words past the bins were written"
        out["bins"], out["invalid"] = bins[:spec.nbins].tobytes(), int(r.invalid)
    else:
        assert r.invalid == rf.GUARD and r.nbins == rf.GUARD32 and ctypes.cast(r.bins, ctypes.c_void_p).value == rf.GUARD
    return out


def bins_of(res, spec):
    return np.frombuffer(res["bins"], np.uint64)


def blocking(dev, db, q, spec, first, cnt, base=BASE):
    r, arrs = struct_of(spec)
    with ih.TemplateEngine(dev, q) as e:
        rc = ih.load_library().iris_template_report(e.handle, db.handle, first, cnt, base, ctypes.byref(r))
    assert rc == 0, ih.load_library().iris_last_error()
    return harvest(r, arrs, spec)


def submit_one(e, db, spec, first, cnt, base=BASE):
    """One submission through the C ABI -> the handle.  The struct's pointers and out fields hold
    guard bytes: the submission reads neither and writes nothing."""
    lib = ih.load_library()
    r, _ = struct_of(spec, arrays=False)
    before = bytes(r)
    h = ctypes.c_void_p()
    rc = lib.iris_template_report_async(e.handle, db.handle, first, cnt, base, ctypes.byref(r), ctypes.byref(h))
    assert rc == 0, lib.iris_last_error()
    assert bytes(r) == before and h.value
    return h


def submit(dev, db, items, first, cnt, base=BASE):
    """The (query, spec) items' report passes back to back, every engine destroyed at once."""
    pend = []
    for q, spec in items:
        with ih.TemplateEngine(dev, q) as e:
            pend.append(submit_one(e, db, spec, first, cnt, base))
    return pend


def wait(h, spec):
    r, arrs = struct_of(spec)
    rc = ih.load_library().iris_pending_report_wait(h, ctypes.byref(r))
    assert rc == 0, ih.load_library().iris_last_error()
    return harvest(r, arrs, spec)


def check_oracle(res, spec, q, data, first, cnt, base=BASE):
    d = oc.template_distances(q, data[first:first + cnt])
    fin = np.isfinite(d)
    if spec.parts & M:
        hits = np.nonzero(fin & (d < spec.thr))[0]
        assert res["matches_count"] == len(hits)
        assert [m[:2] for m in res["matches"]] == [(int(d[i].view(np.uint64)), int(i) + first + base) for i in hits[:spec.cap]]
    if spec.parts & T:
        order = [int(i) for i in np.lexsort((np.arange(cnt), d)) if fin[i]][:spec.k]
        assert [m[:2] for m in res["topk"]] == [(int(d[i].view(np.uint64)), i + first + base) for i in order]
    if spec.parts & H:
        b = np.minimum(np.floor(d[fin] * spec.nbins).astype(np.int64), spec.nbins - 1)
        assert (bins_of(res, spec) == np.bincount(b, minlength=spec.nbins).astype(np.uint64)).all()
        assert res["invalid"] == int((~fin).sum())


def check_sum(res, spec, cnt):
    if spec.parts & H:
        assert int(bins_of(res, spec).sum()) + res["invalid"] == cnt


def shared_stats(dev):
    return tuple((s[0], s[2]) for s in (dev.kernel_stats(n) for n in ("report_shared", "topk_shared", "match_shared", "search_shared")))


def only_report(regs, carried):
    return ((regs, carried), (0, 0), (0, 0), (0, 0))


# ---------------------------------------------------------------- 1. full sharing


@gpu
@pytest.mark.parametrize("ntiles", [1, 17, 16 * 5 + 3])
def test_forced_full_sharing(hooked_device, recs, queries, ntiles):
    """Two different queries back to back, all three parts each with different arguments: the first
    pass carries the second in every workgroup.  The guest's moving near record lies in the first
    tile group, the last one, and the last (clamped, partial) tile in turn."""
    dev = hooked_device(**FORCED)
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    last_tile = first // TILE + ntiles - 1
    sites = sorted({first + 1, min(first + cnt - 1, last_tile * TILE - 9) if ntiles > 1 else first + 2,
                    first + cnt - 1})
    hits_a = sorted({first + 3, first + min(cnt - 1, 11), first + cnt // 2})
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        data = recs.copy()
        for j, i in enumerate(hits_a):
            data[i] = near(qa, limb=3 + j)
        data[first + 4] = near(qb, limb=6)
        data[first - 1] = data[first + cnt + 1] = qb  # exact copies just outside the range are in no part
        data[first - 2] = data[first + cnt] = qa
        for j, site in enumerate(sites):
            cur = data.copy()
            cur[site] = near(qb, limb=5)
            db.truncate(0)
            db.append(cur)
            dev.reset_stats()
            pa, pb = submit(dev, db, [(qa, HOST), (qb, GUEST)], first, cnt)
            ra, rb = wait(pa, HOST), wait(pb, GUEST)
            stats = shared_stats(dev)
            print(f"ntiles={ntiles} site={site} report_shared={stats[0]} grid={grid_of(ntiles)}")
            assert stats == only_report(1, grid_of(ntiles))
            check_sum(ra, HOST, cnt)
            check_sum(rb, GUEST, cnt)
            assert [m[1] for m in ra["matches"]] == [i + BASE for i in hits_a] and ra["matches_count"] == len(hits_a)
            assert [m[1] for m in rb["matches"]] == sorted(i + BASE for i in {first + 4, site}) and rb["matches_count"] == 2
            assert len(ra["topk"]) == 5 and len(rb["topk"]) == min(64, cnt)
            assert ra == blocking(dev, db, qa, HOST, first, cnt)
            assert rb == blocking(dev, db, qb, GUEST, first, cnt)
            if j == 0:
                check_oracle(ra, HOST, qa, cur, first, cnt)
                check_oracle(rb, GUEST, qb, cur, first, cnt)


# ---------------------------------------------------------------- 2. every subset


@gpu
@pytest.mark.parametrize("role", ["guest", "host"])
@pytest.mark.parametrize("parts", rf.SUBSETS)
def test_every_subset(hooked_device, recs, queries, parts, role):
    """Each non-empty `parts` as guest under an all-parts host and as host over an all-parts guest,
    17 tiles: the arrays and fields of an unselected part keep their guard bytes (harvest), and so
    do the entries past the counts."""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    qa, qb = queries[0], queries[1]
    sub = Spec(parts, 0.25, 3, 9, 256)
    sa, sb = (HOST, sub) if role == "guest" else (sub, GUEST)
    data = recs.copy()
    for j, i in enumerate([first + 2, first + 16 * TILE + 1, first + cnt - 2, first + 200]):
        data[i] = near(qa, limb=3 + j)
        data[i + 1] = near(qb, limb=9 + j)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, sa), (qb, sb)], first, cnt)
        ra, rb = wait(pa, sa), wait(pb, sb)
        assert shared_stats(dev) == only_report(1, grid_of(17))
        check_sum(ra, sa, cnt)
        check_sum(rb, sb, cnt)
        if sa.parts & M:
            assert ra["matches_count"] == 4
        if sb.parts & M:
            assert rb["matches_count"] == 4
        assert ra == blocking(dev, db, qa, sa, first, cnt)
        assert rb == blocking(dev, db, qb, sb, first, cnt)
        check_oracle(ra if role == "host" else rb, sub, qa if role == "host" else qb, data, first, cnt)


# ---------------------------------------------------------------- 3. mixed groups


@gpu
def test_mixed_groups(hooked_device, recs, queries):
    """IRIS_SEARCH_SHARE_EVEN=1, 83 tiles, A, B and C back to back: A carries B in even tile groups,
    B -- a guest itself -- computes its odd groups and carries C there, C computes the even ones:
    one pass has carrying, solo and, in the guest's launch, skipped groups.  A threshold every
    record passes with cap = 0: the totals are the range, the histograms add up to it."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qs = [queries[0], queries[1], queries[2]]
    tile0 = first // TILE
    data = recs.copy()
    for qi, q in enumerate(qs):
        for g in range(6):  # a near record in every tile group, an equal pair across an even and an odd one
            data[(tile0 + 16 * g + 2 + qi) * TILE + 9 + g] = near(q, limb=4 if g < 2 else 10 + g)
    specs = [Spec(ALL, 1.0, 0, 4, 1024), Spec(ALL, 1.0, 0, 8, 64), Spec(ALL, 1.0, 0, 64, 1)]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, list(zip(qs, specs)), first, cnt)
        got = [wait(p, s) for p, s in zip(pend, specs)]
        assert shared_stats(dev) == only_report(2, 6)
        for j, (r, q, s) in enumerate(zip(got, qs, specs)):
            assert r["matches_count"] == cnt and r["matches"] == []
            check_sum(r, s, cnt)
            assert r["invalid"] == 0 and len({m[1] for m in r["topk"]}) == s.k
            assert r == blocking(dev, db, q, s, first, cnt)
            if j == 1:
                check_oracle(r, s, q, data, first, cnt)


# ---------------------------------------------------------------- 4. two merge levels


@pytest.fixture(scope="module")
def big_recs():
    return oc.gen_templates(9393, 0, BIG_NDB)


@gpu
def test_more_than_one_merge_level(hooked_device, big_recs, queries):
    """275 tiles: 18 workgroups and 72 lists per query, above the merge's fan-in of 64, so host and
    guest of one shared pass are folded in two levels, k = 64 for both."""
    dev = hooked_device(**FORCED)
    first, cnt = TILE + 5, BIG_TILES * TILE - 5 - 7
    assert grid_of(BIG_TILES) == 18
    qa, qb = queries[0], queries[1]
    sa, sb = Spec(ALL, 0.3, 8, 64, 64), Spec(ALL, 0.01, 8, 64, 1024)
    data = big_recs.copy()
    data[first + 2], data[first + cnt - 1] = near(qa), near(qa, limb=9)
    data[first + 70], data[first + cnt - 40] = near(qb, limb=5), near(qb, limb=11)
    with ih.Database(dev, ih.KIND_TEMPLATES, BIG_NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, sa), (qb, sb)], first, cnt)
        ra, rb = wait(pa, sa), wait(pb, sb)
        assert shared_stats(dev) == only_report(1, 18)
        assert len(ra["topk"]) == len(rb["topk"]) == 64 and ra["matches_count"] == rb["matches_count"] == 2
        check_sum(ra, sa, cnt)
        check_sum(rb, sb, cnt)
        assert ra == blocking(dev, db, qa, sa, first, cnt)
        assert rb == blocking(dev, db, qb, sb, first, cnt)
        check_oracle(ra, sa, qa, data, first, cnt)
        check_oracle(rb, sb, qb, data, first, cnt)


# ---------------------------------------------------------------- 5. equal records


@gpu
def test_cut_through_equal_records(hooked_device, recs, queries):
    """The placement of test_gpu_topk_async's test of this name (19 tiles; one closer record, then
    three records of one distance in tiles 1, 6 and 14: waves 0, 1 and 3, both rounds).  k cuts
    through the tie; the threshold sits at the tie's distance (strict: the tie is out) and at the
    next f64 (the tie is in): the list and the match list are in the blocking order."""
    dev = hooked_device(**FORCED)
    first, cnt = span(19)
    qa, qb = queries[0], queries[1]

    def in_tile(t, r):  # record r of the range's tile t (the range starts in tile 0 at record 5)
        return (1 + t) * TILE + r

    eq_a = [in_tile(1, 30), in_tile(6, 3), in_tile(14, 2)]
    eq_b = [in_tile(1, 7), in_tile(6, 17), in_tile(14, 29)]
    top_a, top_b = in_tile(17, 4), in_tile(9, 9)
    data = recs.copy()
    for i in eq_a:
        data[i] = near(qa)
    for i in eq_b:
        data[i] = near(qb, limb=5)
    data[top_a] = near(qa, limb=8, flips=0xFF)
    data[top_b] = near(qb, limb=8, flips=0xFF)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        with ih.TemplateEngine(dev, qa) as e:
            tie_a = e.topk(db, 2, first, cnt)[1].distance
        with ih.TemplateEngine(dev, qb) as e:
            tie_b = e.topk(db, 2, first, cnt)[1].distance
        for j, (k, above) in enumerate([(3, False), (4, True), (2, True)]):
            sa = Spec(ALL, float(np.nextafter(tie_a, 1.0)) if above else tie_a, 3, k, 1024)
            sb = Spec(ALL, tie_b if above else float(np.nextafter(tie_b, 1.0)), 2, k, 512)
            dev.reset_stats()
            pa, pb = submit(dev, db, [(qa, sa), (qb, sb)], first, cnt)
            ra, rb = wait(pa, sa), wait(pb, sb)
            assert shared_stats(dev) == only_report(1, grid_of(19))
            assert [m[1] for m in ra["topk"]] == [i + BASE for i in ([top_a] + eq_a)[:k]]
            assert [m[1] for m in rb["topk"]] == [i + BASE for i in ([top_b] + eq_b)[:k]]
            assert ra["matches_count"] == (4 if above else 1) and rb["matches_count"] == (1 if above else 4)
            assert [m[1] for m in ra["matches"]] == ([i + BASE for i in sorted([top_a] + eq_a)[:3]] if above else [top_a + BASE])
            assert [m[1] for m in rb["matches"]] == ([top_b + BASE] if above else [i + BASE for i in sorted([top_b] + eq_b)[:2]])
            assert ra == blocking(dev, db, qa, sa, first, cnt)
            assert rb == blocking(dev, db, qb, sb, first, cnt)
            if j == 0:
                check_oracle(ra, sa, qa, data, first, cnt)
                check_oracle(rb, sb, qb, data, first, cnt)


# ---------------------------------------------------------------- 6. overflow at the wait


@gpu
@pytest.mark.parametrize("role", ["guest", "host"])
def test_overflow_at_the_wait(hooked_device, recs, queries, role):
    """83 tiles (2644 records), threshold 1.0, cap = 5: the total exceeds the pass's room of 1024
    records, so the wait runs the matches part again -- with the engine long destroyed -- and returns
    the count and the 5 lowest indices; the top-k list and the histogram of the same pending are
    delivered intact.  Once the overflowing pass is the guest, once the host."""
    dev = hooked_device(**FORCED)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    over = Spec(ALL, 1.0, 5, 16, 1024)
    sa, sb = (HOST, over) if role == "guest" else (over, GUEST)
    data = recs.copy()
    data[first + 40], data[first + 900] = near(qa), near(qb, limb=5)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, sa), (qb, sb)], first, cnt)
        ra, rb = wait(pa, sa), wait(pb, sb)
        assert shared_stats(dev) == only_report(1, grid_of(ntiles))
        ro, qo = (rb, qb) if role == "guest" else (ra, qa)
        assert ro["matches_count"] == cnt and [m[1] for m in ro["matches"]] == [first + BASE + i for i in range(5)]
        check_sum(ra, sa, cnt)
        check_sum(rb, sb, cnt)
        assert ra == blocking(dev, db, qa, sa, first, cnt)
        assert rb == blocking(dev, db, qb, sb, first, cnt)
        check_oracle(ro, over, qo, data, first, cnt)
        # the buffers the rerun replaced serve the next submissions
        pa, pb = submit(dev, db, [(qa, sa), (qb, sb)], first, cnt)
        assert wait(pa, sa) == ra and wait(pb, sb) == rb


# ---------------------------------------------------------------- 7. kinds do not mix


@gpu
@pytest.mark.parametrize("case", ["write", "search-first", "search-second", "match-first", "match-second", "topk-first",
                                  "topk-second"])
def test_kinds_do_not_mix(hooked_device, recs, queries, case):
    """A report pass submitted behind a search, a match or a top-k pass of the same range registers
    nowhere, and neither does any of those behind a report pass; nor a report pass behind a report
    pass when the database was written in between (report 2 sees the new record)."""
    dev = hooked_device(**FORCED)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    data[first + 40] = near(qa)
    data[first + 900] = near(qb, limb=5, flips=0xFFFF00FFFFFF00FF)
    site = first + 2000
    kind = case.split("-")[0]

    def other(e, thr):
        return e.search_async(db, first, cnt, index_base=BASE) if kind == "search" else \
            e.matches_async(db, thr, first, cnt, index_base=BASE) if kind == "match" else \
            e.topk_async(db, 4, first, cnt, index_base=BASE)

    def check_other(r, want):
        if kind == "search":
            assert r.index == want + BASE
        elif kind == "match":
            assert ([m.index for m in r[0]], r[1]) == ([want + BASE], 1)
        else:
            assert r[0].index == want + BASE and len(r) == 4

    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        want_a = blocking(dev, db, qa, HOST, first, cnt)  # ahead of the write
        dev.reset_stats()
        with ih.TemplateEngine(dev, qa) as e:
            pa = other(e, 0.3) if case.endswith("-first") else submit_one(e, db, HOST, first, cnt)
        if case == "write":
            data[site] = near(qb, limb=5)
            db.write(site, data[site][None, :])
        with ih.TemplateEngine(dev, qb) as e:
            pb = other(e, 0.2) if case.endswith("-second") else submit_one(e, db, GUEST, first, cnt)
        if case.endswith("-first"):
            check_other(pa.wait(), first + 40)
        else:
            ra = wait(pa, HOST)
            assert ra == want_a and ra["matches_count"] == 1
        if case.endswith("-second"):
            check_other(pb.wait(), first + 900)
        else:
            rb = wait(pb, GUEST)
            assert rb == blocking(dev, db, qb, GUEST, first, cnt)
            assert [m[1] for m in rb["matches"]] == [i + BASE for i in ([first + 900, site] if case == "write" else [first + 900])]
            check_oracle(rb, GUEST, qb, data, first, cnt)
        assert shared_stats(dev) == only_report(0, 0)


# ---------------------------------------------------------------- 8. chains and the ring


def rotating(i):
    parts = rf.SUBSETS[(3 * i + 6) % 7]
    return Spec(parts, [0.3, 0.01, 1.0, 0.2][i % 4], [8, 0, 3, 40][i % 4], [1, 64, 7, 16][i % 4], [1024, 1, 64, 256][i % 4])


@gpu
def test_twelve_submissions(hooked_device, recs, queries):
    """12 report submissions back to back over 17 tiles, past the ring's 8 entries, with rotating
    parts and arguments: every result equals the blocking one.  (How many register depends on when
    ring entries come free, so the stat is printed.)"""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    data = recs.copy()
    for i in range(4):
        data[first + 7 + 100 * i] = near(queries[i], limb=2 + i)
        data[first + 300 + 50 * i] = near(queries[i], limb=9 + i)
    items = [(queries[i % 4], rotating(i)) for i in range(12)]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, items, first, cnt)
        got = [wait(p, s) for p, (_, s) in zip(pend, items)]
        stats = shared_stats(dev)
        print(f"12 submissions: report_shared={stats[0]}")
        assert stats[1:] == ((0, 0), (0, 0), (0, 0)) and 1 <= stats[0][0] <= 11
        for r, (q, s) in zip(got, items):
            check_sum(r, s, cnt)
            assert r == blocking(dev, db, q, s, first, cnt)
        check_oracle(got[-1], items[-1][1], items[-1][0], data, first, cnt)


@gpu
def test_chain_of_three(hooked_device, recs, queries):
    """Three passes before any wait: the middle one is the first one's guest and the last one's
    host.  All of its tile groups were computed by its host, so its own launch exits at once and
    the third pass computes alone: two registrations, one grid carried."""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    data = recs.copy()
    for i in range(3):
        data[first + 7 + 100 * i] = near(queries[i], limb=2 + i)
    items = [(queries[0], HOST), (queries[1], Spec(H, nbins=1024)), (queries[2], GUEST)]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, items, first, cnt)
        got = [wait(p, s) for p, (_, s) in zip(pend, items)]
        assert shared_stats(dev) == only_report(2, grid_of(17))
        for r, (q, s) in zip(got, items):
            check_sum(r, s, cnt)
            assert r == blocking(dev, db, q, s, first, cnt)
        check_oracle(got[1], items[1][1], queries[1], data, first, cnt)


@gpu
def test_python_mirror(hooked_device, recs, queries):
    """TemplateEngine.report_async(...).wait() returns what report() returns, cap None included."""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    data = recs.copy()
    data[first + 7] = near(queries[0])
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        with ih.TemplateEngine(dev, queries[0]) as e:
            pend = [e.report_async(db, threshold=0.3, k=5, nbins=64, first=first, n=cnt, index_base=BASE),
                    e.report_async(db, nbins=16, first=first, n=cnt),
                    e.report_async(db, threshold=1.0, k=2, first=first, n=cnt)]
            assert isinstance(pend[0], ih.PendingReport)
            want = [e.report(db, threshold=0.3, k=5, nbins=64, first=first, n=cnt, index_base=BASE),
                    e.report(db, nbins=16, first=first, n=cnt), e.report(db, threshold=1.0, k=2, first=first, n=cnt)]
            for p, w in zip(pend, want):
                r = p.wait()
                assert (r.matches_count, r.invalid) == (w.matches_count, w.invalid)
                assert [mfields(m) for m in r.matches or []] == [mfields(m) for m in w.matches or []]
                assert [mfields(m) for m in r.topk or []] == [mfields(m) for m in w.topk or []]
                assert (r.bins is None and w.bins is None) or (r.bins == w.bins).all()
            assert want[0].matches_count == 1 and want[2].matches_count == cnt == len(want[2].matches)
            with pytest.raises(ih.IrisError):
                pend[0].wait()


# ---------------------------------------------------------------- 9. unshared forms


@gpu
@pytest.mark.parametrize("form", ["off", "lanes", "ksplit"])
def test_unshared_forms(device, hooked_device, recs, queries, form):
    """IRIS_SEARCH_SHARE=0, a LANES database, and -- without any hook -- a small range in its natural
    K-split form: the blocking report's kernels with the pending's sinks, all parts and one part
    alone through each; nothing registers."""
    dev = device if form == "ksplit" else hooked_device(**dict(FORCED, IRIS_SEARCH_SHARE=0)) if form == "off" else \
        hooked_device(**FORCED)
    first, cnt = span(40 if form == "ksplit" else 17)
    layout = ih.LAYOUT_LANES if form == "lanes" else ih.LAYOUT_TILES
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    data[first + 17], data[first + cnt - 1] = near(qa), near(qa, limb=7)
    data[first + 400] = near(qb, limb=5)
    items = [(qa, HOST), (qb, GUEST), (qa, Spec(H, nbins=128)), (qb, Spec(T, k=64)), (qa, Spec(M, 0.3, 1))]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB, layout) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, items, first, cnt)
        got = [wait(p, s) for p, (_, s) in zip(pend, items)]
        assert shared_stats(dev) == only_report(0, 0)
        for r, (q, s) in zip(got, items):
            check_sum(r, s, cnt)
            assert r == blocking(dev, db, q, s, first, cnt)
            check_oracle(r, s, q, data, first, cnt)
        assert got[0]["matches_count"] == 2 and got[4]["matches_count"] == 2 and len(got[4]["matches"]) == 1


# ---------------------------------------------------------------- 10. edges


@gpu
def test_empty_range(device, recs, queries):
    """n == 0: zero counts and zero bins, nothing launched."""
    names = ("template_report", "template_match", "template_topk", "template_hist", "topk_merge", "hist_reduce")
    with ih.Database(device, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        device.reset_stats()
        device.set_profiling(True)
        try:
            specs = [GUEST, Spec(H, nbins=8), Spec(M | T, 0.5, 0, 3)]
            pend = submit(device, db, [(queries[0], s) for s in specs], 40, 0)
            got = [wait(p, s) for p, s in zip(pend, specs)]
        finally:
            device.set_profiling(False)
        assert all(device.kernel_stats(n)[0] == 0 for n in names)
        assert got[0]["matches_count"] == 0 and got[0]["topk"] == [] and got[0]["invalid"] == 0
        assert not bins_of(got[0], GUEST).any() and not bins_of(got[1], specs[1]).any()
        for r, s in zip(got, specs):
            assert r == blocking(device, db, queries[0], s, 40, 0)


@gpu
def test_zero_masks(hooked_device, recs, queries):
    """17 tiles whose records all have zero masks but three: count < k, invalid == cnt - 3 and three
    matches under a threshold of 1.0, for host and guest of one shared pass."""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    keep = [first + 2, first + 16 * TILE + 1, first + cnt - 1]  # tile group 0, and group 1 twice
    data = recs.copy()
    for i in range(first, first + cnt):
        if i not in keep:
            data[i, 200:] = 0
    sa, sb = Spec(ALL, 1.0, 8, 64, 64), Spec(ALL, 1.0, 2, 7, 1024)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(queries[0], sa), (queries[1], sb)], first, cnt)
        ra, rb = wait(pa, sa), wait(pb, sb)
        assert shared_stats(dev) == only_report(1, grid_of(17))
        for r, s, q in ((ra, sa, queries[0]), (rb, sb, queries[1])):
            assert r["matches_count"] == 3 and r["invalid"] == cnt - 3 and len(r["topk"]) == 3
            assert sorted(m[1] for m in r["topk"]) == [i + BASE for i in keep]
            check_sum(r, s, cnt)
            assert r == blocking(dev, db, q, s, first, cnt)
            check_oracle(r, s, q, data, first, cnt)


@gpu
def test_hist_copies(hooked_device, recs, queries):
    """IRIS_HIST_COPIES=1 (the passes add into one row, a copy brings it back) and =64 give equal bytes."""
    first, cnt = span(16 * 5 + 3)
    got = []
    for copies in (1, 64):
        dev = hooked_device(**FORCED, IRIS_HIST_COPIES=copies)
        with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
            db.append(recs)
            dev.reset_stats()
            pa, pb = submit(dev, db, [(queries[0], HOST), (queries[1], GUEST)], first, cnt)
            got.append((wait(pa, HOST), wait(pb, GUEST)))
            assert shared_stats(dev) == only_report(1, grid_of(16 * 5 + 3))
            assert got[-1][1] == blocking(dev, db, queries[1], GUEST, first, cnt)
    assert got[0] == got[1]
    check_sum(got[0][0], HOST, cnt)
    check_sum(got[0][1], GUEST, cnt)


# ---------------------------------------------------------------- 11. wait-side refusals


@gpu
@pytest.mark.parametrize("case", ["parts", "k", "nbins", "matches_cap", "topk-null", "bins-null", "matches-null"])
def test_wait_refusals(hooked_device, recs, queries, case):
    """The wait's struct differs from the submission's in parts, k, nbins or matches_cap, or a
    selected part's array is missing: IRIS_E_ARG naming the field, nothing written, the handle
    consumed -- a following submission reuses its buffers."""
    dev = hooked_device(**FORCED)
    lib = ih.load_library()
    first, cnt = span(17)
    spec = Spec(ALL, 0.5, 4, 6, 32)
    bad = {"parts": Spec(M | T, 0.5, 4, 6, 32), "k": Spec(ALL, 0.5, 4, 7, 32), "nbins": Spec(ALL, 0.5, 4, 6, 64),
           "matches_cap": Spec(ALL, 0.5, 5, 6, 32)}.get(case, spec)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        with ih.TemplateEngine(dev, queries[0]) as e:
            h = submit_one(e, db, spec, first, cnt)
        r, arrs = struct_of(bad)
        if case == "topk-null":
            r.topk = None
        elif case == "bins-null":
            r.bins = None
        elif case == "matches-null":
            r.matches = None
        before = bytes(r)
        assert lib.iris_pending_report_wait(h, ctypes.byref(r)) == -1
        err = lib.iris_last_error().decode()
        assert {"parts": "parts differs", "k": "k differs", "nbins": "nbins differs", "matches_cap": "matches_cap differs",
                "topk-null": "out is NULL", "bins-null": "bins is NULL", "matches-null": "out is NULL with cap > 0"}[case] in err
        assert bytes(r) == before
        assert bytes(arrs[0]) == bytes([rf.GUARD_BYTE]) * ctypes.sizeof(arrs[0])
        assert bytes(arrs[1]) == bytes([rf.GUARD_BYTE]) * ctypes.sizeof(arrs[1])
        assert arrs[2] is None or (arrs[2] == WORD).all()
        # the handle is gone and its buffers are back: the same submission again, waited for properly
        pa, = submit(dev, db, [(queries[0], spec)], first, cnt)
        assert wait(pa, spec) == blocking(dev, db, queries[0], spec, first, cnt)


@gpu
def test_handles_of_another_kind(device, recs, queries):
    """A report handle given to iris_pending_topk_wait, and a top-k handle given to
    iris_pending_report_wait: refused with both names, and still waitable afterwards.  A template
    batch engine is refused at the submission, and the handle stays NULL."""
    lib = ih.load_library()
    first, cnt = span(40)
    with ih.Database(device, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        with ih.TemplateEngine(device, queries[0]) as e:
            hr = submit_one(e, db, HOST, first, cnt)
            pt = e.topk_async(db, 4, first, cnt, index_base=BASE)
        four, c32 = rf.match_array(4), ctypes.c_uint32(77)
        assert lib.iris_pending_topk_wait(hr, four, ctypes.byref(c32)) == -1
        err = lib.iris_last_error().decode()
        assert "iris_template_report_async" in err and "iris_pending_report_wait" in err and c32.value == 77
        r, arrs = struct_of(HOST)
        before = bytes(r)
        assert lib.iris_pending_report_wait(pt.handle, ctypes.byref(r)) == -1
        err = lib.iris_last_error().decode()
        assert "iris_template_topk_async" in err and "iris_pending_topk_wait" in err and bytes(r) == before
        assert wait(hr, HOST) == blocking(device, db, queries[0], HOST, first, cnt)
        assert len(pt.wait()) == 4
        with ih.TemplateBatchEngine(device, queries) as be:
            r, _ = struct_of(HOST, arrays=False)
            h = ctypes.c_void_p()
            assert lib.iris_template_report_async(be.handle, db.handle, first, cnt, 0, ctypes.byref(r), ctypes.byref(h)) == -1
            assert "single-query" in lib.iris_last_error().decode() and not h.value
