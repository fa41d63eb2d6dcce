"""Pipelined threshold matching (iris_template_matches_async): a match pass that
is still streaming the database also appends the hits of the match pass submitted after it,
workgroup by workgroup.  Whatever is shared, every result equals the blocking matches() of the
same query on the same device field by field (the distance as its f64 bit pattern, index, num,
den, rotation) with the same exact count, and, once per test, the CPU oracle's distances filtered
by the threshold.

The fixtures are tests/test_gpu_search_share.py's: 86 tiles of generated records, four generated
queries, near() records at distance 0.0017 to 0.0028 of their query while no generated record is
closer than 0.4576 to any of them, so thresholds of 0.3 and 0.2 admit exactly the planted records.
The forced tests pin the 4-tiles-per-wave form on small ranges and hold every pass back behind a
2-ms spin, so the next registration lands before the pass starts and every workgroup carries the
guest: `match_shared` (registrations, tile groups carried) is then exact."""
import ctypes

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_search_share import FORCED, NDB, TILE, grid_of, near, queries, recs, span  # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
BASE = 3
INF = float("inf")


def mfields(m):
    return (int(np.float64(m.distance).view(np.uint64)), m.index, m.num, m.den, m.rotation)


def listed(res):
    return [mfields(m) for m in res[0]], res[1]


def blocking(dev, db, q, thr, first, cnt, cap=None, base=BASE):
    with ih.TemplateEngine(dev, q) as e:
        return e.matches(db, thr, first, cnt, index_base=base, cap=cap)


def submit(dev, db, items, first, cnt, cap=None, base=BASE):
    """The (query, threshold) items' asynchronous match passes back to back, every engine
    destroyed at once."""
    pend = []
    for q, thr in items:
        with ih.TemplateEngine(dev, q) as e:
            pend.append(e.matches_async(db, thr, first, cnt, index_base=base, cap=cap))
    return pend


def check_oracle(res, q, thr, data, first, cnt, cap=None, base=BASE):
    d = oc.template_distances(q, data[first:first + cnt])
    idx = np.nonzero(d < thr)[0]
    assert res[1] == len(idx)
    idx = idx if cap is None else idx[:cap]
    assert [m.index for m in res[0]] == [int(i) + first + base for i in idx]
    assert [mfields(m)[0] for m in res[0]] == [int(d[i].view(np.uint64)) for i in idx]


def shared_stats(dev):
    m, s = dev.kernel_stats("match_shared"), dev.kernel_stats("search_shared")
    return (m[0], m[2]), (s[0], s[2])


@gpu
@pytest.mark.parametrize("ntiles", [1, 17, 16 * 5 + 3])
def test_forced_full_sharing(hooked_device, recs, queries, ntiles):
    """Two different queries and thresholds back to back: the first pass carries the second in
    every workgroup.  The guest's moving hit lies in the first tile group, the last one, and the
    last (clamped, partial) tile in turn."""
    dev = hooked_device(**FORCED)
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    last_tile = first // TILE + ntiles - 1
    sites = sorted({first + 1, min(first + cnt - 1, last_tile * TILE - 9) if ntiles > 1 else first + 2,
                    first + cnt - 1})
    hits_a = sorted({first + 3, first + min(cnt - 1, 11), first + cnt // 2})
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        data = recs.copy()
        for k, i in enumerate(hits_a):
            data[i] = near(qa, limb=3 + k)
        data[first + 4] = near(qb, limb=6)
        data[first - 1] = data[first + cnt + 1] = qb  # exact copies just outside the range are never listed
        data[first - 2] = data[first + cnt] = qa
        for k, site in enumerate(sites):
            cur = data.copy()
            cur[site] = near(qb, limb=5)
            db.truncate(0)
            db.append(cur)
            dev.reset_stats()
            pa, pb = submit(dev, db, [(qa, 0.3), (qb, 0.2)], first, cnt)
            ra, rb = pa.wait(), pb.wait()
            stats = shared_stats(dev)
            print(f"ntiles={ntiles} site={site} match_shared={stats[0]} search_shared={stats[1]} grid={grid_of(ntiles)}")
            assert stats == ((1, grid_of(ntiles)), (0, 0))
            assert [m.index for m in ra[0]] == [i + BASE for i in hits_a] and ra[1] == len(hits_a)
            assert [m.index for m in rb[0]] == [i + BASE for i in sorted({first + 4, site})] and rb[1] == 2
            assert listed(ra) == listed(blocking(dev, db, qa, 0.3, first, cnt))
            assert listed(rb) == listed(blocking(dev, db, qb, 0.2, first, cnt))
            if k == 0:
                check_oracle(ra, qa, 0.3, cur, first, cnt)
                check_oracle(rb, qb, 0.2, cur, first, cnt)


@gpu
def test_threshold_edge_in_a_shared_pass(hooked_device, recs, queries):
    """distance < threshold, as f64: a threshold equal to a planted record's distance excludes it,
    the next f64 above includes it -- for the guest and for the hosting query of one pass."""
    dev = hooked_device(**FORCED)
    ntiles = 17
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    ia, ib = first + 100, first + 16 * TILE + 7  # tile groups 0 and 1
    data[ia], data[ib] = near(qa), near(qb, limb=5)
    da = float(oc.template_distances(qa, data[ia:ia + 1])[0])
    db_ = float(oc.template_distances(qb, data[ib:ib + 1])[0])
    assert 0 < da < 0.01 and 0 < db_ < 0.01
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        for k, (ta, tb, in_a, in_b) in enumerate([(da, np.nextafter(db_, 1.0), False, True),
                                                   (np.nextafter(da, 1.0), db_, True, False)]):
            dev.reset_stats()
            pa, pb = submit(dev, db, [(qa, ta), (qb, tb)], first, cnt)
            ra, rb = pa.wait(), pb.wait()
            assert shared_stats(dev) == ((1, grid_of(ntiles)), (0, 0))
            assert ([m.index for m in ra[0]], ra[1]) == (([ia + BASE], 1) if in_a else ([], 0))
            assert ([m.index for m in rb[0]], rb[1]) == (([ib + BASE], 1) if in_b else ([], 0))
            assert listed(ra) == listed(blocking(dev, db, qa, ta, first, cnt))
            assert listed(rb) == listed(blocking(dev, db, qb, tb, first, cnt))
            if k == 0:
                check_oracle(ra, qa, ta, data, first, cnt)
                check_oracle(rb, qb, tb, data, first, cnt)


@gpu
@pytest.mark.parametrize("cap", [10, 0, 3000])
def test_overflow(hooked_device, recs, queries, cap):
    """Threshold +inf over 83 tiles: 2644 matches.  cap = 10: above the 1024-record room, so both
    waits -- host and guest of one shared pass, engines long destroyed -- run the pass again; the
    count is exact and the ten lowest indices come back.  cap = 0: the count only, no rerun.
    cap = 3000: the room holds everything, the inline copy does not."""
    dev = hooked_device(**FORCED)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    assert cnt == 2644
    qa, qb = queries[0], queries[1]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, INF), (qb, INF)], first, cnt, cap=cap)
        ra, rb = pa.wait(), pb.wait()
        assert shared_stats(dev) == ((1, grid_of(ntiles)), (0, 0))
        for r, q in ((ra, qa), (rb, qb)):
            assert r[1] == cnt
            assert [m.index for m in r[0]] == [first + BASE + i for i in range(min(cap, cnt))]
            assert listed(r) == listed(blocking(dev, db, q, INF, first, cnt, cap=cap))
        check_oracle(rb, qb, INF, recs, first, cnt, cap=cap)


@gpu
def test_mixed_groups(hooked_device, recs, queries):
    """IRIS_SEARCH_SHARE_EVEN=1: the hosting pass carries its guest in even tile groups only, so
    one pass has carrying and solo workgroups and the guest's own launch has skipped and computed
    ones.  Hits of both queries lie in even and odd groups: no record twice, none lost."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    tile0 = first // TILE

    def in_group(g, k):  # a record of tile group g (16 tiles from tile0 + 16 g)
        return (tile0 + 16 * g + k) * TILE + 9 + k

    hits_a = [in_group(0, 0), in_group(1, 3), in_group(1, 15), in_group(4, 7), in_group(5, 1)]
    hits_b = [in_group(0, 15), in_group(1, 0), in_group(2, 5), in_group(3, 2), in_group(3, 9), in_group(5, 2)]
    data = recs.copy()
    for k, i in enumerate(hits_a):
        data[i] = near(qa, limb=2 + k)
    for k, i in enumerate(hits_b):
        data[i] = near(qb, limb=9 + k)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, 0.3), (qb, 0.2)], first, cnt)
        ra, rb = pa.wait(), pb.wait()
        even = (grid_of(ntiles) + 1) // 2
        assert shared_stats(dev) == ((1, even), (0, 0))
        assert ([m.index for m in ra[0]], ra[1]) == ([i + BASE for i in hits_a], len(hits_a))
        assert ([m.index for m in rb[0]], rb[1]) == ([i + BASE for i in hits_b], len(hits_b))
        assert listed(ra) == listed(blocking(dev, db, qa, 0.3, first, cnt))
        assert listed(rb) == listed(blocking(dev, db, qb, 0.2, first, cnt))
        check_oracle(rb, qb, 0.2, data, first, cnt)
        # +inf: every record of every group counted once for either query
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, INF), (qb, INF)], first, cnt, cap=0)
        assert (pa.wait(), pb.wait()) == (([], cnt), ([], cnt))
        assert shared_stats(dev) == ((1, even), (0, 0))


@gpu
@pytest.mark.parametrize("count", [3, 4])
def test_submissions_without_a_wait(hooked_device, recs, queries, count):
    """Three and four passes submitted before any wait, every engine destroyed before the first
    wait: each pass hosts at most one guest (the pass after it), and every list equals the
    blocking one."""
    dev = hooked_device(**FORCED)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    data = recs.copy()
    hits = []
    for i in range(count):
        hits.append(sorted([first + 7 + 600 * i, first + 300 + 500 * i]))
        for k, j in enumerate(hits[i]):
            data[j] = near(queries[i], limb=2 + i + 4 * k)
    thr = [0.3, 0.2, 0.25, 0.3]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, [(queries[i], thr[i]) for i in range(count)], first, cnt)
        got = [p.wait() for p in pend]
        stats = shared_stats(dev)
        print(f"count={count} match_shared={stats[0]}")
        # every pass but the first registers with the pass before it; a pass whose own tile groups
        # were all computed by its host exits at once and carries nothing: passes 1 and 3 carry
        assert stats == ((count - 1, count // 2 * grid_of(ntiles)), (0, 0))
        for i, r in enumerate(got):
            assert ([m.index for m in r[0]], r[1]) == ([j + BASE for j in hits[i]], 2)
            assert listed(r) == listed(blocking(dev, db, queries[i], thr[i], first, cnt))
        check_oracle(got[-1], queries[count - 1], thr[count - 1], data, first, cnt)


@gpu
@pytest.mark.parametrize("case", ["write", "other-first", "other-n", "lanes", "off", "search-first", "search-second"])
def test_no_sharing(hooked_device, recs, queries, case):
    """What must not share: a database written between the two submissions (list 2 sees the new
    record), another `first` or `n`, a LANES database, IRIS_SEARCH_SHARE=0, and a search next to
    a match pass of the same range, in either order."""
    env = dict(FORCED, IRIS_SEARCH_SHARE=0) if case == "off" else FORCED
    dev = hooked_device(**env)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    layout = ih.LAYOUT_LANES if case == "lanes" else ih.LAYOUT_TILES
    first2, cnt2 = (first + 1, cnt - 1) if case == "other-first" else (first, cnt - 1) if case == "other-n" else (first, cnt)
    data = recs.copy()
    data[first + 40] = near(qa)
    data[first + 900] = near(qb, limb=5, flips=0xFFFF00FFFFFF00FF)
    site = first + 2000
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB, layout) as db:
        db.append(data)
        dev.reset_stats()
        with ih.TemplateEngine(dev, qa) as e:
            pa = e.search_async(db, first, cnt, index_base=BASE) if case == "search-first" else \
                e.matches_async(db, 0.3, first, cnt, index_base=BASE)
        want_b = [first + 900]
        if case == "write":
            data[site] = near(qb, limb=5)
            db.write(site, data[site][None, :])
            want_b.append(site)
        with ih.TemplateEngine(dev, qb) as e:
            pb = e.search_async(db, first2, cnt2, index_base=BASE) if case == "search-second" else \
                e.matches_async(db, 0.2, first2, cnt2, index_base=BASE)
        ra, rb = pa.wait(), pb.wait()
        assert shared_stats(dev) == ((0, 0), (0, 0))
        if case == "search-first":
            assert ra.index == first + 40 + BASE
        else:
            assert ([m.index for m in ra[0]], ra[1]) == ([first + 40 + BASE], 1)
            assert listed(ra) == listed(blocking(dev, db, qa, 0.3, first, cnt))
        if case == "search-second":
            assert rb.index == first + 900 + BASE
        else:
            assert ([m.index for m in rb[0]], rb[1]) == ([i + BASE for i in want_b], len(want_b))
            assert listed(rb) == listed(blocking(dev, db, qb, 0.2, first2, cnt2))
            check_oracle(rb, qb, 0.2, data, first2, cnt2)


@gpu
def test_unshared_forms_without_hooks(device, recs, queries):
    """No hook: the K-split form (40 tiles), a one-record range (its record is a generated one:
    empty list, count 0), an empty range, a template batch engine (refused), and `out == NULL`
    with cap > 0 at the wait (refused; the handle is freed all the same)."""
    qa, qb = queries[0], queries[1]
    first, cnt = span(40)
    data = recs.copy()
    data[first + 17], data[first + cnt - 1] = near(qa), near(qa, limb=7)
    data[first + 600] = near(qb, limb=5)
    lib = ih.load_library()
    with ih.Database(device, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        device.reset_stats()
        pa, pb = submit(device, db, [(qa, 0.3), (qb, 0.2)], first, cnt)
        p1, p0 = submit(device, db, [(qa, 0.3)], first, 1)[0], submit(device, db, [(qb, INF)], first, 0)[0]
        ra, rb = pa.wait(), pb.wait()
        assert shared_stats(device) == ((0, 0), (0, 0))
        assert ([m.index for m in ra[0]], ra[1]) == ([first + 17 + BASE, first + cnt - 1 + BASE], 2)
        assert ([m.index for m in rb[0]], rb[1]) == ([first + 600 + BASE], 1)
        assert listed(ra) == listed(blocking(device, db, qa, 0.3, first, cnt))
        assert listed(rb) == listed(blocking(device, db, qb, 0.2, first, cnt))
        check_oracle(ra, qa, 0.3, data, first, cnt)
        assert p1.wait() == ([], 0) and p0.wait() == ([], 0)
        with ih.TemplateBatchEngine(device, queries) as be:
            h = ctypes.c_void_p()
            assert lib.iris_template_matches_async(be.handle, db.handle, first, cnt, 0, 0.3, 4, ctypes.byref(h)) == -1
            assert "single-query" in lib.iris_last_error().decode() and not h.value
        with ih.TemplateEngine(device, qa) as e:
            h = ctypes.c_void_p()
            assert lib.iris_template_matches_async(e.handle, db.handle, first, cnt, 0, 0.3, 4, ctypes.byref(h)) == 0
            hs = ctypes.c_void_p()
            assert lib.iris_template_search_async(e.handle, db.handle, first, cnt, 0, ctypes.byref(hs)) == 0
        count, m = ctypes.c_uint64(77), ih.Match()
        # each wait refuses the other submission's handle and leaves it to its own wait
        assert lib.iris_pending_wait(h, ctypes.byref(m)) == -1
        assert "iris_pending_matches_wait" in lib.iris_last_error().decode()
        assert lib.iris_pending_matches_wait(hs, (ih.Match * 4)(), ctypes.byref(count)) == -1
        assert "iris_pending_wait" in lib.iris_last_error().decode() and count.value == 77
        assert lib.iris_pending_wait(hs, ctypes.byref(m)) == 0 and m.index == first + 17
        assert lib.iris_pending_matches_wait(h, None, ctypes.byref(count)) == -1
        assert "out is NULL" in lib.iris_last_error().decode() and count.value == 77


@gpu
def test_forced_sharing_no_candidate(hooked_device, recs, queries):
    """Every record has a zero joint mask with both queries: no record matches, not even under
    +inf, in a shared pass."""
    dev = hooked_device(**FORCED)
    first, cnt = span(17)
    qa, qb = queries[0].copy(), queries[1].copy()
    qa[200:] = 0
    qb[200:] = 0
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(recs)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, INF), (qb, 0.3)], first, cnt)
        assert (pa.wait(), pb.wait()) == (([], 0), ([], 0))
        assert shared_stats(dev) == ((1, grid_of(17)), (0, 0))
        assert blocking(dev, db, qa, INF, first, cnt) == ([], 0)


@gpu
def test_unforced_pipeline_at_natural_size(device):
    """No hook: 2.2M templates (4297 workgroups, just above the fused limit of 4096), 12 pipelined
    steps with 12 different queries, each a perturbed copy of one record.  Whether a pass carries
    the next one depends on timing, so the counters are only printed."""
    n, steps = 2_200_000, 12
    rng = np.random.default_rng(5)
    with ih.Database(device, ih.KIND_TEMPLATES, n) as db:
        db.generate(n, 77)
        sites = [int(x) for x in rng.choice(n, steps, replace=False)]
        qs = [near(db.read(s, 1)[0], limb=1 + k) for k, s in enumerate(sites)]
        device.reset_stats()
        got, pend = [], None
        for q in qs:
            with ih.TemplateEngine(device, q) as e:
                p = e.matches_async(db, 0.3)
            if pend is not None:
                got.append(pend.wait())
            pend = p
        got.append(pend.wait())
        stats = shared_stats(device)
        print(f"unforced: {steps} steps, match_shared={stats[0]} search_shared={stats[1]} (grid 4297)")
        for q, s, r in zip(qs, sites, got):
            assert ([m.index for m in r[0]], r[1]) == ([s], 1)
            assert listed(r) == listed(blocking(device, db, q, 0.3, 0, n, base=0))
