"""Pipelined top-k (iris_template_topk_async): a top-k pass that is still streaming
the database also ranks the candidates of the top-k pass submitted after it, workgroup by
workgroup.  Whatever is shared, every result equals the blocking topk() of the same query on the
same device field by field (the distance as its f64 bit pattern, then index, num, den, rotation)
and, once per test, the CPU oracle's distances sorted by distance, then index.

The fixtures are tests/test_gpu_search_share.py's: 86 tiles of generated records, four generated
queries, near() records at distance 0.0017 to 0.0028 of their query while no generated record is
closer than 0.4576 to any of them.  The forced tests pin the 4-tiles-per-wave form on small ranges
and hold every pass back behind a 2-ms spin, so the next registration lands before the pass starts
and every workgroup carries the guest: `topk_shared` (registrations, tile groups carried) is then
exact.  The file's 21 tests take 2.6 s together on an MI355X."""
import ctypes

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_search_share import FORCED, NDB, TILE, grid_of, near, queries, recs, span  # noqa: F401 (fixtures)

gpu = pytest.mark.gpu
BASE = 3
BIG_TILES = 16 * 17 + 3  # 18 workgroups, 72 lists: two merge levels (kTopkFanIn = 64)
BIG_NDB = (BIG_TILES + 3) * TILE


def mfields(m):
    return (int(np.float64(m.distance).view(np.uint64)), m.index, m.num, m.den, m.rotation)


def listed(res):
    return [mfields(m) for m in res]


def blocking(dev, db, q, k, first, cnt, base=BASE):
    with ih.TemplateEngine(dev, q) as e:
        return e.topk(db, k, first, cnt, index_base=base)


def submit(dev, db, items, first, cnt, base=BASE):
    """The (query, k) items' asynchronous top-k passes back to back, every engine destroyed at once."""
    pend = []
    for q, k in items:
        with ih.TemplateEngine(dev, q) as e:
            pend.append(e.topk_async(db, k, first, cnt, index_base=base))
    return pend


def oracle_list(q, k, data, first, cnt, base=BASE):
    """(distance bits, index) of the k closest records: by distance, then index; +inf never listed."""
    d = oc.template_distances(q, data[first:first + cnt])
    order = np.lexsort((np.arange(cnt), d))
    order = [int(i) for i in order if np.isfinite(d[i])][:k]
    return [(int(d[i].view(np.uint64)), i + first + base) for i in order]


def check_oracle(res, q, k, data, first, cnt, base=BASE):
    assert [mfields(m)[:2] for m in res] == oracle_list(q, k, data, first, cnt, base)


def shared_stats(dev):
    t, m, s = dev.kernel_stats("topk_shared"), dev.kernel_stats("match_shared"), dev.kernel_stats("search_shared")
    return (t[0], t[2]), (m[0], m[2]), (s[0], s[2])


def only_topk(regs, carried):
    return ((regs, carried), (0, 0), (0, 0))


def wait_raw(p, room=ih.TOPK_MAX):
    """The wait through the C ABI on a sentinel-filled array -> (listed entries, the array, count)."""
    out = (ih.Match * room)()
    for m in out:
        m.index, m.num, m.den, m.rotation, m.distance = 0xABCDEF, 77, 78, 79, -5.0
    cnt = ctypes.c_uint32(12345)
    h, p.handle = p.handle, None
    assert ih.load_library().iris_pending_topk_wait(h, out, ctypes.byref(cnt)) == 0
    return [out[i] for i in range(cnt.value)], out, cnt.value


def untouched(out, count):
    return all((m.index, m.num, m.den, m.rotation, m.distance) == (0xABCDEF, 77, 78, 79, -5.0)
               for m in list(out)[count:])


@gpu
@pytest.mark.parametrize("ntiles", [1, 17, 16 * 5 + 3])
def test_forced_full_sharing(hooked_device, recs, queries, ntiles):
    """Two different queries back to back, k = 5 and k = 64: the first pass carries the second in
    every workgroup.  The guest's moving near record lies in the first tile group, the last one, and
    the last (clamped, partial) tile in turn."""
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
        data[first - 1] = data[first + cnt + 1] = qb  # exact copies just outside the range are never listed
        data[first - 2] = data[first + cnt] = qa
        for j, site in enumerate(sites):
            cur = data.copy()
            cur[site] = near(qb, limb=5)
            db.truncate(0)
            db.append(cur)
            dev.reset_stats()
            pa, pb = submit(dev, db, [(qa, 5), (qb, 64)], first, cnt)
            ra, rb = pa.wait(), pb.wait()
            stats = shared_stats(dev)
            print(f"ntiles={ntiles} site={site} topk_shared={stats[0]} grid={grid_of(ntiles)}")
            assert stats == only_topk(1, grid_of(ntiles))
            assert len(ra) == 5 and len(rb) == min(64, cnt)
            assert sorted(m.index for m in ra[:len(hits_a)]) == [i + BASE for i in hits_a]
            assert sorted(m.index for m in rb[:2]) == sorted(i + BASE for i in {first + 4, site})
            assert all(0 < m.distance and first + BASE <= m.index < first + cnt + BASE for m in ra + rb)
            assert listed(ra) == listed(blocking(dev, db, qa, 5, first, cnt))
            assert listed(rb) == listed(blocking(dev, db, qb, 64, first, cnt))
            if j == 0:
                check_oracle(ra, qa, 5, cur, first, cnt)
                check_oracle(rb, qb, 64, cur, first, cnt)


@gpu
@pytest.mark.parametrize("case", ["one-tile", "zero-masks"])
def test_ranges_smaller_than_k(hooked_device, recs, queries, case):
    """k = 64 over a one-tile range of 20 records, and over 17 tiles whose records all have zero
    masks but three: count < k for host and guest of one shared pass, entries past it untouched."""
    dev = hooked_device(**FORCED)
    ntiles = 1 if case == "one-tile" else 17
    first, cnt = span(ntiles)
    qa, qb = queries[0], queries[1]
    data = recs.copy()
    want = cnt
    if case == "zero-masks":
        keep = [first + 2, first + 16 * TILE + 1, first + cnt - 1]  # tile group 0, and group 1 twice
        for i in range(first, first + cnt):
            if i not in keep:
                data[i, 200:] = 0
        want = 3
    else:
        assert cnt == 20
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, 64), (qb, 64)], first, cnt)
        (ra, outa, ca), (rb, outb, cb) = wait_raw(pa), wait_raw(pb)
        assert shared_stats(dev) == only_topk(1, grid_of(ntiles))
        assert ca == cb == want and untouched(outa, ca) and untouched(outb, cb)
        assert listed(ra) == listed(blocking(dev, db, qa, 64, first, cnt))
        assert listed(rb) == listed(blocking(dev, db, qb, 64, first, cnt))
        check_oracle(rb, qb, 64, data, first, cnt)
        if case == "zero-masks":
            assert sorted(m.index for m in rb) == [i + BASE for i in keep]


@gpu
def test_cut_through_equal_records(hooked_device, recs, queries):
    """19 tiles.  For either query one closer record, then three records of one distance in tile 1
    (wave 0, first round), tile 6 (wave 1, second round) and tile 14 (wave 3, second round): k = 3
    cuts between the second and the third, and the two lowest indices are kept, in index order."""
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
        for j, k in enumerate([3, 4, 2]):
            dev.reset_stats()
            pa, pb = submit(dev, db, [(qa, k), (qb, k)], first, cnt)
            ra, rb = pa.wait(), pb.wait()
            assert shared_stats(dev) == only_topk(1, grid_of(19))
            assert [m.index for m in ra] == [i + BASE for i in ([top_a] + eq_a)[:k]]
            assert [m.index for m in rb] == [i + BASE for i in ([top_b] + eq_b)[:k]]
            assert len({mfields(m)[0] for m in ra[1:]}) == 1 and len({mfields(m)[0] for m in rb[1:]}) == 1
            assert listed(ra) == listed(blocking(dev, db, qa, k, first, cnt))
            assert listed(rb) == listed(blocking(dev, db, qb, k, first, cnt))
            if j == 0:
                check_oracle(ra, qa, k, data, first, cnt)
                check_oracle(rb, qb, k, data, first, cnt)


@gpu
def test_mixed_groups(hooked_device, recs, queries):
    """IRIS_SEARCH_SHARE_EVEN=1, 83 tiles, A, B and C back to back: A carries B in even tile groups,
    B -- a guest itself -- computes its odd groups and carries C there, C computes the even ones.
    B's and C's k best are spread over groups of both launches, an equal pair with one record on
    either side included, either one first: no record twice, none lost."""
    dev = hooked_device(**FORCED, IRIS_SEARCH_SHARE_EVEN=1)
    ntiles = 16 * 5 + 3
    first, cnt = span(ntiles)
    qa, qb, qc = queries[0], queries[1], queries[2]
    tile0 = first // TILE

    def in_group(g, t):  # a record of tile group g (16 tiles from tile0 + 16 g)
        return (tile0 + 16 * g + t) * TILE + 9 + t

    data = recs.copy()
    hits = {}
    for qi, q in ((1, qb), (2, qc)):
        pair_lo_even = [in_group(0, 3 + qi), in_group(1, 2 + qi)]   # the lower index in a hosted group
        pair_lo_odd = [in_group(3, 5 + qi), in_group(4, 1 + qi)]    # the lower index in an own group
        single = [in_group(2, 8 + qi), in_group(5, qi)]
        for i in pair_lo_even:
            data[i] = near(q, limb=4)
        for i in pair_lo_odd:
            data[i] = near(q, limb=12, flips=0xFFFF)
        for j, i in enumerate(single):
            data[i] = near(q, limb=20 + j, flips=0xFF << (8 * j))
        hits[qi] = sorted(pair_lo_even + pair_lo_odd + single)
    data[in_group(1, 0)] = near(qa)
    data[in_group(4, 15)] = near(qa, limb=9)
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        for j, (ka, kb, kc) in enumerate([(4, 8, 64), (64, 3, 5)]):
            dev.reset_stats()
            pa, pb, pc = submit(dev, db, [(qa, ka), (qb, kb), (qc, kc)], first, cnt)
            ra, rb, rc = pa.wait(), pb.wait(), pc.wait()
            assert shared_stats(dev) == only_topk(2, 6)
            for r, q, k, qi in ((ra, qa, ka, 0), (rb, qb, kb, 1), (rc, qc, kc, 2)):
                assert len(r) == k and len({m.index for m in r}) == k
                if qi:
                    n_near = min(k, 6)
                    assert {m.index - BASE for m in r[:n_near]} <= set(hits[qi])
                    assert k < 6 or sorted(m.index - BASE for m in r[:6]) == hits[qi]
                assert listed(r) == listed(blocking(dev, db, q, k, first, cnt))
                if j == 0:
                    check_oracle(r, q, k, data, first, cnt)


@pytest.fixture(scope="module")
def big_recs():
    return oc.gen_templates(9393, 0, BIG_NDB)


@gpu
def test_more_than_one_merge_level(hooked_device, big_recs, queries):
    """275 tiles: 18 workgroups and 72 lists per query, above the merge's fan-in of 64, so host and
    guest of one shared pass are folded in two levels.  k = 64, near records in the first and the
    last workgroup, both lists checked against the oracle."""
    dev = hooked_device(**FORCED)
    first, cnt = TILE + 5, BIG_TILES * TILE - 5 - 7
    assert grid_of(BIG_TILES) == 18
    qa, qb = queries[0], queries[1]
    data = big_recs.copy()
    data[first + 2], data[first + cnt - 1] = near(qa), near(qa, limb=9)
    data[first + 70], data[first + cnt - 40] = near(qb, limb=5), near(qb, limb=11)
    with ih.Database(dev, ih.KIND_TEMPLATES, BIG_NDB) as db:
        db.append(data)
        dev.reset_stats()
        pa, pb = submit(dev, db, [(qa, 64), (qb, 64)], first, cnt)
        ra, rb = pa.wait(), pb.wait()
        assert shared_stats(dev) == only_topk(1, 18)
        assert len(ra) == len(rb) == 64
        assert listed(ra) == listed(blocking(dev, db, qa, 64, first, cnt))
        assert listed(rb) == listed(blocking(dev, db, qb, 64, first, cnt))
        check_oracle(ra, qa, 64, data, first, cnt)
        check_oracle(rb, qb, 64, data, first, cnt)


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
        for j, site in enumerate(hits[i]):
            data[site] = near(queries[i], limb=2 + i + 4 * j)
    ks = [7, 64, 1, 16]
    with ih.Database(dev, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        dev.reset_stats()
        pend = submit(dev, db, [(queries[i], ks[i]) for i in range(count)], first, cnt)
        got = [p.wait() for p in pend]
        stats = shared_stats(dev)
        print(f"count={count} topk_shared={stats[0]}")
        # every pass but the first registers with the pass before it; a pass whose own tile groups
        # were all computed by its host exits at once and carries nothing: passes 1 and 3 carry
        assert stats == only_topk(count - 1, count // 2 * grid_of(ntiles))
        for i, r in enumerate(got):
            assert len(r) == ks[i]
            assert {m.index for m in r[:2]} <= {site + BASE for site in hits[i]}
            assert listed(r) == listed(blocking(dev, db, queries[i], ks[i], first, cnt))
        check_oracle(got[-1], queries[count - 1], ks[count - 1], data, first, cnt)


@gpu
@pytest.mark.parametrize("case", ["write", "other-first", "other-n", "lanes", "off", "search-first", "search-second",
                                  "match-first", "match-second"])
def test_no_sharing(hooked_device, recs, queries, case):
    """What must not share: a database written between the two submissions (list 2 sees the new
    record), another `first` or `n`, a LANES database, IRIS_SEARCH_SHARE=0, and a search or a match
    pass next to a top-k pass of the same range, in either order."""
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

    def other(e, kind, thr, f, c):
        return e.search_async(db, f, c, index_base=BASE) if kind == "search" else \
            e.matches_async(db, thr, f, c, index_base=BASE)

    with ih.Database(dev, ih.KIND_TEMPLATES, NDB, layout) as db:
        db.append(data)
        dev.reset_stats()
        with ih.TemplateEngine(dev, qa) as e:
            pa = other(e, case.split("-")[0], 0.3, first, cnt) if case.endswith("-first") and case != "other-first" else \
                e.topk_async(db, 6, first, cnt, index_base=BASE)
        want_b = [first + 900]
        if case == "write":
            data[site] = near(qb, limb=5)
            db.write(site, data[site][None, :])
            want_b.append(site)
        with ih.TemplateEngine(dev, qb) as e:
            pb = other(e, case.split("-")[0], 0.2, first2, cnt2) if case.endswith("-second") else \
                e.topk_async(db, 9, first2, cnt2, index_base=BASE)
        ra, rb = pa.wait(), pb.wait()
        assert shared_stats(dev) == only_topk(0, 0)
        if case == "search-first":
            assert ra.index == first + 40 + BASE
        elif case == "match-first":
            assert ([m.index for m in ra[0]], ra[1]) == ([first + 40 + BASE], 1)
        else:
            assert ra[0].index == first + 40 + BASE and len(ra) == 6
            assert listed(ra) == listed(blocking(dev, db, qa, 6, first, cnt))
        if case == "search-second":
            assert rb.index == first + 900 + BASE
        elif case == "match-second":
            assert ([m.index for m in rb[0]], rb[1]) == ([first + 900 + BASE], 1)
        else:
            assert sorted(m.index for m in rb[:len(want_b)]) == [i + BASE for i in want_b] and len(rb) == 9
            assert listed(rb) == listed(blocking(dev, db, qb, 9, first2, cnt2))
            check_oracle(rb, qb, 9, data, first2, cnt2)


@gpu
def test_unshared_forms_without_hooks(device, recs, queries):
    """No hook: the K-split form (40 tiles), a one-record range, an empty range, a template batch
    engine (refused, the handle stays NULL), `out == NULL` at the wait (refused; the handle is freed
    all the same), and each of the three waits given the other two kinds of handle (refused; the
    handle still serves its own wait)."""
    qa, qb = queries[0], queries[1]
    first, cnt = span(40)
    data = recs.copy()
    data[first + 17], data[first + cnt - 1] = near(qa), near(qa, limb=7)
    data[first + 600] = near(qb, limb=5)
    lib = ih.load_library()
    with ih.Database(device, ih.KIND_TEMPLATES, NDB) as db:
        db.append(data)
        device.reset_stats()
        pa, pb = submit(device, db, [(qa, 10), (qb, 64)], first, cnt)
        p1, p0 = submit(device, db, [(qa, 4)], first, 1)[0], submit(device, db, [(qb, 4)], first, 0)[0]
        ra, rb = pa.wait(), pb.wait()
        assert shared_stats(device) == only_topk(0, 0)
        assert sorted(m.index for m in ra[:2]) == [first + 17 + BASE, first + cnt - 1 + BASE] and len(ra) == 10
        assert rb[0].index == first + 600 + BASE and len(rb) == 64
        assert listed(ra) == listed(blocking(device, db, qa, 10, first, cnt))
        assert listed(rb) == listed(blocking(device, db, qb, 64, first, cnt))
        check_oracle(ra, qa, 10, data, first, cnt)
        r1, out1, c1 = wait_raw(p1, 4)
        assert c1 == 1 and r1[0].index == first + BASE and untouched(out1, 1)
        assert listed(r1) == listed(blocking(device, db, qa, 4, first, 1))
        r0, out0, c0 = wait_raw(p0, 4)
        assert c0 == 0 and untouched(out0, 0)
        with ih.TemplateBatchEngine(device, queries) as be:
            h = ctypes.c_void_p()
            assert lib.iris_template_topk_async(be.handle, db.handle, first, cnt, 0, 4, ctypes.byref(h)) == -1
            assert "single-query" in lib.iris_last_error().decode() and not h.value
        with ih.TemplateEngine(device, qa) as e:
            ht, hm, hs, hn = ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p(), ctypes.c_void_p()
            assert lib.iris_template_topk_async(e.handle, db.handle, first, cnt, 0, 4, ctypes.byref(ht)) == 0
            assert lib.iris_template_matches_async(e.handle, db.handle, first, cnt, 0, 0.3, 4, ctypes.byref(hm)) == 0
            assert lib.iris_template_search_async(e.handle, db.handle, first, cnt, 0, ctypes.byref(hs)) == 0
            assert lib.iris_template_topk_async(e.handle, db.handle, first, cnt, 0, 4, ctypes.byref(hn)) == 0
        c32, c64, m, four = ctypes.c_uint32(77), ctypes.c_uint64(77), ih.Match(), (ih.Match * 4)()
        # each wait refuses the other submissions' handles and leaves them to their own waits
        assert lib.iris_pending_wait(ht, ctypes.byref(m)) == -1
        assert "iris_pending_topk_wait" in lib.iris_last_error().decode()
        assert lib.iris_pending_matches_wait(ht, four, ctypes.byref(c64)) == -1
        assert "iris_pending_topk_wait" in lib.iris_last_error().decode() and c64.value == 77
        assert lib.iris_pending_topk_wait(hs, four, ctypes.byref(c32)) == -1
        assert "iris_pending_wait" in lib.iris_last_error().decode() and c32.value == 77
        assert lib.iris_pending_topk_wait(hm, four, ctypes.byref(c32)) == -1
        assert "iris_pending_matches_wait" in lib.iris_last_error().decode() and c32.value == 77
        assert lib.iris_pending_wait(hs, ctypes.byref(m)) == 0 and m.index == first + 17
        assert lib.iris_pending_matches_wait(hm, four, ctypes.byref(c64)) == 0 and c64.value == 2
        assert lib.iris_pending_topk_wait(ht, four, ctypes.byref(c32)) == 0 and c32.value == 4
        assert sorted(x.index for x in four[:2]) == [first + 17, first + cnt - 1]
        assert lib.iris_pending_topk_wait(hn, None, ctypes.byref(c32)) == -1
        assert "out is NULL" in lib.iris_last_error().decode() and c32.value == 4


@gpu
def test_unforced_pipeline_at_natural_size(device):
    """No hook: 2.2M templates (4297 workgroups, just above the fused limit of 4096), 12 pipelined
    steps with 12 different queries and k = 16, each query a perturbed copy of one record: entry 0
    is that record and every list equals the blocking call's.  Whether a pass carries the next one
    depends on timing, so the counters are only printed."""
    n, steps, k = 2_200_000, 12, 16
    rng = np.random.default_rng(5)
    with ih.Database(device, ih.KIND_TEMPLATES, n) as db:
        db.generate(n, 77)
        sites = [int(x) for x in rng.choice(n, steps, replace=False)]
        qs = [near(db.read(s, 1)[0], limb=1 + j) for j, s in enumerate(sites)]
        device.reset_stats()
        got, pend = [], None
        for q in qs:
            with ih.TemplateEngine(device, q) as e:
                p = e.topk_async(db, k)
            if pend is not None:
                got.append(pend.wait())
            pend = p
        got.append(pend.wait())
        stats = shared_stats(device)
        print(f"unforced: {steps} steps, topk_shared={stats[0]} match_shared={stats[1]} search_shared={stats[2]} (grid 4297)")
        for q, s, r in zip(qs, sites, got):
            assert len(r) == k and r[0].index == s
            assert listed(r) == listed(blocking(device, db, q, k, 0, n, base=0))
