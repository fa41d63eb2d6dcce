"""GPU: rotation ties and equal fractions in different terms through every ranking kernel.  Every
search, match list and top-k list is decided by one rule -- the exact fraction num/den, then the
lowest record index, and inside one record the lowest rotation k -- which the kernels implement
several times (best_rotation's exchange between the two halves of a wave, the batched search's
partial_better_rot at the end of its walk, the ascending scans of the LANES and resolver kernels).
The fixtures of order_fixtures.py make that rule decide: periodic queries (every record's minimum is
reached at several rotations), a crafted query (1/2 as 32/64 and as 64/128 inside one record and
across records), resolver rows at 1/4 in different terms, and resolver rows over the whole u16 range.

Every expectation comes from the CPU oracle's counts (test_gpu_matches.Expected recomputes the best
rotation in integers, test_gpu_topk.order proves its sort in int64); every comparison is exact: all
Match fields, the distance as its f64 bit pattern.  The fixture facts and the host merges need no GPU."""
import numpy as np
import pytest

import iris_hip as ih
import order_fixtures as of
from oracle import oracle_c as oc
from test_gpu_masks_batch import VARIANTS as BATCH_VARIANTS
from test_gpu_masks_batch import DeviceShares
from test_gpu_matches import VARIANTS, DeviceArrays, Expected, bits_of, resolver_expected
from test_gpu_search_share import FORCED, grid_of
from test_gpu_topk import check, order

gpu = pytest.mark.gpu
ROT, N, SEED = of.ROT, of.N, of.SEED
INF = float("inf")
BASE = 2**40 + 7
KS = (1, 5, 64)
HALF = 0.5
ABOVE_HALF = float(np.nextafter(0.5, np.inf))
ABOVE_QUARTER = float(np.nextafter(of.QUARTER, np.inf))
FORMS = ("search", "matches", "topk")


def _variant(v, device, hooked_device):
    if v in ("tiles-tpw1", "tiles-batch1"):
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v in ("tiles-tpw4", "tiles-batch4"):
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    return _variant(request.param, device, hooked_device)


@pytest.fixture(params=BATCH_VARIANTS)
def bctx(request, device, hooked_device):
    return _variant(request.param, device, hooked_device)


def check_best(e, m, first, n, base):
    """A search's Match over records [first, first + n) of e; Match.index = base + record."""
    want = order(e, first, n)[:1]
    if len(want):
        check(e, [m], want, base)
    else:
        assert m.distance == INF and (m.num, m.den) == (0, 0)


def edges(e, first=0, n=None):
    """Thresholds that make the exact comparison decide: the distance at a quarter of the valid
    records of the range and the next f64 after it."""
    idx = order(e, first, n)
    t = float(e.dist[idx[len(idx) // 4]])
    return [t, float(np.nextafter(t, np.inf))]


# ---------------------------------------------------------------- template fixtures (A, B)


class TemplateCases:
    QUERIES = ("p5", "crafted", "p4", "p8", "random")  # a batch's order: a tied and an untied query side by side

    def __init__(self):
        self.recs = {"generated": oc.gen_templates(SEED, 0, N), "crafted": of.crafted_db(),
                     "crafted-no-better": of.crafted_db(better=False)}
        self.queries = {f"p{p}": of.periodic_query(p) for p in of.PERIODS}
        self.queries["crafted"] = of.crafted_query()
        self.queries["random"] = oc.gen_templates(99, 0, 1)[0]
        self.counts, self.exp = {}, {}
        for dn, recs in self.recs.items():
            for qn, q in self.queries.items():
                self.counts[qn, dn] = oc.template_counts(q, recs)
                self.exp[qn, dn] = Expected(*self.counts[qn, dn])
                assert (bits_of(self.exp[qn, dn].dist) == bits_of(oc.template_distances(q, recs))).all()
        # search ranges, picked by the oracle: the winner's lowest tied k is 4 (half 1, its next tie k = 9
        # in half 0) and is in 0..3 (half 0, the next tie in half 1 for p = 4)
        e5 = self.exp["p5", "generated"]
        self.half1_ranges = of.ranges_by_lowest_k(e5, lambda k: k == 4, 2)
        self.half0_ranges = of.ranges_by_lowest_k(e5, lambda k: k < 4, 2)
        # crafted: a range from every tied record on (that record wins: the index decides), ranges that
        # end before the strictly better record, and the whole database (the better record wins)
        self.crafted_ranges = [(t, min(N - t, 1089 - t)) for t in of.TIED] + [(41, 257), (71, 5), (0, N), (1089, 11)]

    def search_ranges(self, qn, dn):
        if dn.startswith("crafted"):
            return self.crafted_ranges if qn == "crafted" else self.crafted_ranges[::6] + [(0, N)]
        return self.half1_ranges + self.half0_ranges + [(0, N), (5, 257)]

    def thresholds(self, qn, dn, first=0, n=None):
        if (qn, dn) == ("crafted", "crafted"):
            return [HALF, ABOVE_HALF]
        return edges(self.exp[qn, dn], first, n)

    def db(self, dev, layout, dn):
        db = ih.Database(dev, ih.KIND_TEMPLATES, N, layout)
        if dn == "generated":
            db.generate(N, SEED)
        else:
            db.append(self.recs[dn])
        return db


@pytest.fixture(scope="module")
def tc():
    return TemplateCases()


def test_periodic_fixture_facts(tc):
    """A: rotations k and k + p agree in both counts for every record; every lowest tied k of p = 5
    occurs often; the search ranges' winners are what they were picked for."""
    for p in of.PERIODS:
        for dn in ("generated", "crafted"):
            num, den = tc.counts[f"p{p}", dn]
            assert (num[:, :ROT - p] == num[:, p:]).all() and (den[:, :ROT - p] == den[:, p:]).all()
            assert (of.lowest(tc.exp[f"p{p}", dn]) < p).all()
    e5, e4, e8 = (tc.exp[f"p{p}", "generated"] for p in of.PERIODS)
    classes = np.bincount(of.lowest(e5)[:400], minlength=5)
    assert classes.min() >= 20, classes
    assert (e5.den != 0).all() and (e4.den != 0).all() and (e8.den != 0).all()
    for first, n in tc.half1_ranges:
        k = of.lowest(e5)[of.winner(e5, first, n)]
        assert k == 4 and of.half(k) == 1 and of.half(k + 5) == 0
        assert of.winner(e5, first, n) == order(e5, first, n)[0]
    for first, n in tc.half0_ranges:
        assert of.lowest(e5)[of.winner(e5, first, n)] < 4
    k4 = of.lowest(e4)
    assert all(of.half(k) == 0 and of.half(k + 4) == 1 for k in k4[:50])
    assert len(set(k4[:400])) == 4 and len(set(of.lowest(e8)[:400])) == 8
    assert all(of.half(k) == of.half(k + 8) for k in range(ROT - 8))


def test_crafted_fixture_facts(tc):
    """B: each planted record has exactly the rotations it opens, at 32/64 and 64/128; the expected
    result is the lowest k with that rotation's own terms; across records the index decides."""
    num, den = (np.asarray(a, np.int64) for a in tc.counts["crafted", "crafted"])
    e = tc.exp["crafted", "crafted"]
    for i, (rh, rf) in {**of.INSIDE, **of.ACROSS}.items():
        valid = {int(k): (int(num[i, k]), int(den[i, k])) for k in np.flatnonzero(den[i])}
        want = {}
        if rh is not None:
            want[rh + 15] = (32, 64)
        if rf is not None:
            want[rf + 15] = (64, 128)
        assert valid == want, (i, valid)
        k = min(want)
        assert (e.num[i], e.den[i], e.rot[i] + 15) == (*want[k], k) and e.dist[i] == 0.5, i
    low = {i: (min(rh, rf) + 15, max(rh, rf) + 15, rh < rf) for i, (rh, rf) in of.INSIDE.items()}
    assert low[40] == (7, 17, True) and low[41] == (7, 17, False)  # half 1 first: smaller terms first, larger first
    assert (of.half(7), of.half(17)) == (1, 0)
    assert low[42][:2] == (2, 6) and low[43][:2] == (2, 6) and (of.half(2), of.half(6)) == (0, 1)
    assert [of.half(k) for k in (*low[44][:2], *low[46][:2])] == [0, 0, 1, 1]
    assert (e.num[40], e.den[40]) == (32, 64) and (e.num[41], e.den[41]) == (64, 128)
    # across records: X (32/64) before Y (64/128) and Y before X, in one tile, in two tiles of one
    # four-tile wave, in two waves of a workgroup (512 records) and in two workgroups
    pairs = [(70, 75), (76, 79), (130, 170), (200, 250), (300, 450), (270, 400), (520, 1040), (600, 1080)]
    assert sorted(i for p in pairs for i in p) == sorted(of.ACROSS)
    assert {(int(e.den[a]), int(e.den[b])) for a, b in pairs} == {(64, 128), (128, 64)}
    assert all(a // 32 == b // 32 for a, b in pairs[:2])
    assert all(a // 32 != b // 32 and a // 128 == b // 128 for a, b in pairs[2:4])
    assert all(a // 128 != b // 128 and a // 512 == b // 512 for a, b in pairs[4:6])
    assert all(a // 512 != b // 512 for a, b in pairs[6:])
    # the thresholds: nothing tied is below 1/2, everything tied is below the next f64; the rest is
    # invalid or strictly worse
    assert list(e.hits(HALF)) == [of.BETTER] and (e.num[of.BETTER], e.den[of.BETTER]) == (31, 64)
    assert list(e.hits(ABOVE_HALF)) == of.TIED + [of.BETTER]
    rest = np.setdiff1d(np.arange(N), of.TIED + [of.BETTER])
    assert ((e.den[rest] == 0) | (2 * e.num[rest] > e.den[rest])).all()
    assert (e.den[rest] == 0).sum() > 300 and (e.den[rest] != 0).sum() > 600
    assert list(order(e)[:len(of.TIED) + 1]) == [of.BETTER] + of.TIED
    for first, n in tc.crafted_ranges[:len(of.TIED)]:
        assert order(e, first, n)[0] == first  # the tied record a range starts at wins it
    assert order(e, 0, N)[0] == of.BETTER and order(e, 1089, 11)[0] == of.BETTER
    nb = tc.exp["crafted", "crafted-no-better"]
    assert order(nb)[0] == 40 and (nb.num[40], nb.den[40], nb.rot[40]) == (32, 64, -8)
    # the periodic queries tie on the crafted records too, the crafted query nowhere on the generated ones
    g = tc.counts["crafted", "generated"]
    f = np.where(g[1] != 0, g[0] / np.maximum(g[1], 1), 9.0)
    assert ((f == f.min(axis=1, keepdims=True)).sum(axis=1) == 1).mean() > 0.9


# ---------------------------------------------------------------- 1. one query


@gpu
def test_template_counts_and_distances(ctx, tc):
    device, layout = ctx
    for dn in ("generated", "crafted"):
        with tc.db(device, layout, dn) as db:
            for qn in tc.QUERIES:
                with ih.TemplateEngine(device, tc.queries[qn]) as eng:
                    num, den = eng.counts(db)
                    assert (num == tc.counts[qn, dn][0]).all() and (den == tc.counts[qn, dn][1]).all(), (qn, dn)
                    assert (bits_of(eng.distances(db)) == bits_of(tc.exp[qn, dn].dist)).all(), (qn, dn)
                    d = eng.distances(db, first=37, n=300)
                    assert (bits_of(d) == bits_of(tc.exp[qn, dn].dist[37:337])).all(), (qn, dn)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_template_engine(ctx, tc, form):
    device, layout = ctx
    for dn in ("generated", "crafted"):
        with tc.db(device, layout, dn) as db:
            for qn in tc.QUERIES:
                e = tc.exp[qn, dn]
                with ih.TemplateEngine(device, tc.queries[qn]) as eng:
                    if form == "search":
                        for first, n in tc.search_ranges(qn, dn):
                            check_best(e, eng.search(db, first=first, n=n, index_base=BASE), first, n, BASE)
                        continue
                    for first, n in [(0, N), (41, 1000)]:
                        if form == "matches":
                            for t in tc.thresholds(qn, dn, first, n):
                                got, count = eng.matches(db, t, first=first, n=n, index_base=BASE)
                                e.check(got, count, e.hits(t, first, n), BASE)
                        else:
                            want = order(e, first, n)
                            for k in KS:
                                check(e, eng.topk(db, k, first=first, n=n, index_base=BASE), want[:k], BASE)


# ---------------------------------------------------------------- 2. batches


@gpu
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("nq,kernel", [(2, None), (3, None), (5, "4"), (5, "2")],
                         ids=["pair", "pair-and-one", "batch_lds_q2", "batch_lds_q4"])
def test_template_batch_engine(device, hooked_device, tc, nq, kernel, form):
    """Two queries (template_multi_kernel<2>), three (the pair, then the odd one) and five (the GEMM
    kernel in both its shapes): the batch mixes periodic, crafted and random queries, so one wave ranks
    a tied and an untied query together.  On the half-1 ranges the batched search's two halves hold
    the same record at the same fraction: the rotation alone decides between them."""
    if kernel == "2":
        device = hooked_device(IRIS_BATCH_KERNEL=kernel)
    names = tc.QUERIES[:nq]
    with ih.TemplateBatchEngine(device, np.stack([tc.queries[qn] for qn in names])) as be:
        for dn in ("generated", "crafted"):
            with tc.db(device, ih.LAYOUT_TILES, dn) as db:
                exps = [tc.exp[qn, dn] for qn in names]
                if form == "search":
                    for first, n in tc.search_ranges("crafted", dn):
                        got = be.search(db, first=first, n=n, index_base=BASE)
                        assert len(got) == nq
                        for e, m in zip(exps, got):
                            check_best(e, m, first, n, BASE)
                    continue
                for first, n in [(0, N), (41, 1000)]:
                    if form == "matches":
                        for t in (HALF, ABOVE_HALF) + tuple(edges(exps[0], first, n)):
                            lists, counts = be.matches(db, t, first=first, n=n, index_base=BASE)
                            for e, got, count in zip(exps, lists, counts):
                                e.check(got, count, e.hits(t, first, n), BASE)
                    else:
                        for k in KS:
                            for e, got in zip(exps, be.topk(db, k, first=first, n=n, index_base=BASE)):
                                check(e, got, order(e, first, n)[:k], BASE)


def _ntiles(first, n):
    return (first + n + 31) // 32 - first // 32


@gpu
@pytest.mark.parametrize("form", ["search", "matches"])
def test_shared_passes_host_and_guest(hooked_device, tc, form):
    """search_async and matches_async back to back under the forced-sharing hooks: the first pass
    carries the second in every workgroup (the counter says so), and host and guest both rank their
    ties as the oracle does."""
    dev = hooked_device(**FORCED)
    pairs = [("p5", "crafted"), ("crafted", "p5"), ("p4", "p8"), ("crafted", "p4")]
    for dn in ("generated", "crafted"):
        ranges = tc.search_ranges("crafted", dn)[:8] + [(0, N)]
        with tc.db(dev, ih.LAYOUT_TILES, dn) as db:
            if form == "matches":
                # two passes over the largest range first: a pending's record buffer that has to grow
                # between two submissions is freed, which waits for the pass that should host
                with ih.TemplateEngine(dev, tc.queries["random"]) as eng:
                    for p in [eng.matches_async(db, 0.0), eng.matches_async(db, 0.0)]:
                        assert p.wait() == ([], 0)
            for j, (first, n) in enumerate(ranges):
                host, guest = pairs[j % len(pairs)]
                pend = []
                thr = {qn: tc.thresholds(qn, dn, first, n)[1] for qn in (host, guest)}  # ahead of the submissions
                dev.reset_stats()
                for qn in (host, guest):
                    with ih.TemplateEngine(dev, tc.queries[qn]) as eng:
                        if form == "search":
                            pend.append(eng.search_async(db, first, n, index_base=BASE))
                        else:
                            pend.append(eng.matches_async(db, thr[qn], first, n, index_base=BASE))
                got = [p.wait() for p in pend]
                s, m = dev.kernel_stats("search_shared"), dev.kernel_stats("match_shared")
                shared = (1, grid_of(_ntiles(first, n)))
                assert ((s[0], s[2]), (m[0], m[2])) == ((shared, (0, 0)) if form == "search" else ((0, 0), shared))
                for qn, res in zip((host, guest), got):
                    e = tc.exp[qn, dn]
                    if form == "search":
                        check_best(e, res, first, n, BASE)
                    else:
                        e.check(res[0], res[1], e.hits(thr[qn], first, n), BASE)


@gpu
def test_group_search_with_ties_in_every_shard(tc):
    """GroupDatabase.search and batch_search over three shards of one device: the tied records lie in
    all three, so the merge of the shards' winners decides by the global index."""
    names = tc.QUERIES
    with ih.Group([0]) as g:
        for dn in ("crafted-no-better", "crafted", "generated"):
            with ih.GroupDatabase(g, ih.KIND_TEMPLATES, N, shards_per_device=3) as gdb:
                if dn == "generated":
                    gdb.generate(SEED)
                else:
                    gdb.write(0, tc.recs[dn])
                bounds = [gdb.shard(i) for i in range(3)]
                shard_of = lambda i: [s for s, (f, c) in enumerate(bounds) if f <= i < f + c][0]
                assert {shard_of(i) for i in of.TIED} == {0, 1, 2}
                for qn in names:
                    check_best(tc.exp[qn, dn], gdb.search(tc.queries[qn]), 0, N, 0)
                for nq in (2, 3, 5):
                    got = gdb.batch_search(np.stack([tc.queries[qn] for qn in names[:nq]]))
                    for qn, m in zip(names, got):
                        check_best(tc.exp[qn, dn], m, 0, N, 0)


# ---------------------------------------------------------------- resolver fixtures (C, D)


class TieRows:
    """C: n masks rows of one query mask with rows at 1/4 in different terms."""

    def __init__(self, qmask, masks, rng, spots, parts):
        self.den = oc.masks_batch(qmask, masks)
        self.uneq, self.planted, self.better = of.resolver_ties(self.den, rng, spots)
        self.shares = of.shares_of(of.encoded(self.den, self.uneq), parts, rng)
        self.exp = resolver_expected(self.shares, self.den)


class ResolverCases:
    n = 600

    def __init__(self):
        rng = np.random.default_rng(31)
        self.masks = oc.gen_masks(SEED, 0, self.n)
        self.qmask = oc.gen_templates(99, 0, 1)[0][200:]
        self.ties = TieRows(self.qmask, self.masks, rng, (3, 100, 290, 520), 3)
        # six slabs of a masks batch (a group of four and a pair), tie rows of its own in each
        self.qmasks = rng.integers(0, 2**64, (6, ih.LIMBS), dtype=np.uint64)
        self.slabs = [TieRows(q, self.masks, rng, (5 + 9 * j, 150 + 11 * j, 400 + 13 * j), 2 + j % 2)
                      for j, q in enumerate(self.qmasks)]
        den, uneq, self.subsets = of.ones_case()
        self.ones_den, self.ones_uneq = den, uneq
        self.ones_shares = of.shares_of(of.encoded(den, uneq), 2, rng)
        self.ones = resolver_expected(self.ones_shares, den)
        self.wide_den, self.wide_uneq, self.wide_odd = of.wide_rows()
        self.wide_shares = of.shares_of(of.encoded(self.wide_den, self.wide_uneq, self.wide_odd), 3, rng)
        self.wide = resolver_expected(self.wide_shares, self.wide_den)

    def arrays(self, name):
        """(shares [parts, n, 31], den [n, 31], Expected, thresholds) of a device-array case."""
        if name == "ties":
            return self.ties.shares, self.ties.den, self.ties.exp, [of.QUARTER, ABOVE_QUARTER, INF]
        if name == "ones":
            return self.ones_shares, self.ones_den, self.ones, [of.QUARTER, ABOVE_QUARTER, 0.4]
        top = [float(self.wide.dist[i]) for i in order(self.wide)[:12]]
        return self.wide_shares, self.wide_den, self.wide, sorted({HALF, ABOVE_HALF, 1.0, 2.0, INF, *top,
                                                                   *(float(np.nextafter(t, np.inf)) for t in top)})


@pytest.fixture(scope="module")
def rc():
    return ResolverCases()


def _check_tie_rows(t):
    e, d = t.exp, t.den.astype(np.int64)
    kinds = {}
    for row, (kind, a, b) in t.planted.items():
        assert a < b and d[row, a] % 4 == 0 and d[row, b] % 4 == 0 and d[row, a] != d[row, b]
        assert (e.num[row], e.den[row], e.rot[row] + 15) == (d[row, a] // 4, d[row, a], a) and e.dist[row] == 0.25
        assert 4 * t.uneq[row, b] == d[row, b]  # the later rotation: the same fraction in other terms
        others = np.setdiff1d(np.arange(ROT), [a, b])
        assert (4 * t.uneq[row, others] > d[row, others]).all()  # strictly worse than 1/4
        want = {"h1-first": (1, 0), "h0-first": (0, 1)}.get(kind)
        assert (of.half(a), of.half(b)) == want if want else of.half(a) == of.half(b)
        kinds.setdefault(kind, []).append(row)
    assert all(len(kinds[k]) >= 3 for k in ("h1-first", "h0-first", "same"))
    rows = sorted(t.planted)
    assert list(e.hits(of.QUARTER)) == [t.better] and t.better > rows[-1]
    assert list(e.hits(ABOVE_QUARTER)) == rows + [t.better]
    assert list(order(e)[:len(rows) + 1]) == [t.better] + rows
    # cross-row ties in both index orders: the smaller terms at the lower index and at the higher
    steps = np.sign(np.diff(e.den[rows]))
    assert (steps > 0).any() and (steps < 0).any()


def test_resolver_fixture_facts(rc):
    _check_tie_rows(rc.ties)
    for slab in rc.slabs:
        _check_tie_rows(slab)
    assert len({tuple(sorted(s.planted)) for s in rc.slabs}) == 6  # tie rows of its own in each slab
    e = rc.ones
    for row, ks in rc.subsets.items():
        assert (e.num[row], e.den[row], e.rot[row] + 15) == (3200, 12800, min(ks))
    assert (of.half(5), of.half(9)) == (1, 0) and (of.half(2), of.half(7)) == (0, 1)
    assert list(e.hits(ABOVE_QUARTER)) == sorted(rc.subsets) and len(e.hits(of.QUARTER)) == 0
    assert list(order(e)[:len(rc.subsets)]) == sorted(rc.subsets)


def test_wide_fixture_facts(rc):
    """D: the shares decode to the drawn uneq, over every forced denominator, with uneq above den, odd
    den - total, and at the top of the order neighbours one cross-product unit apart and equal
    fractions in different terms."""
    e, den, uneq = rc.wide, rc.wide_den.astype(np.int64), rc.wide_uneq
    total = rc.wide_shares.astype(np.int64).sum(axis=0) & 0xFFFF
    assert ((((den - total) & 0xFFFF) >> 1) == uneq).all() and (((den - total) & 1) == rc.wide_odd).all()
    assert rc.wide_odd.min() == 0 and rc.wide_odd.max() == 1
    assert all((den == v).any() for v in of.FORCED_DEN) and uneq.max() == 32767 and den.max() == 65535
    assert (uneq > den).any() and (e.num > e.den).any() and e.den[5] == 0
    assert int(e.num.max()) * int(e.den.max()) < 2**31  # the kernels' u32 cross products are exact
    for row, k, u, d in of.PLANTED_WIDE:
        assert (uneq[row, k], den[row, k]) == (u, d)
    top = order(e)[:64]
    planted_rows = {row for row, *_ in of.PLANTED_WIDE}
    assert planted_rows <= set(top[:32].tolist())
    a, b = top[:-1], top[1:]
    gap = e.num[b] * e.den[a] - e.num[a] * e.den[b]
    assert (gap >= 0).all() and (gap == 1).sum() >= 2
    assert ((gap == 0) & (e.den[a] != e.den[b])).sum() >= 2 and ((gap == 0) & (e.den[a] == e.den[b])).any()
    assert (e.den[top] > 65000).any() and (e.den[top] < 3).any()


# ---------------------------------------------------------------- 3. resolver: device arrays, host form


@gpu
@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "offset2"])
@pytest.mark.parametrize("case", ["ties", "ones", "wide"])
def test_resolver_device_arrays(device, rc, case, offset):
    shares, den, e, thresholds = rc.arrays(case)
    total = den.shape[0]
    with DeviceArrays(device, list(shares) + [den], offset) as ptrs:
        sp, dp = ptrs[:-1], ptrs[-1]
        for n in (total, total - 11, 257, 41, 1):
            dist = device.alloc(max(8 * n, 16))
            try:
                m = ih.resolver_search_device(device, sp, dp, n, index_base=BASE, dist_out_device=dist)
                got = np.empty(n, np.float64)
                device.d2h(got, dist)
            finally:
                device.free(dist)
            check_best(e, m, 0, n, BASE)
            assert (bits_of(got) == bits_of(e.dist[:n])).all()
            want = order(e, 0, n)
            for k in KS:
                check(e, ih.resolver_topk(device, sp, dp, n, k, index_base=BASE), want[:k], BASE)
            for t in thresholds:
                lst, count = ih.resolver_matches(device, sp, dp, n, t, index_base=BASE)
                e.check(lst, count, e.hits(t, 0, n), BASE)


@gpu
@pytest.mark.parametrize("case", ["ties", "ones", "wide"])
def test_resolver_host_form(device, rc, case):
    shares, den, e, _ = rc.arrays(case)
    for n in (den.shape[0], 257, 41):
        m = ih.resolver_search([s[:n] for s in shares], den[:n], index_base=BASE, device=device)
        check_best(e, m, 0, n, BASE)


# ---------------------------------------------------------------- 4. resolver: fused with the masks pass


def _fused(device, eng, db, shares, e, first, n, form):
    """MasksEngine.resolve, matches or topk over masks rows [first, first + n): Match.index = BASE + row of the range."""
    with DeviceArrays(device, shares[:, first:first + n]) as ptrs:
        if form == "search":
            check_best(e, eng.resolve(db, ptrs, first=first, n=n, index_base=BASE), first, n, BASE - first)
        elif form == "matches":
            for t in (of.QUARTER, ABOVE_QUARTER):
                got, count = eng.matches(db, ptrs, t, first=first, n=n, index_base=BASE)
                e.check(got, count, e.hits(t, first, n), BASE - first)
        else:
            want = order(e, first, n)
            for k in KS:
                check(e, eng.topk(db, ptrs, k, first=first, n=n, index_base=BASE), want[:k], BASE - first)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_masks_engine_ties(ctx, rc, form):
    """The ranges that start at a tie row and end before the strictly better row are won by that tie row
    (rows[0] and rows[3]: the lowest k in half 1; rows[4]: in half 0; the last: inside one half)."""
    device, layout = ctx
    t = rc.ties
    rows = sorted(t.planted)
    assert [t.planted[r][0] for r in (rows[0], rows[3], rows[4], rows[-1])] == ["h1-first", "h1-first", "h0-first", "same"]
    with ih.Database(device, ih.KIND_MASKS, rc.n, layout) as db, ih.MasksEngine(device, rc.qmask) as eng:
        db.generate(rc.n, SEED)
        for first, n in [(0, rc.n), (rows[0], 300), (rows[3], 257), (rows[4], 257), (rows[1], rc.n - rows[1] - 30),
                         (rows[-1], 1)]:
            _fused(device, eng, db, t.shares, t.exp, first, n, form)
    ones = np.full(ih.LIMBS, ~np.uint64(0))
    n = rc.ones_den.shape[0]
    with ih.Database(device, ih.KIND_MASKS, n, layout) as db, ih.MasksEngine(device, ones) as eng:
        db.append(np.tile(ones, (n, 1)))
        for first, m in [(0, n), (4, 200), (41, 216)]:
            _fused(device, eng, db, rc.ones_shares, rc.ones, first, m, form)


@gpu
@pytest.mark.parametrize("form", FORMS)
def test_masks_batch_ties(bctx, rc, form):
    """Six queries (a group of four and a left-over pair), each slab with tie rows of its own; the range
    (0, 390) ends before every slab's strictly better row, so each slab's first tie row (the lowest k in
    half 1) wins it."""
    device, layout = bctx
    nq = len(rc.slabs)
    assert all(s.better > 390 and s.planted[min(s.planted)][0] == "h1-first" for s in rc.slabs)
    with ih.Database(device, ih.KIND_MASKS, rc.n, layout) as db, ih.MasksBatchEngine(device, rc.qmasks) as eng:
        db.generate(rc.n, SEED)
        for first, n in [(0, rc.n), (0, 390), (7, 500), (160, 257)]:
            # every part holds all six slabs: a slab shared two ways gets a zero third share
            stacked = np.zeros((3, nq, n, ROT), np.uint16)
            for q, s in enumerate(rc.slabs):
                stacked[:len(s.shares), q] = s.shares[:, first:first + n]
            with DeviceShares(device, list(stacked)) as ptrs:
                if form == "search":
                    got = eng.resolve(db, ptrs, first=first, n=n, index_base=BASE)
                    assert len(got) == nq
                    for s, m in zip(rc.slabs, got):
                        check_best(s.exp, m, first, n, BASE - first)
                elif form == "matches":
                    for t in (of.QUARTER, ABOVE_QUARTER):
                        lists, counts = eng.matches(db, ptrs, t, first=first, n=n, index_base=BASE)
                        for s, lst, count in zip(rc.slabs, lists, counts):
                            s.exp.check(lst, count, s.exp.hits(t, first, n), BASE - first)
                else:
                    for k in KS:
                        for s, lst in zip(rc.slabs, eng.topk(db, ptrs, k, first=first, n=n, index_base=BASE)):
                            check(s.exp, lst, order(s.exp, first, n)[:k], BASE - first)


# ---------------------------------------------------------------- 5. the host merges (no GPU)


def _matches_of(e, idx, base):
    out = []
    for i in idx:
        m = ih.Match()
        m.distance, m.index, m.num, m.den, m.rotation = float(e.dist[i]), base + int(i), int(e.num[i]), int(e.den[i]), int(e.rot[i])
        out.append(m)
    return out


@pytest.mark.parametrize("case", ["wide", "ties"])
@pytest.mark.parametrize("chunks", [[(0, 100), (100, 1), (101, 199)], [(0, 31), (31, 11), (42, 258)],
                                    [(c, 20) for c in range(0, 300, 20)]], ids=["three", "uneven", "fifteen"])
def test_host_merges_of_chunk_lists(rc, case, chunks):
    """merge_topk of the chunks' top-k lists is the top-k of the whole and merge_matches of the chunks'
    winners is its winner, on the wide rows (neighbours one cross-product unit apart, equal fractions in
    different terms across chunk borders) and on the tie rows."""
    e = rc.arrays(case)[2]
    total = sum(n for _, n in chunks)
    for k in KS:
        lists = [m for first, n in chunks for m in _matches_of(e, order(e, first, n)[:k], BASE)]
        check(e, ih.merge_topk(lists, k), order(e, 0, total)[:k], BASE)
        check(e, ih.merge_topk(lists[::-1], k), order(e, 0, total)[:k], BASE)
    best = [m for first, n in chunks for m in _matches_of(e, order(e, first, n)[:1], BASE)]
    for winners in (best, best[::-1]):
        check_best(e, ih.merge_matches(winners), 0, total, BASE)
