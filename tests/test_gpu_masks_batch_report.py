"""GPU: the masks batch report (iris_resolver_batch_report_masks): for every query of a masks batch
engine any of its match list, its k closest records and its score histogram from one pass over the
masks database and the participants' share slabs.

Expectations come from the CPU oracle alone (test_gpu_matches.resolver_expected per query, through
resolver_report_fixtures.check) and, byte for byte, from the three sibling batch calls.  The C entry
point is called raw (masks_batch_report_fixtures): guard bytes fill the fields and arrays of
unselected parts and stand behind every output array and every count.

Variants (test_gpu_masks_batch_matches.VARIANTS): a TILES database under the library's own dispatch
(on the 257-record fixture one fused single-query report pass per query), TILES with
IRIS_TILES_PER_WAVE=1 and =4 (the hook pins masks_batch_kernel<G, T, BATCH_REPORT> at one tile per
wave and at its large form: groups of four queries, a left-over three in the four-slot kernel, a
left-over two in the two-slot kernel, a left-over one in the single-query kernel) and a LANES
database (the masks kernel into the workspace, then the resolver kernel's report mode, per query).
257 records are 9 tiles: one tile per wave and 4 (or 2) per wave both end in a ragged group, and
waves without a tile group must still store empty lists and reach both histogram barriers."""
import ctypes
import subprocess

import numpy as np
import pytest

import iris_hip as ih
import masks_batch_report_fixtures as mf
from masks_batch_report_fixtures import ALL, HIST, MATCHES, MULTI, TOPK
from oracle import oracle_c as oc
from test_gpu_masks_batch_matches import PERSIST_N, VARIANTS, SmallCase, background, planted_shares
from test_gpu_matches import DeviceArrays, resolver_expected
from test_gpu_topk import order
from test_masks_batch_report_abi import build_cpp_program

pytestmark = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
BASE = 2**40 + 7
RANGES = [(0, 257), (5, 200), (33, 1), (256, 1), (0, 0)]
# (threshold, k, nbins, cap of a 257-record range): the cap is this file's choice -- a short list, every
# record, and the count alone
SETTINGS = [(0.25, 1, 1, 3), (float(np.nextafter(0.25, 1.0)), 16, 64, 257), (0.5, 64, 1024, 0)]
PASSES = ("masks_batch_report", "masks_batch_match", "masks_batch_topk", "masks_batch_hist", "masks_report", "masks_match",
          "masks_topk", "masks_resolve_hist", "resolver_report", "resolver_match", "resolver_topk", "resolver_hist", "masks")
MATCH_FIRST_ROOM = 1024  # kMatchFirstRoom (csrc/iris_api_select.hip); not exported: a change there is made here too
HOOKS = {"tiles-tpw1": 1, "tiles-tpw4": 4}


def open_variant(variant, device, hooked_device, **env):
    if variant in HOOKS:
        return hooked_device(IRIS_TILES_PER_WAVE=HOOKS[variant], **env), ih.LAYOUT_TILES
    return (hooked_device(**env) if env else device), ih.LAYOUT_TILES if variant == "tiles" else ih.LAYOUT_LANES


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    return open_variant(request.param, device, hooked_device) + (request.param,)


@pytest.fixture(scope="module")
def case():
    return SmallCase()


@pytest.fixture
def own_device():
    """A device handle of the test's own: its match buffer starts empty, so launch counts do not
    depend on what ran before, and the buffer the test grows is not the session device's."""
    with ih.Device(0) as dev:
        yield dev


def profiled(device, call):
    """call() under profiling -> (its result, {pass name: launches})."""
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = call()
    finally:
        device.set_profiling(False)
    return res, {name: device.kernel_stats(name)[0] for name in PASSES}


def only(launches, **want):
    """The launch counts are `want` and nothing else ran (the "masks" denominators aside)."""
    got = {name: c for name, c in launches.items() if c and name != "masks"}
    assert got == want, launches


def run(eng, db, ptrs, exps, parts, first, n, threshold=None, cap=None, k=None, nbins=None, base=0):
    """One raw call, every selected part of every query checked against the oracle -> its result."""
    res = mf.raw_report(eng, db, first, n, ptrs, parts, threshold=threshold, cap=cap, k=k, nbins=nbins, index_base=base)
    mf.check(exps[:eng.nq], res, parts, first, n, threshold, cap, k, nbins, base)
    if parts & TOPK:  # the lists' order is the search order: exact fraction, then index (test_gpu_topk.order)
        for q, e in enumerate(exps[:eng.nq]):
            assert [m.index - base + first for m in res.topk[q]] == list(order(e, first, n)[:k]), q
    return res


# ---------------------------------------------------------------- 1. the oracle and the siblings, byte for byte


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 6, 7])
def test_against_oracle_and_siblings(ctx, case, nq):
    device, layout, _ = ctx
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng:
        for first, n in RANGES:
            offset = 2 if first == 5 else 0  # slabs that are not 16-B aligned take the element-wise staging
            with DeviceArrays(device, case.shares[:, :nq, first:first + n], offset) as ptrs:
                for threshold, k, nbins, cap in SETTINGS:
                    cap = min(cap, max(n, 1))
                    sib = mf.siblings(eng, db, first, n, ptrs, BASE, threshold, cap, k, nbins)
                    for parts in MULTI:
                        res = run(eng, db, ptrs, case.exp, parts, first, n, threshold, cap, k, nbins, BASE)
                        mf.same(res, sib, parts)
                    if first == 0 and n:  # the zero-mask record is in no list and counts in invalid
                        assert res.invalid == [1] * nq
                        for q in range(nq):
                            assert case.ZERO + BASE not in [m.index for m in res.matches[q] + res.topk[q]]


def test_one_part_is_the_sibling_call(ctx, case):
    device, layout, _ = ctx
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks) as eng, \
            DeviceArrays(device, case.shares[:, :, 5:205]) as ptrs:
        sib = mf.siblings(eng, db, 5, 200, ptrs, BASE, 0.35, 4, 16, 64)
        for parts in (MATCHES, TOPK, HIST):
            mf.same(run(eng, db, ptrs, case.exp, parts, 5, 200, 0.35, 4, 16, 64, BASE), sib, parts)


# ---------------------------------------------------------------- 2. persistent waves, 6. overflow


class LargeCase:
    """6 queries over PERSIST_N generated masks (4099 tiles; every record has valid rotations): the
    group of queries 0-3 and the group of queries 4-5.  Slab 1 is dense (background uneq under
    0.3 den: every record matches at 0.35), the others sparse (background 0.4-0.6) with planted
    records.  At one tile per wave, wave w walks tiles w, w + 2048 and w + 4096; at two tiles per
    wave (four slots), wave w walks tiles 2 w, 2 w + 1 and then 4096 + 2 w, 4097 + 2 w.  The plants
    of a slot lie in a wave's first and in its later group, different waves for different slots."""

    N, NQ, SEED, DENSE = PERSIST_N, 6, 21, 1
    SPOTS = {0: [5, 4096 * 32 + 3], 2: [33, 4097 * 32 + 8], 3: [70, PERSIST_N - 1], 4: [4097 * 32 + 1, 2048 * 32 + 9], 5: [37]}

    def __init__(self):
        rng = np.random.default_rng(28)
        masks = oc.gen_masks(self.SEED, 0, self.N)
        self.qmasks = rng.integers(0, 2**64, (self.NQ, ih.LIMBS), dtype=np.uint64)
        self.den = np.stack([oc.masks_batch(q, masks) for q in self.qmasks])
        assert (self.den != 0).all()
        uneq = background(rng, self.den, 0.4, 0.6)
        uneq[self.DENSE] = background(rng, self.den[self.DENSE], 0.0, 0.3)
        for q, spots in self.SPOTS.items():
            for j, s in enumerate(spots):
                rot = (7 * q + 11 * j) % ROT
                uneq[q, s, rot] = int(self.den[q, s, rot]) // (8 + q - j)  # a slab's first spot is its best record
        self.shares = planted_shares(rng, self.den, uneq)  # [3, 6, N, 31]
        self.exp = [resolver_expected(self.shares[:, q], self.den[q]) for q in range(self.NQ)]

    def db(self, dev):
        db = ih.Database(dev, ih.KIND_MASKS, self.N, ih.LAYOUT_TILES)
        db.generate(self.N, self.SEED)
        return db


@pytest.fixture(scope="module")
def large():
    return LargeCase()


def test_large_fixture_is_known_by_construction(large):
    for q, e in enumerate(large.exp):
        hits = list(e.hits(0.35))
        assert hits == (list(range(large.N)) if q == large.DENSE else sorted(large.SPOTS[q])), q
        if q != large.DENSE:  # the plants lead the top-k order, better first as planted
            assert list(order(e)[:len(hits)]) == large.SPOTS[q]


@pytest.mark.parametrize("variant", sorted(HOOKS))
def test_persistent_waves_carry_lists_and_bins_across_groups(hooked_device, large, variant):
    """Four slots, some waves walking two or three tile groups: a slot's matches, its list's order and
    its bins hold what the wave found in its first group when it ends its last."""
    dev, _ = open_variant(variant, None, hooked_device)
    nq, n = 4, large.N
    with large.db(dev) as db, ih.MasksBatchEngine(dev, large.qmasks[:nq]) as eng, \
            DeviceArrays(dev, large.shares[:, :nq]) as ptrs:
        res, launches = profiled(dev, lambda: run(eng, db, ptrs, large.exp, ALL, 0, n, 0.35, 8, 16, 64, BASE))
        only(launches, masks_batch_report=1, masks_batch_match=1)  # the dense slab 1 overflows the first room: one rerun
        for q in (0, 2, 3):
            assert [m.index - BASE for m in res.matches[q]] == sorted(large.SPOTS[q])
            assert [m.index - BASE for m in res.topk[q]][:2] == large.SPOTS[q]
            assert int(res.bins[q][:64 * 35 // 100].sum()) == 2  # the two plants alone lie below 0.35
        assert res.matches_counts[large.DENSE] == n and [m.index - BASE for m in res.matches[large.DENSE]] == list(range(8))
        # a sub-range that starts and ends inside tiles (its first record no multiple of 8), two parts
        first, m = 37, n - 37 - 50
        with DeviceArrays(dev, large.shares[:, :nq, first:first + m]) as sub:
            run(eng, db, sub, large.exp, TOPK | HIST, first, m, None, None, 64, 1024, BASE)
            two = run(eng, db, sub, large.exp, MATCHES | TOPK, first, m, 0.35, 8, 1, None, 3)
            assert two.matches_counts[3] == 1 and two.matches[3][0].index == 3 + 70 - first  # N - 1 lies outside


def test_overflow_reruns_only_the_overflowing_group(own_device, large):
    """cap = 1500 is above the first pass's 1024-record room, and the dense slab 1 matches every
    record: group 0 alone runs again, as the plain match pass; the other group's results, the top-k
    lists and the histograms are what a call that never reruns (cap = 0) gives; and the buffer has
    grown, so the next identical call is one pass."""
    dev, n, cap = own_device, large.N, 1500
    assert cap > MATCH_FIRST_ROOM
    with large.db(dev) as db, ih.MasksBatchEngine(dev, large.qmasks) as eng, DeviceArrays(dev, large.shares) as ptrs:
        quiet, launches = profiled(dev, lambda: run(eng, db, ptrs, large.exp, ALL, 0, n, 0.35, 0, 16, 64, BASE))
        only(launches, masks_batch_report=2)
        res, launches = profiled(dev, lambda: run(eng, db, ptrs, large.exp, ALL, 0, n, 0.35, cap, 16, 64, BASE))
        only(launches, masks_batch_report=2, masks_batch_match=1)
        assert res.matches_counts == quiet.matches_counts == [n if q == large.DENSE else len(large.SPOTS[q]) for q in range(6)]
        assert [m.index - BASE for m in res.matches[large.DENSE]] == list(range(cap))
        mf.same(res, quiet, TOPK | HIST)
        again, launches = profiled(dev, lambda: run(eng, db, ptrs, large.exp, ALL, 0, n, 0.35, cap, 16, 64, BASE))
        only(launches, masks_batch_report=2)
        mf.same(again, res, ALL)
        # two parts, and the siblings' bytes
        sib = mf.siblings(eng, db, 0, n, ptrs, BASE, 0.35, cap, 16, 64)
        mf.same(again, sib, ALL)
        mf.same(run(eng, db, ptrs, large.exp, MATCHES | HIST, 0, n, 0.35, cap, None, 64, BASE), sib, MATCHES | HIST)


# ---------------------------------------------------------------- 3. slot isolation


def test_slot_isolation(ctx, case):
    device, layout, _ = ctx
    n = case.N
    with case.db(device, layout) as db, DeviceArrays(device, case.shares) as ptrs:
        with ih.MasksBatchEngine(device, case.qmasks) as eng:
            res = run(eng, db, ptrs, case.exp, ALL, 0, n, 0.35, n, 4, 64)
            lists = [[m.index for m in res.matches[q]] for q in range(case.NQ)]
            assert lists[0] == [] and lists[1] == [0] and lists[2] == list(case.EDGES) and lists[4] == [100, 200]
            assert lists[3] == list(case.many) and lists[5] == [10] + list(case.TIE)
            assert res.topk[1][0].index == 0 and res.topk[4][0].index in (100, 200)
            for q in (0, 1, 2, 4):  # a slot's low bins hold its own plants and nobody else's
                assert int(res.bins[q][:64 * 35 // 100].sum()) == len(lists[q]), q
        # three queries in the four-slot kernel: the unused slot writes nowhere (raw_report's guards
        # stand behind the third query's list, count and row)
        with ih.MasksBatchEngine(device, case.qmasks[:3]) as eng, DeviceArrays(device, case.shares[:, :3]) as three:
            res3 = run(eng, db, three, case.exp, ALL, 0, n, 0.35, n, 4, 64)
            assert res3.matches_bytes == res.matches_bytes[:3] and res3.topk_bytes == res.topk_bytes[:3]
            assert res3.bins.tobytes() == res.bins[:3].tobytes()


def test_sixty_four_queries(ctx, case):
    """The 7 queries cycled: every slab repeats its source's parts."""
    device, layout, _ = ctx
    src = np.arange(64) % case.NQ
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[src]) as eng, \
            DeviceArrays(device, case.shares[:, src]) as ptrs:
        res = run(eng, db, ptrs, [case.exp[s] for s in src], ALL, 0, case.N, 0.35, 50, 16, 64, BASE)
        for q in range(case.NQ, 64):
            assert res.matches_bytes[q] == res.matches_bytes[q - case.NQ] and res.topk_bytes[q] == res.topk_bytes[q - case.NQ]


# ---------------------------------------------------------------- 4. ties through the cut, fewer than k valid


def test_ties_through_the_cut_and_fewer_than_k_valid(ctx, case):
    device, layout, _ = ctx
    a, b = case.TIE
    e5 = case.exp[5]
    assert list(order(e5)[:3]) == [a, b, 10] and e5.dist[a] == e5.dist[b]
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks) as eng:
        with DeviceArrays(device, case.shares) as ptrs:
            for k, want in ((1, [a]), (2, [a, b]), (3, [a, b, 10])):  # the tie is cut at the lower index
                res = run(eng, db, ptrs, case.exp, ALL, 0, case.N, 0.35, 2, k, 64)
                assert [m.index for m in res.topk[5]] == want
                assert [m.index for m in res.matches[5]] == [10, a] and res.matches_counts[5] == 3
                assert res.topk[5][0].rotation == case.tie_rot[0]
        # 10 records, one of them the zero mask: 9 valid for k = 16; then the zero mask alone
        for first, n, valid in ((70, 10, 9), (case.ZERO, 1, 0)):
            with DeviceArrays(device, case.shares[:, :, first:first + n]) as ptrs:
                res = run(eng, db, ptrs, case.exp, ALL, first, n, float("inf"), n, 16, 64, BASE)
                assert res.topk_counts == [valid] * case.NQ and res.matches_counts == [valid] * case.NQ
                assert res.invalid == [n - valid] * case.NQ and [int(r.sum()) for r in res.bins] == [valid] * case.NQ


# ---------------------------------------------------------------- 5. launch families


@pytest.mark.parametrize("variant", VARIANTS)
def test_launch_families(device, hooked_device, case, variant):
    """The suite does not pass on a fallback: which kernels ran, by the profiled launch names."""
    dev, layout = open_variant(variant, device, hooked_device)
    n = case.N
    with case.db(dev, layout) as db, DeviceArrays(dev, case.shares) as ptrs:
        for nq in (7, 5, 2):
            with ih.MasksBatchEngine(dev, case.qmasks[:nq]) as eng:
                for parts in MULTI:
                    _, launches = profiled(dev, lambda: mf.raw_report(eng, db, 0, n, ptrs, parts, threshold=0.35, cap=4, k=5,
                                                                      nbins=64))
                    if variant in HOOKS:  # groups of 2..4 in the batch kernel, a single left-over query alone
                        only(launches, **{"masks_batch_report": (nq + 2) // 4, **({"masks_report": 1} if nq % 4 == 1 else {})})
                    elif variant == "tiles":  # 9 tiles: below the batch kernel's ranges
                        only(launches, masks_report=nq)
                    else:
                        only(launches, resolver_report=nq)
                        assert launches["masks"] == nq
                if nq != 7:
                    continue
                for parts, batch, tiles, lanes in ((MATCHES, "masks_batch_match", "masks_match", "resolver_match"),
                                                   (TOPK, "masks_batch_topk", "masks_topk", "resolver_topk"),
                                                   (HIST, "masks_batch_hist", "masks_resolve_hist", "resolver_hist")):
                    _, launches = profiled(dev, lambda: mf.raw_report(eng, db, 0, n, ptrs, parts, threshold=0.35, cap=4, k=5,
                                                                      nbins=64))
                    only(launches, **({batch: 2} if variant in HOOKS else {tiles: 7} if variant == "tiles" else {lanes: 7}))
                _, launches = profiled(dev, lambda: mf.raw_report(eng, db, 10, 0, ptrs, ALL, threshold=0.35, cap=4, k=5, nbins=64))
                assert not any(launches.values())  # n == 0: nothing is launched


# ---------------------------------------------------------------- 7. IRIS_HIST_COPIES


@pytest.mark.parametrize("variant", ["tiles-tpw1", "tiles-tpw4", "lanes"])
def test_hist_copies_do_not_change_a_byte(device, hooked_device, case, variant):
    results = []
    for copies in (None, 1, 2, 64):
        env = {} if copies is None else {"IRIS_HIST_COPIES": copies}
        dev, layout = open_variant(variant, device, hooked_device, **env)
        with case.db(dev, layout) as db, ih.MasksBatchEngine(dev, case.qmasks) as eng, DeviceArrays(dev, case.shares) as ptrs:
            results.append(run(eng, db, ptrs, case.exp, ALL, 0, case.N, 0.35, 5, 16, 1024, BASE))
            mf.same(run(eng, db, ptrs, case.exp, TOPK | HIST, 0, case.N, None, None, 16, 1024, BASE), results[-1], TOPK | HIST)
    for res in results[1:]:
        mf.same(res, results[0], ALL)


# ---------------------------------------------------------------- 8. refusals with live handles


def test_refusals_write_nothing_and_leave_the_device_usable(ctx, case):
    device, layout, _ = ctx
    nq, n = 3, case.N
    good = dict(threshold=0.35, cap=4, k=5, nbins=64)
    enc = np.zeros((2, ih.BITS), np.uint16)
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
            ih.MasksEngine(device, case.qmasks[0]) as single, ih.DistanceBatchEngine(device, enc) as dbe, \
            ih.Database(device, ih.KIND_TEMPLATES, 300, layout) as tdb, \
            DeviceArrays(device, case.shares[:, :nq]) as ptrs:
        tdb.generate(257, 8)

        def refused(code, word="", e=eng, d=db, p=ptrs, first=0, count=n, parts=ALL, **kw):
            args = dict(good)
            args.update(kw)
            res = mf.raw_report(e, d, first, count, p, parts, nq=nq, expect_rc=code, **args)
            assert res.error and word in res.error, (res.error, word)

        for parts in MULTI + [MATCHES, TOPK, HIST]:
            refused(E_ARG, "masks batch engine", e=single, parts=parts)  # a single-query masks engine
            refused(E_ARG, e=dbe, parts=parts)  # a distance batch engine
            refused(E_ARG, d=tdb, parts=parts)  # a template database
            refused(E_RANGE, first=200, count=100, parts=parts)
            refused(E_RANGE, first=258, count=1, parts=parts)
            refused(E_ARG, p=[ptrs[0], None, ptrs[2]], parts=parts)  # a NULL share pointer
            refused(E_ARG, p=[ptrs[0], ptrs[1] + 1, ptrs[2]], parts=parts)  # a misaligned one
            refused(E_ARG, p=None, nparts=3, parts=parts)
        refused(E_ARG, "parts must be 1..8", nparts=9)
        refused(E_ARG, "parts must be one or more", parts=8)
        refused(E_ARG, "reserved must be 0", reserved=1)
        refused(E_ARG, "threshold is NaN", threshold=float("nan"))
        refused(E_ARG, "IRIS_TOPK_MAX", k=65)
        refused(E_ARG, "IRIS_HIST_MAX_BINS", nbins=48)
        for field in ("matches", "matches_counts", "topk", "topk_counts", "bins", "invalid"):
            refused(E_ARG, "NULL", null=(field,))
        # the single-query report still refuses the batch engine, and names this call
        lib = ih.load_library()
        r = ih.Report()
        r.parts = TOPK
        one = (ih.Match * 5)()
        r.k, r.topk = 5, ctypes.cast(one, ctypes.POINTER(ih.Match))
        rc = lib.iris_resolver_report_masks(eng.handle, db.handle, 0, n, mf.share_array(ptrs), 3, 0, ctypes.byref(r))
        assert rc == E_ARG and mf.NAME.encode() in lib.iris_last_error()
        # afterwards a valid call returns the right answer
        run(eng, db, ptrs, case.exp, ALL, 0, n, **good)


# ---------------------------------------------------------------- 9. the mirrors: a three-party flow


def three_party(device, layout, n, seed, queries):
    """prepare -> every party's batched rows on the device -> (masks database, row pointers, the
    parties' share databases: the caller frees and closes them)."""
    nq = len(queries)
    templates = oc.gen_templates(seed, 0, n)
    shares, masks = oc.prepare_shares(templates, bytes(range(32)))
    enc = np.stack([oc.encode(q) for q in queries])
    ptrs, sdbs = [], [ih.Database(device, ih.KIND_SHARES, n) for _ in range(3)]
    with ih.DistanceBatchEngine(device, enc) as de:
        for p, sdb in enumerate(sdbs):
            sdb.append(shares[p])
            ptrs.append(device.alloc(nq * n * ROT * 2))
            de.batch_process_device(sdb, ptrs[-1])
    mdb = ih.Database(device, ih.KIND_MASKS, n, layout)
    mdb.append(masks)
    return mdb, ptrs, sdbs


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles", "lanes"])
def test_python_mirror_and_cpp_program_in_a_three_party_flow(device, layout, tmp_path):
    """Plaintext templates shared among three parties, each party's rows from its batched
    DistanceEngine, then the report: the Python mirror's records are the raw call's bytes, every
    query's first top-k entry is the batched resolve's record, and tests/cpp/masks_batch_report.cpp
    (its own process, prepare on the device) writes the same bytes through iris_hip.hpp."""
    n, nq, seed, threshold, cap, k, nbins = 300, 5, 8, 0.48, 6, 5, 64
    queries = oc.gen_templates(99, 0, nq)
    mdb, ptrs, sdbs = three_party(device, layout, n, seed, queries)
    try:
        with mdb, ih.MasksBatchEngine(device, queries[:, 200:]) as eng:
            raw = mf.raw_report(eng, mdb, 0, n, ptrs, ALL, threshold=threshold, cap=cap, k=k, nbins=nbins, index_base=BASE)
            res = eng.report(mdb, ptrs, ALL, threshold=threshold, cap=cap, k=k, nbins=nbins, index_base=BASE)
            found = eng.resolve(mdb, ptrs, index_base=BASE)
            assert res.matches_counts == raw.matches_counts and list(res.invalid) == raw.invalid
            assert (res.bins == raw.bins).all() and any(0 < c < n for c in raw.matches_counts)
            for q in range(nq):
                assert b"".join(bytes(m) for m in res.matches[q]) == raw.matches_bytes[q]
                assert b"".join(bytes(m) for m in res.topk[q]) == raw.topk_bytes[q]
                assert bytes(res.topk[q][0]) == bytes(found[q])
            two = eng.report(mdb, ptrs, TOPK | HIST, k=k, nbins=nbins, index_base=BASE)
            assert two.matches is None and two.matches_counts is None and (two.bins == raw.bins).all()
            assert [bytes(m) for m in two.topk[0]] == [bytes(m) for m in res.topk[0]]
            with pytest.raises(ih.IrisError):
                eng.report(mdb, ptrs, ALL, threshold=threshold, cap=cap, k=k, nbins=1000)
    finally:
        for p in ptrs:
            device.free(p)
        for sdb in sdbs:
            sdb.close()
    exe = build_cpp_program(tmp_path)
    (tmp_path / "queries.bin").write_bytes(np.ascontiguousarray(queries).tobytes())
    out = tmp_path / "report.bin"
    r = subprocess.run([str(exe), str(tmp_path / "queries.bin"), str(nq), str(n), str(seed), str(layout), str(BASE),
                        repr(threshold), str(cap), str(k), str(nbins), str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    data, pos = out.read_bytes(), 0

    def word():
        nonlocal pos
        pos += 8
        return int(np.frombuffer(data, np.uint64, 1, pos - 8)[0])

    def take(count):
        nonlocal pos
        pos += count
        return data[pos - count:pos]

    for q in range(nq):
        assert word() == raw.matches_counts[q]
        assert take(word() * mf.SIZE) == raw.matches_bytes[q]
        assert take(word() * mf.SIZE) == raw.topk_bytes[q]
        assert take(8 * nbins) == raw.bins[q].tobytes()
        assert word() == raw.invalid[q]
        assert take(mf.SIZE) == bytes(found[q])
    assert pos == len(data)
