"""GPU: batched top-k (iris_resolver_batch_topk_masks): for every query of a masks batch engine, the k
closest records of the resolver step, best first -- byte for byte against lists built from the CPU
oracle (oc.masks_batch for the denominators, the integer best-rotation restatement of
test_gpu_matches.py, ordered by the exact fraction through integer cross products and then the
index: test_gpu_topk.order) and against the single-query iris_resolver_topk_masks calls it replaces.

Variants as in test_gpu_masks_batch_matches.py: a TILES database under the library's own dispatch
(on the small fixture one fused single-query launch per query), TILES with IRIS_TILES_PER_WAVE=1 and
=4 (the hook pins masks_batch_kernel<G, T, BATCH_TOPK> at one tile per wave and at its large form on
ranges of any size: groups of four queries, a left-over three in the four-slot kernel, a left-over
two in the two-slot kernel, a left-over one in the single-query kernel) and a LANES database (the
masks kernel into a workspace, then the resolver top-k kernel, per query).

Share slabs with known lists are built as in test_gpu_masks_batch_matches.py: a target uneq per
(query, record, rotation), parts 0 and 1 uniform random, part 2 the rest (planted_shares)."""
import ctypes
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_matches import DeviceArrays, Expected, resolver_expected
from test_gpu_masks_batch_matches import (MATCH_DT, PERSIST_N, RANGES, ROT, VARIANTS, SmallCase, background,
                                          planted_shares, slab_ptrs, want_records)
from test_gpu_topk import BASE, KS, order
from test_masks_batch_topk_abi import build_cpp_program

gpu = pytest.mark.gpu
E_ARG, E_RANGE = -1, -5
FILL = 0x5A
UNTOUCHED = bytes([FILL]) * 32


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES, v
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES, v
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES, v


@pytest.fixture(scope="module")
def case():
    return SmallCase()


# ---------------------------------------------------------------- helpers


def batch_call(eng, db, ptrs, k, first=0, n=None, base=0, extra=1):
    """One batched call into a 0x5A-filled buffer of nq + extra query rooms ->
    (counts, raw bytes of the nq rooms, raw bytes of the extra rooms)."""
    n = len(db) - first if n is None else n
    nq = eng.nq
    out = (ih.Match * ((nq + extra) * k))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint32 * (nq + extra))(*([99] * (nq + extra)))
    arr = (ctypes.c_void_p * max(len(ptrs), 1))(*ptrs)
    rc = ih.load_library().iris_resolver_batch_topk_masks(eng.handle, db.handle, first, n, arr, len(ptrs), base, k, out,
                                                          counts)
    assert rc == 0, ih.load_library().iris_last_error()
    assert list(counts)[nq:] == [99] * extra
    raw = bytes(out)
    return list(counts)[:nq], raw[:nq * k * 32], raw[nq * k * 32:]


def room(raw, q, k):
    return raw[q * k * 32:(q + 1) * k * 32]


def want_bytes(e, k, first, n, base):
    """(count, bytes) of the oracle's list: the first k records of order(e) in the range."""
    idx = order(e, first, n)[:k]
    return len(idx), want_records(e, idx, first, base).tobytes()


def check_against_oracle(counts, raw, tail, exps, k, first, n, base):
    for q, e in enumerate(exps):
        c, want = want_bytes(e, k, first, n, base)
        assert counts[q] == c, (q, k, first, n)
        r = room(raw, q, k)
        assert r[:32 * c] == want, (q, k, first, n)
        assert r[32 * c:] == UNTOUCHED * (k - c), (q, "entries past the count were written")
    assert tail == UNTOUCHED * (len(tail) // 32), "records were written past the last query's room"


# ---------------------------------------------------------------- 1. oracle and the single calls


@gpu
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 7])
def test_against_oracle_and_single_calls(ctx, case, nq):
    device, layout, _ = ctx
    singles = [ih.MasksEngine(device, case.qmasks[q]) for q in range(nq)]
    try:
        with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng:
            for first, n in RANGES:
                with DeviceArrays(device, case.shares[:, :nq, first:first + n]) as ptrs:
                    best = eng.resolve(db, ptrs, first=first, n=n, index_base=BASE)
                    full = None
                    for k in reversed(KS):
                        counts, raw, tail = batch_call(eng, db, ptrs, k, first, n, BASE)
                        check_against_oracle(counts, raw, tail, case.exp[:nq], k, first, n, BASE)
                        assert batch_call(eng, db, ptrs, k, first, n, BASE) == (counts, raw, tail)  # identical bytes
                        if full is None:
                            full = raw  # k = 64
                        for q in range(nq):
                            r = room(raw, q, k)
                            one = singles[q].topk(db, slab_ptrs(ptrs, q, n), k, first=first, n=n, index_base=BASE)
                            assert len(one) == counts[q], (q, k, first, n)
                            assert b"".join(bytes(m) for m in one) == r[:32 * counts[q]], (q, k, first, n)
                            assert r[:32 * counts[q]] == room(full, q, 64)[:32 * counts[q]]  # a prefix of the k = 64 list
                            if counts[q]:
                                assert r[:32] == bytes(best[q]), (q, k, first, n)
                            else:
                                assert n == 0 or best[q].distance == float("inf")
    finally:
        for s in singles:
            s.close()


# ---------------------------------------------------------------- 2. persistence


class LargeCase:
    """6 queries (a group of four and a pair) over PERSIST_N generated masks; the background uneq lies
    in [0.4, 0.6) den and every query's winners are planted below 0.21: in the first tiles, in tile
    groups that later waves and later rounds of a persistent wave take, in the last full tile and in
    the last, partial tile -- at different records per query.  Query 1 holds two winners in one tile."""

    N, NQ, SEED = PERSIST_N, 6, 21

    @staticmethod
    def spots(q):
        n = PERSIST_N
        s = [5 + 7 * q, 37 + 64 * q, 1500 * 32 + q, 2049 * 32 + 3 * q, 4095 * 32 + 31 - 32 * q, 4097 * 32 + 1 + q,
             4098 * 32 + q, n - 1 - 2 * q - (q == 0)]
        if q == 1:
            s.append(37 + 64 + 3)  # the tile of 37 + 64
        return sorted(set(s))

    def __init__(self):
        rng = np.random.default_rng(16)
        masks = oc.gen_masks(self.SEED, 0, self.N)
        self.qmasks = rng.integers(0, 2**64, (self.NQ, ih.LIMBS), dtype=np.uint64)
        self.den = np.stack([oc.masks_batch(q, masks) for q in self.qmasks])
        assert (self.den != 0).all()
        uneq = background(rng, self.den, 0.4, 0.6)
        for q in range(self.NQ):
            for j, s in enumerate(self.spots(q)):
                k = (5 * q + j) % ROT
                uneq[q, s, k] = int(self.den[q, s, k]) // (5 + ((3 * j + q) % 9))
        self.shares = planted_shares(rng, self.den, uneq)  # [3, 6, N, 31]
        self.exp = [resolver_expected(self.shares[:, q], self.den[q]) for q in range(self.NQ)]


@pytest.fixture(scope="module")
def large():
    return LargeCase()


@gpu
@pytest.mark.parametrize("tpw", [1, 4])
def test_persistent_waves_keep_their_lists(hooked_device, large, tpw):
    device, n = hooked_device(IRIS_TILES_PER_WAVE=tpw), large.N
    for q, e in enumerate(large.exp):  # CPU: the planted records are each query's winners
        sp = large.spots(q)
        assert sorted(order(e)[:len(sp)]) == sp and e.dist[sp].max() < 0.21
    assert {101, 104} <= set(large.spots(1)) and 101 // 32 == 104 // 32  # slot 1: two winners in one full tile
    with ih.Database(device, ih.KIND_MASKS, n, ih.LAYOUT_TILES) as db, ih.MasksBatchEngine(device, large.qmasks) as eng:
        db.generate(n, large.SEED)
        with DeviceArrays(device, large.shares) as ptrs:
            device.reset_stats()
            device.set_profiling(True)
            try:
                counts, raw, tail = batch_call(eng, db, ptrs, 64, 0, n, BASE)
            finally:
                device.set_profiling(False)
            check_against_oracle(counts, raw, tail, large.exp, 64, 0, n, BASE)
            # two units (four queries, two queries); on the MI355X's 256 CUs each unit's pass writes
            # 1028..2048 lists per query: 64 at a time, two merge levels, one launch per level and unit
            assert device.kernel_stats("masks_batch_topk")[0] == 2 and device.kernel_stats("masks_topk")[0] == 0
            assert device.kernel_stats("topk_merge")[0] == 4
            counts, raw, tail = batch_call(eng, db, ptrs, 5, 0, n, 0)
            check_against_oracle(counts, raw, tail, large.exp, 5, 0, n, 0)
            for q in (1, 5):
                with ih.MasksEngine(device, large.qmasks[q]) as single:
                    one = single.topk(db, slab_ptrs(ptrs, q, n), 5)
                assert b"".join(bytes(m) for m in one) == room(raw, q, 5)
        first, m = 37, n - 37 - 50  # starts and ends inside tiles, its first record no multiple of 8
        with DeviceArrays(device, large.shares[:, :, first:first + m]) as ptrs:
            counts, raw, tail = batch_call(eng, db, ptrs, 16, first, m, 5)
            check_against_oracle(counts, raw, tail, large.exp, 16, first, m, 5)


# ---------------------------------------------------------------- 3. slot isolation


class IsolationCase:
    """SmallCase's masks and the first four of its queries; the distances of query 0 rise with the
    record index, those of query 1 fall, query 2 is random and query 3 rises from the middle."""

    NQ = 4

    def __init__(self, case):
        rng = np.random.default_rng(33)
        n = case.N
        den = case.den[:self.NQ].astype(np.int64)
        rec = np.arange(n)
        frac = np.stack([0.1 + 0.3 * rec / n, 0.1 + 0.3 * (n - rec) / n, 0.1 + 0.3 * rng.random(n),
                         0.1 + 0.3 * np.abs(rec - n // 2) / n])
        uneq = (den * frac[:, :, None]).astype(np.int64)
        self.shares = planted_shares(rng, case.den[:self.NQ], uneq)
        self.exp = [resolver_expected(self.shares[:, q], case.den[q]) for q in range(self.NQ)]


@pytest.fixture(scope="module")
def isolation(case):
    return IsolationCase(case)


@gpu
def test_slot_isolation_and_untouched_output(ctx, case, isolation):
    device, layout, _ = ctx
    o0, o1 = order(isolation.exp[0]), order(isolation.exp[1])
    assert not set(o0[:16]) & set(o1[:16]) and set(o0[:16]) <= set(o1[-40:]) and set(o1[:16]) <= set(o0[-40:])
    n = case.N
    assert n % 2 == 1 and (n * ROT * 2) % 16 != 0  # slab 0 starts 16-B aligned, slabs 1 and 2 do not
    for nq in (3, 4):
        with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
                DeviceArrays(device, isolation.shares[:, :nq]) as ptrs:
            assert ptrs[0] % 16 == 0 and slab_ptrs(ptrs, 1, n)[0] % 16 != 0
            for k in (8, 64):
                counts, raw, tail = batch_call(eng, db, ptrs, k, 0, n, 0, extra=2)  # nq = 3: nothing for a fourth query
                check_against_oracle(counts, raw, tail, isolation.exp[:nq], k, 0, n, 0)
                assert len({room(raw, q, k) for q in range(nq)}) == nq
        # a range of 40 records: every count is below k = 64 and the rest of each room keeps its fill
        with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
                DeviceArrays(device, isolation.shares[:, :nq, 8:48]) as ptrs:
            counts, raw, tail = batch_call(eng, db, ptrs, 64, 8, 40, 3)
            assert counts == [40] * nq
            check_against_oracle(counts, raw, tail, isolation.exp[:nq], 64, 8, 40, 3)


# ---------------------------------------------------------------- 4. ties through the cut


class TieCase:
    """6 of SmallCase's queries.  In queries 2 (slot 2 of the group of four) and 5 (slot 1 of the pair)
    ten records hold the fraction 1/5 exactly, at rotations whose denominators differ, and three
    records lie below it; everything else lies above 0.4."""

    NQ = 6
    TIES = [3, 40, 41, 64, 95, 130, 131, 200, 250, 256]
    BETTER = [10, 128, 255]

    def __init__(self, case):
        rng = np.random.default_rng(44)
        den = case.den[:self.NQ]
        d = den.astype(np.int64)
        uneq = background(rng, den, 0.4, 0.6)
        self.rot = {}
        for q in (2, 5):
            for rec in self.TIES:
                k = next(k for k in range(ROT) if d[q, rec, k] % 5 == 0 and d[q, rec, k] > 0)
                uneq[q, rec, k] = d[q, rec, k] // 5
            for j, rec in enumerate(self.BETTER):
                uneq[q, rec, 7 * j] = d[q, rec, 7 * j] // (6 + j)
        self.shares = planted_shares(rng, den, uneq)
        self.exp = [resolver_expected(self.shares[:, q], den[q]) for q in range(self.NQ)]


@pytest.fixture(scope="module")
def ties(case):
    return TieCase(case)


@gpu
def test_ties_through_the_cut(ctx, case, ties):
    device, layout, _ = ctx
    for q in (2, 5):  # CPU: the fixture holds the tie
        e = ties.exp[q]
        assert sorted(order(e)[:3]) == ties.BETTER and list(order(e)[3:13]) == ties.TIES
        assert (e.num[ties.TIES] * 5 == e.den[ties.TIES]).all() and len(set(e.den[ties.TIES])) > 3
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:ties.NQ]) as eng, \
            DeviceArrays(device, ties.shares) as ptrs:
        for k in (1, 4, 5, 8, 12, 13, 14):
            counts, raw, tail = batch_call(eng, db, ptrs, k)
            check_against_oracle(counts, raw, tail, ties.exp, k, 0, case.N, 0)
        lists = eng.topk(db, ptrs, 8)
        for q in (2, 5):  # the cut falls inside the tie of ten: the lowest indices win
            assert [m.index for m in lists[q]][3:] == ties.TIES[:5]


# ---------------------------------------------------------------- 5. fewer than k valid


@gpu
def test_fewer_than_k_valid(ctx):
    """Query 1's mask lies in matrix row 0 alone (limbs 0..2) and all but three records have no mask bit
    there (limbs 0..3 zero; rotations stay inside a row): its count is 3.  Query 3's mask is zero: count
    0.  The other queries list k records."""
    device, layout, _ = ctx
    n, keep = 200, [7, 64, 199]
    rng = np.random.default_rng(55)
    masks = oc.gen_masks(8, 0, n).copy()
    full = masks[keep].copy()
    masks[:, :4] = 0
    masks[keep] = full
    qmasks = rng.integers(0, 2**64, (5, ih.LIMBS), dtype=np.uint64)
    qmasks[1, 3:] = 0
    qmasks[3] = 0
    den = np.stack([oc.masks_batch(q, masks) for q in qmasks])
    shares = rng.integers(0, 2**16, (3, 5, n, ROT), dtype=np.uint16)
    exps = [resolver_expected(shares[:, q], den[q]) for q in range(5)]
    assert [len(order(e)) for e in exps] == [n, 3, n, 0, n] and sorted(order(exps[1])) == keep
    with ih.Database(device, ih.KIND_MASKS, n, layout) as db, ih.MasksBatchEngine(device, qmasks) as eng, \
            DeviceArrays(device, shares) as ptrs:
        db.append(masks)
        for k in (1, 3, 4, 64):
            counts, raw, tail = batch_call(eng, db, ptrs, k)
            check_against_oracle(counts, raw, tail, exps, k, 0, n, 0)
            assert counts == [k, min(k, 3), k, 0, k]
        assert room(raw, 3, 64) == UNTOUCHED * 64
        best = eng.resolve(db, ptrs)
        assert best[3].distance == float("inf") and bytes(best[1]) == room(raw, 1, 64)[:32]


# ---------------------------------------------------------------- 6. every record inserts


@gpu
def test_every_record_inserts_in_one_slot(ctx):
    """4096 rows over all-ones masks (den = 12800 at every rotation): in slot 1 the distance strictly
    falls with the index -- every row beats all before it, an insertion per record -- while slots 0
    and 2 rise."""
    device, layout, _ = ctx
    n, nq = 4096, 3
    asc, desc = 2 * (1 + np.arange(n)), 2 * (n - np.arange(n))
    u = np.stack([asc, desc, asc + 1])
    total = (12800 - 2 * np.repeat(u[:, :, None], ROT, axis=2)) & 0xFFFF
    shares = np.random.default_rng(4).integers(0, 2**16, (2, nq, n, ROT), dtype=np.uint16)
    shares[1] = (total - shares[0].astype(np.int64)) & 0xFFFF
    den = np.full((n, ROT), 12800, np.uint16)
    exps = [resolver_expected(shares[:, q], den) for q in range(nq)]
    assert list(order(exps[1])[:3]) == [n - 1, n - 2, n - 3] and list(order(exps[0])[:3]) == [0, 1, 2]
    ones = np.full(ih.LIMBS, ~np.uint64(0))
    with ih.Database(device, ih.KIND_MASKS, n, layout) as db, ih.MasksBatchEngine(device, np.stack([ones] * nq)) as eng, \
            DeviceArrays(device, shares) as ptrs:
        db.append(np.tile(ones, (n, 1)))
        for k in (1, 16, 64):
            counts, raw, tail = batch_call(eng, db, ptrs, k, 0, n, BASE)
            check_against_oracle(counts, raw, tail, exps, k, 0, n, BASE)
        first, m = 1000, 2077
        with DeviceArrays(device, shares[:, :, first:first + m]) as sub:
            counts, raw, tail = batch_call(eng, db, sub, 33, first, m, 0)
            check_against_oracle(counts, raw, tail, exps, 33, first, m, 0)


# ---------------------------------------------------------------- 7. nq = 64


@gpu
def test_sixty_four_queries(ctx, case):
    """The 7 queries cycled: every slab repeats its source's list."""
    device, layout, _ = ctx
    src = np.arange(64) % case.NQ
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[src]) as eng, \
            DeviceArrays(device, case.shares[:, src]) as ptrs:
        counts, raw, tail = batch_call(eng, db, ptrs, 64)
        check_against_oracle(counts, raw, tail, [case.exp[s] for s in src], 64, 0, case.N, 0)


# ---------------------------------------------------------------- 8. three-party flow


@gpu
def test_three_party_flow(ctx):
    """Plaintext templates shared among three parties, each party's rows from its batched
    DistanceEngine for 5 queries, summed and ranked in the batched call: every query's list is
    iris_template_topk's over the plaintext database."""
    device, layout, _ = ctx
    n, nq, k = 257, 5, 33
    templates = oc.gen_templates(8, 0, n)
    queries = oc.gen_templates(99, 0, nq)
    shares, masks = oc.prepare_shares(templates, bytes(range(32)))
    enc = np.stack([oc.encode(q) for q in queries])
    ptrs = []
    sdbs = [ih.Database(device, ih.KIND_SHARES, n) for _ in range(3)]
    try:
        with ih.DistanceBatchEngine(device, enc) as de:
            for p, sdb in enumerate(sdbs):
                sdb.append(shares[p])
                ptrs.append(device.alloc(nq * n * ROT * 2))
                de.batch_process_device(sdb, ptrs[-1])
        with ih.Database(device, ih.KIND_TEMPLATES, n, layout) as tdb, ih.Database(device, ih.KIND_MASKS, n, layout) as mdb, \
                ih.MasksBatchEngine(device, queries[:, 200:]) as me:
            tdb.append(templates)
            mdb.append(masks)
            lists = me.topk(mdb, ptrs, k)
            for q in range(nq):
                with ih.TemplateEngine(device, queries[q]) as te:
                    plain = te.topk(tdb, k)
                e = Expected(*oc.template_counts(queries[q], templates))
                assert [m.index for m in plain] == list(order(e)[:k])
                assert [bytes(m) for m in lists[q]] == [bytes(m) for m in plain], q
    finally:
        for p in ptrs:
            device.free(p)
        for db in sdbs:
            db.close()


# ---------------------------------------------------------------- 9. launch families


@gpu
@pytest.mark.parametrize("nq", [5, 7])
def test_launch_families(ctx, case, nq):
    """Ranges the batch kernel runs: one masks_batch_topk pass per group of 2..4 queries, masks_topk for
    a single left-over query, and per unit one topk_merge launch per level (257 records: at most 64
    lists, one level).  Elsewhere the single-query families, per query."""
    device, layout, variant = ctx
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
            DeviceArrays(device, case.shares[:, :nq]) as ptrs:
        device.reset_stats()
        device.set_profiling(True)
        try:
            eng.topk(db, ptrs, 16)
        finally:
            device.set_profiling(False)
        got = {f: device.kernel_stats(f)[0] for f in ("masks_batch_topk", "masks_topk", "masks", "resolver_topk",
                                                      "topk_merge", "masks_batch_resolve", "reduce")}
    groups, single = (nq + 3) // 4 - (nq % 4 == 1), int(nq % 4 == 1)
    if variant.startswith("tiles-tpw"):
        want = dict(masks_batch_topk=groups, masks_topk=single, masks=0, resolver_topk=0, topk_merge=groups + single)
    elif variant == "tiles":
        want = dict(masks_batch_topk=0, masks_topk=nq, masks=0, resolver_topk=0, topk_merge=nq)
    else:
        want = dict(masks_batch_topk=0, masks_topk=0, masks=nq, resolver_topk=nq, topk_merge=nq)
    want.update(masks_batch_resolve=0, reduce=0)
    assert got == want


# ---------------------------------------------------------------- 10. refusals with live handles


@gpu
def test_refusals_leave_the_device_usable(ctx, case):
    dev, layout, _ = ctx
    lib = ih.load_library()
    f = lib.iris_resolver_batch_topk_masks
    nq = 3
    out = (ih.Match * (nq * 4))()
    ctypes.memset(out, FILL, ctypes.sizeof(out))
    counts = (ctypes.c_uint32 * nq)(*([99] * nq))
    enc = np.zeros((2, ih.BITS), np.uint16)
    with ih.Device(0) as other, ih.Database(other, ih.KIND_MASKS, 300, layout) as odb, \
            case.db(dev, layout) as db, ih.MasksBatchEngine(dev, case.qmasks[:nq]) as eng, \
            ih.MasksEngine(dev, case.qmasks[0]) as single, ih.DistanceBatchEngine(dev, enc) as dbe, \
            DeviceArrays(dev, case.shares[:, :nq]) as ptrs:
        odb.generate(257, 8)
        arr = (ctypes.c_void_p * 3)(*ptrs)
        null_part = (ctypes.c_void_p * 3)(ptrs[0], None, ptrs[2])
        cases = [
            ((single.handle, db.handle, 0, 257, arr, 3, 0, 4, out, counts), E_ARG),  # a single-query masks engine
            ((dbe.handle, db.handle, 0, 257, arr, 3, 0, 4, out, counts), E_ARG),  # a distance batch engine
            ((eng.handle, odb.handle, 0, 257, arr, 3, 0, 4, out, counts), E_ARG),  # a database on another device
            ((eng.handle, db.handle, 200, 100, arr, 3, 0, 4, out, counts), E_RANGE),  # a range past the end
            ((eng.handle, db.handle, 0, 257, null_part, 3, 0, 4, out, counts), E_ARG),  # a NULL share array
            ((eng.handle, db.handle, 0, 257, None, 3, 0, 4, out, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 9, 0, 4, out, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 3, 0, 65, out, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 3, 0, 4, None, counts), E_ARG),
            ((eng.handle, db.handle, 0, 257, arr, 3, 0, 4, out, None), E_ARG),
        ]
        for args, code in cases:
            assert f(*args) == code, args[2:8]
            assert lib.iris_last_error(), args[2:8]
        assert list(counts) == [99] * nq and bytes(out) == bytes([FILL]) * ctypes.sizeof(out)
        # the single-query call still refuses the batch engine, and names this call
        one = ctypes.c_uint32()
        assert lib.iris_resolver_topk_masks(eng.handle, db.handle, 0, 257, arr, 3, 0, 4, out, ctypes.byref(one)) == E_ARG
        assert b"iris_resolver_batch_topk_masks" in lib.iris_last_error()
        # afterwards a valid call returns the right answer
        got, raw, tail = batch_call(eng, db, ptrs, 4)
        check_against_oracle(got, raw, tail, case.exp[:nq], 4, 0, case.N, 0)


# ---------------------------------------------------------------- 11. the C++ program


@gpu
@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_masks_batch_topk(layout, device, tmp_path):
    """iris_hip.hpp's MasksBatchEngine::topk, run as its own process: every query's k-list and the list
    of k = 2, against the Python call on the same inputs and against the oracle."""
    nq, n, seed, k = 5, 300, 41, 33
    exe = build_cpp_program(tmp_path)
    path = tmp_path / "lists.bin"
    r = subprocess.run([str(exe), str(path), str(nq), str(n), str(seed), str(layout), str(k)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = path.read_bytes()
    i = np.arange(ih.LIMBS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        qm = np.stack([((i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * j + 1)) ^ np.uint64(j << 7)
                       for j in range(nq)])
    el = np.arange(nq * n * ROT, dtype=np.uint64)
    shares = np.stack([(((el * 2654435761) & 0xFFFFFFFF) >> 7) + 12345 * p for p in range(2)]).astype(np.uint16)
    shares = shares.reshape(2, nq, n, ROT)
    masks = oc.gen_masks(seed, 0, n)
    exps = [resolver_expected(shares[:, q], oc.masks_batch(qm[q], masks)) for q in range(nq)]
    with ih.Database(device, ih.KIND_MASKS, n, layout) as db, ih.MasksBatchEngine(device, qm) as eng, \
            DeviceArrays(device, shares) as ptrs:
        db.generate(n, seed)
        mirror = {kk: eng.topk(db, ptrs, kk, index_base=7) for kk in (k, 2)}
    pos = 0
    for kk in (k, 2):
        for q in range(nq):
            count = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
            got = raw[pos + 8:pos + 8 + 32 * count]
            pos += 8 + 32 * count
            assert count == kk and got == b"".join(bytes(m) for m in mirror[kk][q]), (kk, q)
            assert got == want_bytes(exps[q], kk, 0, n, 7)[1], (kk, q)
    assert pos == len(raw)
