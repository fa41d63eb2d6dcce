"""GPU: threshold matching (iris_template_matches, iris_resolver_matches, iris_resolver_matches_masks):
every record of a range whose distance is below a threshold, in ascending index order, with the exact
total -- against lists built from the CPU oracle's counts (the best rotation recomputed in integer
arithmetic, the lowest rotation on ties), never from the library's own search.

Variants as in test_gpu_masks_batch.py: a TILES database under the library's own dispatch (on these
small ranges the K-split template kernel), TILES with IRIS_TILES_PER_WAVE=1 and =4 (the two one-pass
forms of the template and of the fused masks kernel) and a LANES database (the VALU template kernel;
the masks kernel into a workspace, then the resolver match kernel)."""
import ctypes
import subprocess

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc
from test_matches_abi import build_cpp_program

pytestmark = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
INF = float("inf")
PERSIST_N = 4098 * 32 + 27  # the masks-batch tests' size: past the K-split forms' 1024 tiles
VARIANTS = ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"]
T_THRESHOLDS = [0.0, -1.0, 0.375, 0.475, 0.48, 0.5, 2.0, INF]
R_THRESHOLDS = [0.0, 0.01, 0.5, 2.0, INF]
RANGES = [(0, 257), (5, 200), (33, 1), (256, 1), (0, 0)]


def bits_of(x):
    return np.asarray(x, np.float64).view(np.uint64)


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


# ---------------------------------------------------------------- expected lists from the oracle


class Expected:
    """Per record: the best rotation's (num, den, k) in the exact fraction order with the lowest k on
    ties (den = 0: none) and the f64 distance (+inf when none)."""

    def __init__(self, num, den):
        num, den = np.asarray(num, np.int64), np.asarray(den, np.int64)
        n = num.shape[0]
        bn, bd, bk = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int64)
        for k in range(ROT):
            better = (den[:, k] != 0) & ((bd == 0) | (num[:, k] * bd < bn * den[:, k]))
            bn[better], bd[better], bk[better] = num[better, k], den[better, k], k
        self.num, self.den, self.rot = bn, bd, bk - 15
        with np.errstate(divide="ignore", invalid="ignore"):
            self.dist = np.where(bd != 0, bn.astype(np.float64) / bd.astype(np.float64), np.inf)

    def hits(self, threshold, first=0, n=None):
        """Record indices of [first, first + n) below the threshold (a record without a valid rotation never)."""
        n = len(self.dist) - first if n is None else n
        idx = np.arange(first, first + n)
        return idx[(self.den[idx] != 0) & (self.dist[idx] < threshold)]

    def check(self, got, count, idx, base, cap=None):
        """got / count of a call against the record indices idx (ascending); Match.index = base + record."""
        assert count == len(idx), (count, len(idx))
        want = idx if cap is None else idx[:cap]
        assert len(got) == len(want)
        for m, i in zip(got, want):
            assert m.index == base + int(i), (m, i)
            assert (m.num, m.den, m.rotation, m.reserved) == (self.num[i], self.den[i], self.rot[i], 0), (m, i)
            assert bits_of(m.distance) == bits_of(self.dist[i]), (m, i)


def resolver_expected(shares, den):
    """shares [parts, n, 31], den [n, 31] -> Expected of decode_distance's fractions (src/lib.rs:97-107),
    tied to the oracle's own distances."""
    total = shares.astype(np.int64).sum(axis=0) & 0xFFFF
    d = den.astype(np.int64)
    uneq = ((d - total) & 0xFFFF) >> 1
    e = Expected(uneq, d)
    assert (bits_of(e.dist) == bits_of(oc.resolver_combine(shares, den))).all()
    return e


def _flip_inside_mask(pattern, mask, flips, rng):
    mb = np.unpackbits(mask.view(np.uint8), bitorder="little")
    pb = np.unpackbits(pattern.view(np.uint8), bitorder="little")
    pos = rng.choice(np.flatnonzero(mb), flips, replace=False)
    pb[pos] ^= 1
    return np.packbits(pb, bitorder="little").view(np.uint64)


def _near_copy(query, rotation, flips, rng):
    """The query rotated, with `flips` pattern bits flipped where its mask is set."""
    pattern, mask = oc.bits_rotated(query[:200], rotation), oc.bits_rotated(query[200:], rotation)
    return np.concatenate([_flip_inside_mask(pattern, mask, flips, rng), mask])


class TemplateCase:
    def __init__(self):
        rng = np.random.default_rng(12)
        self.query = oc.gen_templates(99, 0, 1)[0]
        self.templates = oc.gen_templates(8, 0, 257).copy()
        self.random = Expected(*oc.template_counts(self.query, self.templates))  # before planting
        self.planted = {}
        for idx, rot, flips in [(0, -15, 0), (31, 0, 40), (32, 7, 400), (256, 15, 1200)]:
            self.planted[idx] = _near_copy(self.query, rot, flips, rng)
        zero_mask = self.templates[100].copy()
        zero_mask[200:] = 0
        tie = np.concatenate([np.zeros(200, np.uint64), np.full(200, ~np.uint64(0))])
        self.planted[100], self.planted[101] = zero_mask, tie
        for idx, rec in self.planted.items():
            self.templates[idx] = rec
        self.exp = Expected(*oc.template_counts(self.query, self.templates))
        assert (bits_of(self.exp.dist) == bits_of(oc.template_distances(self.query, self.templates))).all()

    def db(self, dev, layout):
        db = ih.Database(dev, ih.KIND_TEMPLATES, 300, layout)
        db.generate(257, 8)
        for idx, rec in self.planted.items():
            db.write(idx, rec[None, :])
        return db


@pytest.fixture(scope="module")
def tcase():
    return TemplateCase()


def test_fixture_is_not_vacuous(tcase):
    """The thresholds cover empty, sparse, dense and full lists on the random records, and the
    planted records are what they are meant to be."""
    r, e = tcase.random, tcase.exp
    counts = [len(r.hits(t)) for t in T_THRESHOLDS]
    assert any(0 < c < 257 for c in counts), counts
    assert len(r.hits(0.375)) == 0 and len(r.hits(0.5)) == 257 and 0 < len(r.hits(0.475)) < len(r.hits(0.48)) < 257
    assert len(e.hits(0.5)) == 256 and 100 not in e.hits(INF) and len(e.hits(INF)) == 256
    assert e.den[100] == 0 and np.isinf(e.dist[100])
    assert e.rot[101] == -15 and e.den[101] != 0  # all 31 rotations tie: the lowest wins
    assert (e.num[0], e.rot[0]) == (0, -15) and e.num[31] == 40 and e.rot[31] == 0 and e.rot[256] == 15
    assert e.dist[0] < e.dist[31] < e.dist[32] < e.dist[256] < 0.375


# ---------------------------------------------------------------- 1. templates


def test_template_matches_against_oracle(ctx, tcase):
    device, layout = ctx
    e = tcase.exp
    edge = float(e.dist[31])  # the planted record's exact distance excludes it, the next f64 includes it
    thresholds = T_THRESHOLDS + [edge, float(np.nextafter(edge, np.inf))]
    with tcase.db(device, layout) as db, ih.TemplateEngine(device, tcase.query) as eng:
        for first, n in RANGES:
            for base in (0, 2**40):
                for t in thresholds:
                    got, count = eng.matches(db, t, first=first, n=n, index_base=base)
                    e.check(got, count, e.hits(t, first, n), base)
        got, _ = eng.matches(db, edge)
        assert 31 not in [m.index for m in got] and 0 in [m.index for m in got]
        got, _ = eng.matches(db, float(np.nextafter(edge, np.inf)))
        assert 31 in [m.index for m in got]
        assert eng.matches(db, 0.0) == ([], 0) and eng.matches(db, -1.0) == ([], 0)
        # a search over the same range agrees with the first entry of the sorted-by-distance list
        best = eng.search(db)
        assert (best.index, best.num, best.den) == (0, e.num[0], e.den[0])


def test_template_cap_and_determinism(ctx, tcase):
    device, layout = ctx
    e = tcase.exp
    idx = e.hits(0.48)
    assert len(idx) >= 20
    with tcase.db(device, layout) as db, ih.TemplateEngine(device, tcase.query) as eng:
        got, count = eng.matches(db, 0.48, cap=3)
        e.check(got, count, idx, 0, cap=3)
        assert eng.matches(db, 0.48, cap=0) == ([], len(idx))
        cnt = ctypes.c_uint64()
        assert ih.load_library().iris_template_matches(eng.handle, db.handle, 0, 257, 0, 0.48, None, 0,
                                                       ctypes.byref(cnt)) == 0 and cnt.value == len(idx)
        # cap past the count: the tail of out stays as it was
        out = (ih.Match * (len(idx) + 5))()
        ctypes.memset(out, 0xA5, ctypes.sizeof(out))
        got, count = eng.matches(db, 0.48, out=out)
        e.check(got, count, idx, 0)
        tail = bytes(out)[len(idx) * 32:]
        assert tail == b"\xa5" * (5 * 32)
        # the same call twice: identical bytes
        again = (ih.Match * (len(idx) + 5))()
        ctypes.memset(again, 0xA5, ctypes.sizeof(again))
        eng.matches(db, 0.48, out=again)
        assert bytes(again) == bytes(out)
        # n == 0 touches nothing
        cnt.value = 99
        assert ih.load_library().iris_template_matches(eng.handle, db.handle, 10, 0, 0, 0.48, out, 5,
                                                       ctypes.byref(cnt)) == 0
        assert cnt.value == 0 and bytes(out) == bytes(again)


def test_template_large_range_and_buffer_regrowth(device):
    """The library's own dispatch past the K-split form (4099 tiles: one tile per wave, several
    workgroups per CU, the last tile partial); at +inf with cap = 10 no first buffer holds the 131k
    records, so the pass runs twice."""
    n, seed = PERSIST_N, 77
    rng = np.random.default_rng(3)
    query = oc.gen_templates(99, 0, 1)[0]
    templates = oc.gen_templates(seed, 0, n)
    spots = [0, 127, 128, 4095 * 32, n - 1]
    with ih.Database(device, ih.KIND_TEMPLATES, n, ih.LAYOUT_TILES) as db, ih.TemplateEngine(device, query) as eng:
        db.generate(n, seed)
        for j, s in enumerate(spots):
            templates[s] = _near_copy(query, 3 * j - 6, 100 + 300 * j, rng)
            db.write(s, templates[s][None, :])
        e = Expected(*oc.template_counts(query, templates))
        tight = float(np.nextafter(e.dist[spots].max(), np.inf))
        idx = e.hits(tight)
        assert list(idx) == spots
        got, count = eng.matches(db, tight, index_base=2**40)
        e.check(got, count, idx, 2**40)
        finite = e.hits(INF)
        assert len(finite) > 100000
        device.reset_stats()
        device.set_profiling(True)
        try:
            got, count = eng.matches(db, INF, cap=10)
        finally:
            device.set_profiling(False)
        e.check(got, count, finite, 0, cap=10)
        assert device.kernel_stats("template_match")[0] == 2
        # a sub-range that starts and ends inside tiles, every record reported
        got, count = eng.matches(db, INF, first=4090 * 32 + 5, n=250)
        e.check(got, count, e.hits(INF, 4090 * 32 + 5, 250), 0)


# ---------------------------------------------------------------- 2. resolver


class ResolverCase:
    def __init__(self):
        self.qmask = oc.gen_templates(99, 0, 1)[0][200:]
        self.masks = oc.gen_masks(8, 0, 257).copy()
        self.zero = 77  # a record without a valid rotation (fused form only: its mask is written as zero)
        self.shares = np.random.default_rng(5).integers(0, 2**16, (3, 257, ROT), dtype=np.uint16)
        self.den = oc.masks_batch(self.qmask, self.masks)
        self.exp = resolver_expected(self.shares, self.den)
        self.masks[self.zero] = 0
        self.den_zero = oc.masks_batch(self.qmask, self.masks)
        self.exp_zero = resolver_expected(self.shares, self.den_zero)


@pytest.fixture(scope="module")
def rcase():
    return ResolverCase()


class DeviceArrays:
    """u16 arrays in device memory, each `offset` bytes past a 16-B aligned allocation."""

    def __init__(self, device, arrays, offset=0):
        self.device, self.raw, self.ptrs = device, [], []
        for a in arrays:
            a = np.ascontiguousarray(a, np.uint16)
            p = device.alloc(a.nbytes + 32)
            assert p % 16 == 0
            self.raw.append(p)
            if a.nbytes:
                device.h2d(p + offset, a)
            self.ptrs.append(p + offset)

    def __enter__(self):
        return self.ptrs

    def __exit__(self, *exc):
        for p in self.raw:
            self.device.free(p)


def test_resolver_fixture_is_not_vacuous(rcase):
    counts = [len(rcase.exp.hits(t)) for t in R_THRESHOLDS]
    assert any(0 < c < 257 for c in counts), counts
    assert counts[0] == 0 and counts[-1] == 257
    assert rcase.exp_zero.den[rcase.zero] == 0 and len(rcase.exp_zero.hits(INF)) == 256


@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "offset2"])
def test_resolver_matches_device_arrays(device, rcase, offset):
    e = rcase.exp
    with DeviceArrays(device, list(rcase.shares) + [rcase.den], offset) as ptrs:
        for t in R_THRESHOLDS:
            for n, base in [(257, 0), (200, 2**40), (1, 5), (0, 0)]:
                got, count = ih.resolver_matches(device, ptrs[:3], ptrs[3], n, t, index_base=base)
                e.check(got, count, e.hits(t, 0, n), base)
        idx = e.hits(0.5)
        got, count = ih.resolver_matches(device, ptrs[:3], ptrs[3], 257, 0.5, cap=3)
        e.check(got, count, idx, 0, cap=3)
        assert ih.resolver_matches(device, ptrs[:3], ptrs[3], 257, 0.5, cap=0) == ([], len(idx))
        # one part and eight parts
        for parts in (1, 8):
            sh = np.random.default_rng(parts).integers(0, 2**16, (parts, 257, ROT), dtype=np.uint16)
            ep = resolver_expected(sh, rcase.den)
            with DeviceArrays(device, sh, offset) as sp:
                got, count = ih.resolver_matches(device, sp, ptrs[3], 257, 0.5)
            ep.check(got, count, ep.hits(0.5), 0)


def test_resolver_matches_masks_fused(ctx, rcase):
    device, layout = ctx
    e = rcase.exp_zero
    with ih.Database(device, ih.KIND_MASKS, 300, layout) as db, ih.MasksEngine(device, rcase.qmask) as eng:
        db.generate(257, 8)
        db.write(rcase.zero, rcase.masks[rcase.zero][None, :])
        rows = np.zeros((257, ROT), np.uint16)
        eng.batch_process(rows, db)
        assert (rows == rcase.den_zero).all()
        for offset in (0, 2):
            for first, n in RANGES:
                with DeviceArrays(device, rcase.shares[:, first:first + n], offset) as ptrs:
                    for t in R_THRESHOLDS:
                        for base in (0, 2**40):
                            got, count = eng.matches(db, ptrs, t, first=first, n=n, index_base=base)
                            # indices are index_base + the row within the range
                            e.check(got, count, e.hits(t, first, n), base - first)
        with DeviceArrays(device, list(rcase.shares) + [rows]) as ptrs:
            for t in R_THRESHOLDS:
                got, count = eng.matches(db, ptrs[:3], t)
                assert rcase.zero not in [m.index for m in got]
                if layout == ih.LAYOUT_TILES:  # equal to iris_resolver_matches over the engine's own rows
                    plain, pcount = ih.resolver_matches(device, ptrs[:3], ptrs[3], 257, t)
                    assert pcount == count and [bytes(m) for m in plain] == [bytes(m) for m in got]
            idx = e.hits(0.5)
            got, count = eng.matches(db, ptrs[:3], 0.5, cap=3)
            e.check(got, count, idx, 0, cap=3)
            a = (ih.Match * (len(idx) + 2))()
            b = (ih.Match * (len(idx) + 2))()
            for o in (a, b):
                ctypes.memset(o, 0x5A, ctypes.sizeof(o))
                eng.matches(db, ptrs[:3], 0.5, out=o)
            assert bytes(a) == bytes(b) and bytes(a)[len(idx) * 32:] == b"\x5a" * 64


def test_three_party_flow(ctx, tcase):
    """Encode the query, share the planted templates among three parties, run each party's
    DistanceEngine on the oracle and sum in the fused call: the matches at 0.48 are those of
    iris_template_matches over the plaintext database."""
    device, layout = ctx
    shares, masks = oc.prepare_shares(tcase.templates, bytes(range(32)))
    enc = oc.encode(tcase.query)
    rows = [oc.distance_batch(enc, shares[p]) for p in range(3)]
    with tcase.db(device, layout) as tdb, ih.TemplateEngine(device, tcase.query) as te, \
            ih.Database(device, ih.KIND_MASKS, 257, layout) as mdb, ih.MasksEngine(device, tcase.query[200:]) as me:
        mdb.append(masks)
        plain, pcount = te.matches(tdb, 0.48)
        with DeviceArrays(device, rows) as ptrs:
            got, count = me.matches(mdb, ptrs, 0.48)
    tcase.exp.check(plain, pcount, tcase.exp.hits(0.48), 0)
    assert count == pcount and [bytes(m) for m in got] == [bytes(m) for m in plain]


# ---------------------------------------------------------------- 3. refusals with live handles


def test_refusals_leave_the_device_usable(ctx, tcase, rcase):
    device, layout = ctx
    lib = ih.load_library()
    out = (ih.Match * 4)()
    cnt = ctypes.c_uint64()
    c = ctypes.byref(cnt)
    tq = np.stack([tcase.query] * 4)
    with tcase.db(device, layout) as tdb, ih.TemplateEngine(device, tcase.query) as te, \
            ih.TemplateBatchEngine(device, tq) as tbe, ih.MasksEngine(device, rcase.qmask) as me, \
            ih.MasksBatchEngine(device, np.stack([rcase.qmask] * 2)) as mbe, \
            ih.Database(device, ih.KIND_MASKS, 300, layout) as mdb, \
            DeviceArrays(device, list(rcase.shares) + [rcase.den]) as ptrs:
        mdb.generate(257, 8)
        arr = (ctypes.c_void_p * 3)(*ptrs[:3])
        null_part = (ctypes.c_void_p * 3)(ptrs[0], None, ptrs[2])
        tm, rm, fm = lib.iris_template_matches, lib.iris_resolver_matches, lib.iris_resolver_matches_masks
        cases = [
            (tm, (tbe.handle, tdb.handle, 0, 257, 0, 0.5, out, 4, c), E_ARG),  # a batch engine
            (tm, (me.handle, tdb.handle, 0, 257, 0, 0.5, out, 4, c), E_ARG),  # an engine of another kind
            (tm, (te.handle, mdb.handle, 0, 257, 0, 0.5, out, 4, c), E_ARG),  # a database of another kind
            (tm, (te.handle, tdb.handle, 200, 100, 0, 0.5, out, 4, c), E_RANGE),
            (tm, (te.handle, tdb.handle, 0, 257, 0, float("nan"), out, 4, c), E_ARG),
            (tm, (te.handle, tdb.handle, 0, 257, 0, 0.5, None, 4, c), E_ARG),
            (tm, (te.handle, tdb.handle, 0, 257, 0, 0.5, out, 4, None), E_ARG),
            (fm, (mbe.handle, mdb.handle, 0, 257, arr, 3, 0, 0.5, out, 4, c), E_ARG),  # a masks batch engine
            (fm, (te.handle, mdb.handle, 0, 257, arr, 3, 0, 0.5, out, 4, c), E_ARG),
            (fm, (me.handle, tdb.handle, 0, 257, arr, 3, 0, 0.5, out, 4, c), E_ARG),
            (fm, (me.handle, mdb.handle, 200, 100, arr, 3, 0, 0.5, out, 4, c), E_RANGE),
            (fm, (me.handle, mdb.handle, 0, 257, arr, 9, 0, 0.5, out, 4, c), E_ARG),
            (fm, (me.handle, mdb.handle, 0, 257, null_part, 3, 0, 0.5, out, 4, c), E_ARG),
            (fm, (me.handle, mdb.handle, 0, 257, None, 3, 0, 0.5, out, 4, c), E_ARG),
            (rm, (device.handle, null_part, 3, ptrs[3], 257, 0, 0.5, out, 4, c), E_ARG),
            (rm, (device.handle, arr, 3, None, 257, 0, 0.5, out, 4, c), E_ARG),
            (rm, (device.handle, arr, 0, ptrs[3], 257, 0, 0.5, out, 4, c), E_ARG),
        ]
        for f, args, code in cases:
            assert f(*args) == code, (f.__name__, args[2:6])
            assert lib.iris_last_error(), f.__name__
        got, count = te.matches(tdb, 0.48)
        tcase.exp.check(got, count, tcase.exp.hits(0.48), 0)


# ---------------------------------------------------------------- 4. the C++ program


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_matches(layout, tmp_path):
    """iris_hip.hpp's TemplateEngine::matches, MasksEngine::matches and resolver_matches, run as
    their own process on 257-record databases."""
    n, seed, threshold, rthreshold = 257, 41, 0.48, 0.125
    exe = build_cpp_program(tmp_path)
    path = tmp_path / "matches.bin"
    r = subprocess.run([str(exe), str(path), str(n), str(seed), str(layout), repr(threshold), repr(rthreshold)], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = path.read_bytes()

    def take(pos):
        count = int(np.frombuffer(raw, np.uint64, 1, pos)[0])
        return count, pos + 8

    def records(pos, k):
        return [ih.Match.from_buffer_copy(raw, pos + 32 * i) for i in range(k)], pos + 32 * k

    query = oc.gen_templates(seed + 1, 3, 1)[0].copy()
    query[0] = ~query[0]
    te = Expected(*oc.template_counts(query, oc.gen_templates(seed, 0, n)))
    idx = te.hits(threshold, 1, n - 1)
    assert 0 < len(idx) < n - 1
    count, pos = take(0)
    got, pos = records(pos, count)
    te.check(got, count, idx, 1000)
    count, pos = take(pos)
    got, pos = records(pos, min(count, 3))
    te.check(got, count, idx, 1000, cap=3)

    e = np.arange(n * ROT, dtype=np.uint64)
    shares = np.stack([(((e * 2654435761) & 0xFFFFFFFF) >> 7) + 12345 * p for p in range(2)]).astype(np.uint16)
    shares = shares.reshape(2, n, ROT)
    re_ = resolver_expected(shares, oc.masks_batch(np.full(200, ~np.uint64(0)), oc.gen_masks(seed, 0, n)))
    ridx = re_.hits(rthreshold)
    assert 0 < len(ridx) < n
    count, pos = take(pos)
    got, pos = records(pos, count)
    re_.check(got, count, ridx, 7)
    assert pos == len(raw)
