"""GPU: the resolver histograms (iris_resolver_histogram, iris_resolver_histogram_masks,
iris_resolver_batch_histogram_masks) against histograms built from the CPU oracle alone
(resolver_hist_fixtures.py: oc.masks_batch for the denominators, resolver_expected's distances,
hist_fixtures.expected's binning), against each other byte for byte, and against the totals of the
sibling threshold-match calls.

Variants as in test_gpu_masks_batch_matches.py: a TILES database under the library's own dispatch
(on the small fixture one fused single-query launch per query), TILES with IRIS_TILES_PER_WAVE=1 and
=4 (the hook pins masks_batch_kernel<G, T, BATCH_HIST> and masks_mfma_kernel<MASKS_HIST> at one tile
per wave and at their large forms on ranges of any size) and a LANES database (the masks kernel into
a workspace, then resolver_kernel's histogram mode, per query)."""
import ctypes
import subprocess

import numpy as np
import pytest

import hist_fixtures as hf
import iris_hip as ih
import resolver_hist_fixtures as rf
from oracle import oracle_c as oc
from test_gpu_masks_batch_matches import planted_shares, slab_ptrs
from test_gpu_matches import DeviceArrays, resolver_expected
from test_resolver_histogram_abi import build_cpp_program

gpu = pytest.mark.gpu
ROT = 31
E_ARG, E_RANGE = -1, -5
INF = float("inf")
GUARD = 0xA5A5A5A5A5A5A5A5
VARIANTS = ["tiles", "tiles-tpw1", "tiles-tpw4", "lanes"]


@pytest.fixture(params=VARIANTS)
def ctx(request, device, hooked_device):
    v = request.param
    if v == "tiles-tpw1":
        return hooked_device(IRIS_TILES_PER_WAVE=1), ih.LAYOUT_TILES
    if v == "tiles-tpw4":
        return hooked_device(IRIS_TILES_PER_WAVE=4), ih.LAYOUT_TILES
    return device, ih.LAYOUT_TILES if v == "tiles" else ih.LAYOUT_LANES


@pytest.fixture(scope="module")
def case():
    return rf.small_case()


def same(got, want):
    """A call's (bins, invalid) against the oracle's."""
    return got[0].dtype == np.uint64 and got[0].tobytes() == want[0].tobytes() and int(got[1]) == want[1]


# ---------------------------------------------------------------- 1. oracle and the single call


@gpu
@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 6, 7])
def test_against_oracle_and_single_calls(ctx, case, nq):
    device, layout = ctx
    singles = [ih.MasksEngine(device, case.qmasks[q]) for q in range(nq)]
    try:
        with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng:
            for parts in rf.PARTS:
                for offset in (0, 2):
                    for first, n in rf.RANGES:
                        with DeviceArrays(device, case.shares[parts][:, :nq, first:first + n], offset) as ptrs:
                            for nbins in rf.NBINS:
                                bins, invalid = eng.histogram(db, ptrs, nbins, first=first, n=n)
                                assert bins.shape == (nq, nbins) and invalid.shape == (nq,)
                                for q in range(nq):
                                    where = (parts, offset, first, n, nbins, q)
                                    assert same((bins[q], invalid[q]), case.want(parts, q, nbins, first, n)), where
                                    one = singles[q].histogram(db, slab_ptrs(ptrs, q, n), nbins, first=first, n=n)
                                    assert one[0].tobytes() == bins[q].tobytes() and one[1] == int(invalid[q]), where
                                    assert int(bins[q].sum()) + int(invalid[q]) == n
    finally:
        for s in singles:
            s.close()


# ---------------------------------------------------------------- 2. denominators given


@gpu
def test_resolver_histogram_over_the_engines_own_rows(ctx, case):
    """iris_resolver_histogram over the rows the masks engine writes is the fused form's histogram."""
    device, layout = ctx
    q = 2
    with case.db(device, layout) as db, ih.MasksEngine(device, case.qmasks[q]) as eng:
        rows = np.zeros((case.N, ROT), np.uint16)
        eng.batch_process(rows, db)
        assert (rows == case.den[q]).all()
        for parts in rf.PARTS:
            for offset in (0, 2):
                with DeviceArrays(device, list(case.shares[parts][:, q]) + [rows], offset) as ptrs:
                    for nbins in rf.NBINS:
                        for n in (case.N, 200, 1, 0):
                            plain = ih.resolver_histogram(device, ptrs[:-1], ptrs[-1], n, nbins)
                            assert same(plain, case.want(parts, q, nbins, 0, n)), (parts, offset, nbins, n)
                            fused = eng.histogram(db, ptrs[:-1], nbins, first=0, n=n)
                            assert fused[0].tobytes() == plain[0].tobytes() and fused[1] == plain[1]


@gpu
@pytest.mark.parametrize("offset", [0, 2], ids=["aligned", "offset2"])
def test_resolver_histogram_arbitrary_denominators(device, offset):
    """Denominators anywhere in u16 (above 12800, zeros among them) and uniform shares; rows 10..19
    decode to uneq above their denominators in every rotation, so their distances lie above 1 and
    fall in the last bin; rows of zeros are invalid; 1000 rows are four workgroups, the last one
    partial."""
    n = 1000
    rng = np.random.default_rng(11)
    den = rng.integers(0, 2**16, (n, ROT), dtype=np.uint16)
    den[::7, ::2] = 0
    den[5] = 0
    den[n - 1] = 0
    den[10:20] = rng.integers(12801, 25000, (10, ROT), dtype=np.uint16)
    for parts in rf.PARTS:
        shares = rng.integers(0, 2**16, (parts, n, ROT), dtype=np.uint16)
        shares[:, 10:20] = planted_shares(rng, den[10:20], rng.integers(26000, 32768, (10, ROT)), parts)
        e = resolver_expected(shares, den)
        assert (e.den > 12800).any() and (e.num[10:20] > e.den[10:20]).all() and (e.den == 0).sum() == 2
        assert (e.dist[10:20] > 1.0).all() and hf.expected(e.dist, 1024, 10, 10)[0][1023] == 10
        with DeviceArrays(device, list(shares) + [den], offset) as ptrs:
            for nbins in rf.NBINS:
                for m in (n, 257, 64, 1):
                    got = ih.resolver_histogram(device, ptrs[:-1], ptrs[-1], m, nbins)
                    assert same(got, hf.expected(e.dist, nbins, 0, m)), (parts, nbins, m)


# ---------------------------------------------------------------- 3. prefix sums and the match totals


@gpu
def test_prefix_sums_equal_the_match_totals(ctx, case):
    device, layout = ctx
    nbins = 64
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks) as eng, \
            ih.MasksEngine(device, case.qmasks[case.GARBAGE]) as single, DeviceArrays(device, case.shares[3]) as ptrs:
        bins, invalid = eng.histogram(db, ptrs, nbins)
        one, _ = single.histogram(db, slab_ptrs(ptrs, case.GARBAGE, case.N), nbins)
        prefix = np.concatenate([np.zeros((case.NQ, 1), np.uint64), np.cumsum(bins, axis=1, dtype=np.uint64)], axis=1)
        prefix1 = np.concatenate([[0], np.cumsum(one, dtype=np.uint64)])
        for j in list(range(nbins)) + [INF]:
            t, col = (INF, nbins) if j == INF else (j / nbins, j)
            _, counts = eng.matches(db, ptrs, t, cap=0)
            assert counts == [int(c) for c in prefix[:, col]], j
            _, c1 = single.matches(db, slab_ptrs(ptrs, case.GARBAGE, case.N), t, cap=0)
            assert c1 == int(prefix1[col]), j
        assert [int(c) for c in prefix[:, nbins]] == [case.N - int(i) for i in invalid]


# ---------------------------------------------------------------- 4. overwritten, untouched, identical


@gpu
def test_outputs_are_overwritten_and_identical(ctx, case):
    device, layout = ctx
    lib = ih.load_library()
    nq = 5
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
            ih.MasksEngine(device, case.qmasks[0]) as single, DeviceArrays(device, case.shares[3][:, :nq]) as ptrs, \
            DeviceArrays(device, [case.den[0]]) as dptr:
        arr = (ctypes.c_void_p * 3)(*ptrs)
        for nbins in rf.NBINS:
            calls = [
                (1, lambda b, i: lib.iris_resolver_histogram(device.handle, arr, 3, dptr[0], case.N, nbins, b, i)),
                (1, lambda b, i: lib.iris_resolver_histogram_masks(single.handle, db.handle, 0, case.N, arr, 3, nbins, b, i)),
                (nq, lambda b, i: lib.iris_resolver_batch_histogram_masks(eng.handle, db.handle, 0, case.N, arr, 3, nbins, b, i)),
            ]
            for rows, call in calls:
                raws = []
                for fill in (GUARD, 0, GUARD):
                    bins = np.full(rows * nbins + 8, fill, np.uint64)
                    invalid = np.full(rows + 2, fill, np.uint64)
                    assert call(bins.ctypes.data, invalid.ctypes.data) == 0
                    assert (bins[rows * nbins:] == np.uint64(fill)).all() and (invalid[rows:] == np.uint64(fill)).all()
                    raws.append(bins[:rows * nbins].tobytes() + invalid[:rows].tobytes())
                    for q in range(rows):
                        assert same((bins[q * nbins:(q + 1) * nbins], invalid[q]), case.want(3, q, nbins)), (rows, nbins, q)
                assert raws[0] == raws[1] == raws[2]
        # n == 0 writes zeros over the guard
        bins, invalid = np.full(nq * 64, GUARD, np.uint64), np.full(nq, GUARD, np.uint64)
        assert lib.iris_resolver_batch_histogram_masks(eng.handle, db.handle, 10, 0, arr, 3, 64, bins.ctypes.data,
                                                       invalid.ctypes.data) == 0
        assert not bins.any() and not invalid.any()


# ---------------------------------------------------------------- 5. the counter copies hook


@gpu
@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles", "lanes"])
def test_counter_copies_do_not_change_the_bytes(device, hooked_device, case, layout):
    def run(dev):
        out = []
        with case.db(dev, layout) as db, ih.MasksBatchEngine(dev, case.qmasks) as eng, \
                ih.MasksEngine(dev, case.qmasks[1]) as single, DeviceArrays(dev, case.shares[3]) as ptrs, \
                DeviceArrays(dev, [case.den[1]]) as dptr:
            for nbins in (64, 1024):
                b, i = eng.histogram(db, ptrs, nbins)
                out.append(b.tobytes() + i.tobytes())
                b, i = single.histogram(db, slab_ptrs(ptrs, 1, case.N), nbins)
                out.append(b.tobytes() + int(i).to_bytes(8, "little"))
                b, i = ih.resolver_histogram(dev, slab_ptrs(ptrs, 1, case.N), dptr[0], case.N, nbins)
                out.append(b.tobytes() + int(i).to_bytes(8, "little"))
        return out

    want = run(device)
    assert run(hooked_device(IRIS_HIST_COPIES=1)) == want
    assert run(hooked_device(IRIS_HIST_COPIES=4)) == want
    if layout == ih.LAYOUT_TILES:  # and through the batch kernel
        assert run(hooked_device(IRIS_HIST_COPIES=1, IRIS_TILES_PER_WAVE=4)) == want
        assert run(hooked_device(IRIS_HIST_COPIES=4, IRIS_TILES_PER_WAVE=1)) == want


# ---------------------------------------------------------------- 6. refusals with live handles


@gpu
def test_refusals_leave_the_device_usable(ctx, case):
    device, layout = ctx
    lib = ih.load_library()
    nq = 3
    bins, invalid = np.full(nq * 64, GUARD, np.uint64), np.full(nq, GUARD, np.uint64)
    b, i = bins.ctypes.data, invalid.ctypes.data
    enc = np.zeros((2, ih.BITS), np.uint16)
    with case.db(device, layout) as db, ih.MasksBatchEngine(device, case.qmasks[:nq]) as eng, \
            ih.MasksEngine(device, case.qmasks[0]) as single, ih.DistanceBatchEngine(device, enc) as dbe, \
            ih.TemplateEngine(device, oc.gen_templates(99, 0, 1)[0]) as te, \
            ih.Database(device, ih.KIND_TEMPLATES, 300, layout) as tdb, \
            DeviceArrays(device, case.shares[3][:, :nq]) as ptrs, DeviceArrays(device, [case.den[0]]) as dptr:
        tdb.generate(257, 8)
        arr = (ctypes.c_void_p * 3)(*ptrs)
        null_part = (ctypes.c_void_p * 3)(ptrs[0], None, ptrs[2])
        fb, fs, fp = lib.iris_resolver_batch_histogram_masks, lib.iris_resolver_histogram_masks, lib.iris_resolver_histogram
        refused = [
            (fb, (single.handle, db.handle, 0, 257, arr, 3, 64, b, i), E_ARG),  # a single-query masks engine
            (fb, (dbe.handle, db.handle, 0, 257, arr, 3, 64, b, i), E_ARG),  # a distance batch engine
            (fb, (te.handle, db.handle, 0, 257, arr, 3, 64, b, i), E_ARG),  # a template engine
            (fb, (eng.handle, tdb.handle, 0, 257, arr, 3, 64, b, i), E_ARG),  # a templates database
            (fb, (eng.handle, db.handle, 200, 100, arr, 3, 64, b, i), E_RANGE),
            (fb, (eng.handle, db.handle, 0, 257, arr, 9, 64, b, i), E_ARG),
            (fb, (eng.handle, db.handle, 0, 257, null_part, 3, 64, b, i), E_ARG),
            (fb, (eng.handle, db.handle, 0, 257, None, 3, 64, b, i), E_ARG),
            (fb, (eng.handle, db.handle, 0, 257, arr, 3, 48, b, i), E_ARG),
            (fb, (eng.handle, db.handle, 0, 257, arr, 3, 64, None, i), E_ARG),
            (fb, (eng.handle, db.handle, 0, 257, arr, 3, 64, b, None), E_ARG),
            (fs, (eng.handle, db.handle, 0, 257, arr, 3, 64, b, i), E_ARG),  # a batch engine in the single-query call
            (fs, (te.handle, db.handle, 0, 257, arr, 3, 64, b, i), E_ARG),
            (fs, (single.handle, tdb.handle, 0, 257, arr, 3, 64, b, i), E_ARG),
            (fs, (single.handle, db.handle, 257, 1, arr, 3, 64, b, i), E_RANGE),
            (fs, (single.handle, db.handle, 0, 257, null_part, 3, 2048, b, i), E_ARG),
            (fp, (device.handle, arr, 3, None, 257, 64, b, i), E_ARG),  # no denominators
            (fp, (device.handle, null_part, 3, dptr[0], 257, 64, b, i), E_ARG),
            (fp, (device.handle, arr, 0, dptr[0], 257, 64, b, i), E_ARG),
            (fp, (device.handle, arr, 3, dptr[0], 257, 0, b, i), E_ARG),
        ]
        for f, args, code in refused:
            assert f(*args) == code, args[2:7]
            assert lib.iris_last_error(), args[2:7]
        assert (bins == np.uint64(GUARD)).all() and (invalid == np.uint64(GUARD)).all()
        assert fs(eng.handle, db.handle, 0, 257, arr, 3, 64, b, i) == E_ARG
        assert b"iris_resolver_batch_histogram_masks" in lib.iris_last_error()
        # afterwards valid calls return the right answers
        got = eng.histogram(db, ptrs, 64)
        for q in range(nq):
            assert same((got[0][q], got[1][q]), case.want(3, q, 64)), q
        assert same(single.histogram(db, slab_ptrs(ptrs, 0, case.N), 64), case.want(3, 0, 64))
        assert same(ih.resolver_histogram(device, slab_ptrs(ptrs, 0, case.N), dptr[0], case.N, 64), case.want(3, 0, 64))


# ---------------------------------------------------------------- 7. large range


@pytest.fixture(scope="module")
def large():
    return rf.large_case()


def _profiled(device, f):
    device.reset_stats()
    device.set_profiling(True)
    try:
        res = f()
    finally:
        device.set_profiling(False)
    return res, device.kernel_stats("masks_batch_hist")[0], device.kernel_stats("masks_resolve_hist")[0]


@gpu
@pytest.mark.parametrize("tpw", [None, 1, 4], ids=["dispatch", "tpw1", "tpw4"])
def test_large_range(device, hooked_device, large, tpw):
    """Waves walk more than one tile group and the last tile is ragged.  Six queries: one 4-slot and
    one 2-slot launch; five: one 4-slot launch and a single-query left-over; sub-ranges that start
    and end inside tiles; the single-query form on a slab."""
    dev = device if tpw is None else hooked_device(IRIS_TILES_PER_WAVE=tpw)
    n, nbins = large.N, 1024
    with large.db(dev) as db:
        for nq, launches in ((6, (2, 0)), (5, (1, 1))):
            with ih.MasksBatchEngine(dev, large.qmasks[:nq]) as eng:
                for first, m in ((0, n), (37, n - 37 - 50)):
                    with DeviceArrays(dev, large.shares[:, :nq, first:first + m]) as ptrs:
                        (bins, invalid), batch, single = _profiled(dev, lambda: eng.histogram(db, ptrs, nbins, first=first, n=m))
                        assert (batch, single) == launches, (nq, first)
                        for q in range(nq):
                            assert same((bins[q], invalid[q]), large.want(q, nbins, first, m)), (nq, first, q)
                        if nq == 6 and first == 37:
                            for q in (1, large.GARBAGE):
                                with ih.MasksEngine(dev, large.qmasks[q]) as one:
                                    got = one.histogram(db, slab_ptrs(ptrs, q, m), nbins, first=first, n=m)
                                assert got[0].tobytes() == bins[q].tobytes() and got[1] == int(invalid[q]), q
        # the fixture: the zero-mask record is invalid, the garbage slab fills the last bin
        assert large.want(0, nbins)[1] == 1 and large.want(large.GARBAGE, nbins)[0][nbins - 1] > 1000


# ---------------------------------------------------------------- 8. three-party flow


@gpu
def test_three_party_flow(ctx):
    """257 planted templates shared among three parties, each party's rows from the oracle's
    DistanceEngine, summed and binned in the fused call: the histogram is iris_template_histogram's
    over the plaintext database."""
    device, layout = ctx
    c = hf.single_case()
    shares, masks = oc.prepare_shares(c.templates, bytes(range(32)))
    with ih.Database(device, ih.KIND_TEMPLATES, 300, layout) as tdb, ih.Database(device, ih.KIND_MASKS, 300, layout) as mdb:
        tdb.append(c.templates)
        mdb.append(masks)
        for key, query in c.queries.items():
            rows = [oc.distance_batch(oc.encode(query), shares[p]) for p in range(3)]
            with ih.TemplateEngine(device, query) as te, ih.MasksEngine(device, query[200:]) as me, \
                    DeviceArrays(device, rows) as ptrs:
                for nbins in rf.NBINS:
                    plain = te.histogram(tdb, nbins)
                    assert same(plain, hf.expected(c.dist[key], nbins)), (key, nbins)
                    got = me.histogram(mdb, ptrs, nbins)
                    assert got[0].tobytes() == plain[0].tobytes() and got[1] == plain[1] == 1, (key, nbins)


# ---------------------------------------------------------------- 9. the C++ program


@gpu
@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles-mfma", "lanes-valu"])
def test_cpp_resolver_histogram(layout, tmp_path):
    """iris_hip.hpp's three forms, run as their own process: every query's histogram from the batched
    call, the single-query call and resolver_histogram, against the oracle."""
    nq, n, seed, nbins = 5, 300, 41, 64
    exe = build_cpp_program(tmp_path)
    path = tmp_path / "hist.bin"
    r = subprocess.run([str(exe), str(path), str(nq), str(n), str(seed), str(layout), str(nbins)],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    raw = np.frombuffer(path.read_bytes(), np.uint64)
    assert raw.shape == (3 * nq * (nbins + 1),)
    raw = raw.reshape(3, nq, nbins + 1)
    i = np.arange(ih.LIMBS, dtype=np.uint64)
    with np.errstate(over="ignore"):
        qm = np.stack([((i + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15) * np.uint64(2 * j + 1)) ^ np.uint64(j << 7)
                       for j in range(nq)])
    el = np.arange(nq * n * ROT, dtype=np.uint64)
    shares = np.stack([(((el * 2654435761) & 0xFFFFFFFF) >> 7) + 12345 * p for p in range(2)]).astype(np.uint16)
    shares = shares.reshape(2, nq, n, ROT)
    masks = oc.gen_masks(seed, 0, n)
    for q in range(nq):
        e = resolver_expected(shares[:, q], oc.masks_batch(qm[q], masks))
        bins, invalid = hf.expected(e.dist, nbins)
        assert np.count_nonzero(bins) > 4, q
        for form in range(3):
            assert raw[form, q, :nbins].tobytes() == bins.tobytes() and raw[form, q, nbins] == invalid, (form, q)
