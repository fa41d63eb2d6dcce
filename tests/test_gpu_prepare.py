"""Share preparation on the device (the reference's
`prepare`, src/main.rs:333-361, EncodedBits::share src/encoded_bits.rs:23-38):
bit-exact against the oracle's restatement of the ChaCha (8/12/20-round) counter-mode
derivation, and the prepared shares drive the MPC flow to the plaintext answer."""
import functools

import numpy as np
import pytest

import iris_hip as ih
from oracle import oracle_c as oc

pytestmark = pytest.mark.gpu
ROT = 31
KEY = bytes(range(7, 39))


@pytest.mark.parametrize("layout", [ih.LAYOUT_TILES, ih.LAYOUT_LANES], ids=["tiles", "lanes"])
@pytest.mark.parametrize("parties,rounds", [(1, 12), (2, 12), (3, 12), (3, 20), (2, 8)])
def test_prepare_matches_oracle(device, layout, parties, rounds):
    n = 70
    t = oc.gen_templates(31, 0, n)
    want_s, want_m = oc.prepare_shares(t[5:5 + 60], KEY, nonce=11, parties=parties, index_base=1000 + 5,
                                       rounds=rounds)
    with ih.Database(device, ih.KIND_TEMPLATES, n, layout) as tdb:
        tdb.append(t)
        sdbs = [ih.Database(device, ih.KIND_SHARES, 64, layout) for _ in range(parties)]
        with ih.Database(device, ih.KIND_MASKS, 64, layout) as mdb:
            mdb.append(t[:1, 200:])  # appends after existing records
            ih.prepare_shares(tdb, sdbs, mdb, key=KEY, nonce=11, first=5, n=60, index_base=1000, rounds=rounds)
            assert len(mdb) == 61 and (mdb.read(1, 60) == want_m).all()
        for j, db in enumerate(sdbs):
            assert len(db) == 60
            assert (db.read(0, 60) == want_s[j]).all()
            db.close()


T, L = ih.LAYOUT_TILES, ih.LAYOUT_LANES
ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


@functools.lru_cache(maxsize=None)
def _templates(n):
    """n oracle templates (read-only, shared) with three hand-made records: 40 = pattern all ones
    under an empty mask, 64 = pattern and mask all ones, n-33 = pattern zero under a full mask."""
    t = oc.gen_templates(31, 0, n)
    if n > 64:
        t[40, :200], t[40, 200:] = ONES, 0
        t[64] = ONES
        t[n - 33, :200], t[n - 33, 200:] = 0, ONES
    t.setflags(write=False)
    return t


@functools.lru_cache(maxsize=8)
def _want(total, first, n, parties, g0, nonce, rounds):
    """The oracle's shares and masks of _templates(total)[first:first+n] at global index g0."""
    s, m = oc.prepare_shares(_templates(total)[first:first + n], KEY, nonce=nonce, parties=parties, index_base=g0,
                             rounds=rounds)
    s.setflags(write=False)
    m.setflags(write=False)
    return s, m


def _path_launches(tl, sls, ml):
    """(unpack, prepare, pack) launches of one single-chunk iris_prepare_shares call, read off
    its dispatch: all TILES is one in-place launch; anything else stages the templates (one
    unpack); share lists with a LANES database are written to staging and packed into every
    share database, TILES ones too; a masks database on a staged call is one more pack."""
    if tl == T and all(s == T for s in sls) and ml in (None, T):
        return {"unpack": 0, "prepare": 1, "pack": 0}
    packs = 0 if all(s == T for s in sls) else len(sls)
    return {"unpack": 1, "prepare": 1, "pack": packs + (ml is not None)}


def _prepare_and_check(device, tl, sls, ml, *, total, first, n, index_base, nonce, rounds=12, prefill=None,
                       chunks=None):
    """One iris_prepare_shares call into pre-filled databases of the given layouts: lengths,
    every new record against the oracle, the older records untouched, and the kernel launches
    that tell which path ran (`chunks` staging chunks; None: a single one)."""
    parties = len(sls)
    t = _templates(total)
    # the 64-party reference is 221 MB: computed for its one test, not kept
    want_s, want_m = (_want if parties <= 8 else _want.__wrapped__)(total, first, n, parties, index_base + first,
                                                                    nonce, rounds)
    pre = [prefill(j) if prefill else 5 + 9 * j for j in range(parties)]
    old = [oc.gen_shares(70 + j, 0, pre[j]) for j in range(parties)]
    old_m = oc.gen_masks(80, 0, 33)
    dbs = []
    try:
        tdb = ih.Database(device, ih.KIND_TEMPLATES, total, tl)
        dbs.append(tdb)
        tdb.append(t)
        sdbs = []
        for j in range(parties):
            sdbs.append(ih.Database(device, ih.KIND_SHARES, pre[j] + n + 7, sls[j]))
            dbs.append(sdbs[j])
            if pre[j]:
                sdbs[j].append(old[j])
        mdb = None
        if ml is not None:
            mdb = ih.Database(device, ih.KIND_MASKS, 33 + n + 7, ml)
            dbs.append(mdb)
            mdb.append(old_m)
        device.reset_stats()
        device.set_profiling(True)
        try:
            ih.prepare_shares(tdb, sdbs, mdb, key=KEY, nonce=nonce, first=first, n=n, index_base=index_base,
                              rounds=rounds)
            launches = {k: device.kernel_stats(k)[0] for k in ("unpack", "prepare", "pack")}
        finally:
            device.set_profiling(False)
        expect = _path_launches(tl, sls, ml)
        if chunks is not None:
            assert expect["unpack"] == 1
            expect = {k: v * chunks for k, v in expect.items()}
        assert launches == expect
        for j, db in enumerate(sdbs):
            assert len(db) == pre[j] + n
            assert (db.read(pre[j], n) == want_s[j]).all(), f"share {j}"
            if pre[j]:
                assert (db.read(0, pre[j]) == old[j]).all(), f"share {j}: older records changed"
        if mdb is not None:
            assert len(mdb) == 33 + n
            assert (mdb.read(33, n) == want_m).all()
            assert (mdb.read(0, 33) == old_m).all()
        return want_s
    finally:
        for db in dbs:
            db.close()


LAYOUT_MATRIX = [  # templates, shares, masks (None: no masks database), rounds
    (T, (T, T, T), T, 12),     # direct kernel (control)
    (T, (T, T, T), None, 12),  # direct kernel (control)
    (L, (T, T, T), T, 12),     # tiles kernel
    (L, (T, T, T), T, 8),
    (L, (T, T, T), T, 20),
    (L, (T, T, T), None, 12),
    (T, (T, T, T), L, 12),
    (L, (T, T), L, 12),
    (T, (L, L, L), T, 12),     # staging kernel, templates unpacked from TILES
    (L, (T, L, T), L, 12),     # staging kernel, mixed packs
    (T, (L, T), None, 12),
]


def _row_id(row):
    name = {T: "T", L: "L", None: "none"}
    return f"{name[row[0]]}-{''.join(name[s] for s in row[1])}-{name[row[2]]}-r{row[3]}"


@pytest.mark.parametrize("row", LAYOUT_MATRIX, ids=_row_id)
def test_prepare_layout_matrix(device, row):
    """Every dispatch of iris_prepare_shares (prepare_direct_kernel, prepare_shares_tiles_kernel,
    prepare_shares_kernel + packs) gives the oracle's records whatever the layouts: 131 records
    from record 37 of 200 cross the TILES tile edges at 64..160 and fill two 64-lane workgroups
    and 3 lanes of a third; the share databases already hold 5, 14, 23 records and the masks
    database 33, so every destination starts inside a tile, at a different place per party."""
    tl, sls, ml, rounds = row
    _prepare_and_check(device, tl, sls, ml, total=200, first=37, n=131, index_base=1000, nonce=11, rounds=rounds)


def test_prepare_pack_chunk_seam_64_parties(device):
    """64 parties into LANES databases: 128 records fill a staging chunk, so 135 records are a
    chunk of 128 and one of 7, with index_base above 2^33 and a nonce with a high word."""
    chunk = staging_chunk(64, False)
    assert chunk == 128
    _prepare_and_check(device, L, (L,) * 64, L, total=140, first=3, n=135, index_base=2**33 + 5,
                       nonce=0xDEADBEEF12345678, prefill=lambda j: j % 5, chunks=-(-135 // chunk))


KERNEL_ROWS = [(T, T, T), (L, T, L), (L, L, L)]  # direct, tiles and staging kernel
KERNEL_IDS = ["direct", "tiles", "staging"]


@pytest.mark.parametrize("tl,sl,ml", KERNEL_ROWS, ids=KERNEL_IDS)
def test_prepare_counter_crosses_2_32(device, tl, sl, ml):
    """3 parties from global index 2^32 // 800 - 30: block counter (g * 2 + j) * 400 + b passes
    2^32 inside the range, so state word 13 goes from 0 to 1."""
    g0, n = 2**32 // 800 - 30, 60
    assert g0 * 2 * 400 < 2**32 < ((g0 + n - 1) * 2 + 1) * 400 + 399
    _prepare_and_check(device, tl, (sl,) * 3, ml, total=70, first=5, n=n, index_base=g0 - 5, nonce=11)


@pytest.mark.parametrize("tl,sl,ml", KERNEL_ROWS, ids=KERNEL_IDS)
@pytest.mark.parametrize("parties", [5, 1])
def test_prepare_large_index_and_nonce(device, tl, sl, ml, parties):
    """index_base 2^40 + 3 (g * (parties-1) needs 64 bits) and a nonce with a high word.  A single
    party draws no keystream: its share is encode() itself."""
    want = _prepare_and_check(device, tl, (sl,) * parties, ml, total=70, first=5, n=60, index_base=2**40 + 3,
                              nonce=0xDEADBEEF12345678)
    if parties == 1:
        assert (want[0] == np.stack([oc.encode(x) for x in _templates(70)[5:65]])).all()


def staging_chunk(parties, shares_in_place):
    """Records per staging chunk of iris_prepare_shares when it is not one in-place launch:
    256 MiB over the staged bytes per record (template 3200 + mask 1600, plus 25 600 per
    share unless every share database is TILES and written in place), in whole 64s."""
    per = 4800 + (0 if shares_in_place else parties * 25600)
    return max(64, (256 << 20) // per // 64 * 64)


@pytest.mark.parametrize("tlayout,mlayout", [(ih.LAYOUT_TILES, None), (ih.LAYOUT_LANES, ih.LAYOUT_LANES)],
                         ids=["all-tiles", "lanes-templates"])
def test_prepare_multi_chunk_sampled(device, tlayout, mlayout):
    """60 000 templates x 3 parties into TILES share databases.  all-tiles: TILES templates, one
    in-place launch with no staging (the control).  lanes-templates: LANES templates and a LANES
    masks database go through the staging loop and prepare_shares_tiles_kernel in two chunks
    (55 872 + 4 128 records), counted by the unpack launches.  Records 0, 1, n-1 and the 64
    around record 55 872 are checked against the oracle at their own global index, and every
    record via the share-sum identity against the oracle's template counts."""
    n, parties = 60_000, 3
    chunk = staging_chunk(parties, True)
    assert chunk == 55_872
    t = oc.gen_templates(99, 0, n)
    with ih.Database(device, ih.KIND_TEMPLATES, n, tlayout) as tdb:
        tdb.generate(n, 99)
        sdbs = [ih.Database(device, ih.KIND_SHARES, n) for _ in range(parties)]
        mdb = ih.Database(device, ih.KIND_MASKS, n, mlayout) if mlayout is not None else None
        device.reset_stats()
        device.set_profiling(True)
        try:
            key = ih.prepare_shares(tdb, sdbs, mdb)  # random key from os.urandom
            launches = {k: device.kernel_stats(k)[0] for k in ("unpack", "prepare", "pack")}
        finally:
            device.set_profiling(False)
        assert len(key) == 32
        if mlayout is None:
            assert launches == {"unpack": 0, "prepare": 1, "pack": 0}
        else:
            chunks = -(-n // chunk)
            assert chunks == 2
            assert launches == {"unpack": chunks, "prepare": chunks, "pack": chunks}  # pack: the masks
        for a, b in ((0, 2), (chunk - 32, chunk + 32), (n - 1, n)):
            assert (tdb.read(a, b - a) == t[a:b]).all()
            want, want_m = oc.prepare_shares(t[a:b], key, parties=parties, index_base=a)
            for j in range(parties):
                assert len(sdbs[j]) == n
                assert (sdbs[j].read(a, b - a) == want[j]).all()
            if mdb is not None:
                assert len(mdb) == n
                assert (mdb.read(a, b - a) == want_m).all()
        if mdb is not None:  # the masks are small enough to compare whole
            assert (mdb.read(0, n) == t[:, 200:]).all()
        # sum identity on everything, via the dot engine: sum_j <q, s_j> == <q, encode(t)> per rotation
        q = ih.encode(ih.Template.from_array(t[17]))
        acc = np.zeros((n, ROT), np.uint32)
        with ih.DistanceEngine(device, q) as eng:
            for db in sdbs:
                out = np.empty((n, ROT), np.uint16)
                eng.batch_process(out, db)
                acc += out
            enc = np.stack([oc.encode(x) for x in t[:64]])
            with ih.Database(device, ih.KIND_SHARES, 64) as edb:
                edb.append(enc)
                direct = np.empty((64, ROT), np.uint16)
                eng.batch_process(direct, edb)
        assert ((acc[:64] % 65536) == direct).all()
        # <q, encode(t)> = |mq & mt| - 2 |(pq ^ pt) & mq & mt| per rotation, from the oracle's counts
        num, den = oc.template_counts(t[17], t)
        assert ((acc % 65536) == (den.astype(np.int64) - 2 * num.astype(np.int64)) % 65536).all()
        for db in sdbs + ([mdb] if mdb is not None else []):
            db.close()


def test_mpc_with_device_prepared_shares(device):
    n = 1500
    templates = oc.gen_templates(55, 0, n)
    q = templates[999].copy()
    q[:200] ^= np.uint64(0x10)
    with ih.Database(device, ih.KIND_TEMPLATES, n) as tdb, ih.TemplateEngine(device, q) as te:
        tdb.append(templates)
        sdbs = [ih.Database(device, ih.KIND_SHARES, n) for _ in range(3)]
        mdb = ih.Database(device, ih.KIND_MASKS, n)
        ih.prepare_shares(tdb, sdbs, mdb)
        enc_q = ih.encode(ih.Template.from_array(q))
        outs = []
        for db in sdbs:
            with ih.DistanceEngine(device, enc_q) as eng:
                out = np.empty((n, ROT), np.uint16)
                eng.batch_process(out, db)
                outs.append(out)
        with ih.MasksEngine(device, q[200:]) as me:
            den = np.empty((n, ROT), np.uint16)
            me.batch_process(den, mdb)
        m = ih.resolver_search(outs, den, device=device)
        ref = te.search(tdb)
        for db in sdbs + [mdb]:
            db.close()
    best, idx = oc.argmin(oc.template_distances(q, templates))
    assert m.index == ref.index == idx == 999
    assert np.float64(m.distance).view(np.uint64) == np.float64(best).view(np.uint64)


def test_prepare_argument_errors(device):
    with ih.Database(device, ih.KIND_TEMPLATES, 10) as tdb, ih.Database(device, ih.KIND_SHARES, 10) as s, \
            ih.Database(device, ih.KIND_MASKS, 10) as m:
        tdb.generate(10, 1)
        with pytest.raises(ih.IrisError):
            ih.prepare_shares(tdb, [s, s])         # the same database twice
        with pytest.raises(ih.IrisError):
            ih.prepare_shares(tdb, [m])            # wrong kind
        with pytest.raises(ih.IrisError):
            ih.prepare_shares(tdb, [s], first=5, n=10)  # outside the template range
        with pytest.raises(ih.IrisError):
            ih.prepare_shares(tdb, [s], rounds=10)      # not ChaCha8/12/20
        assert len(s) == 0
        many = [ih.Database(device, ih.KIND_SHARES, 4) for _ in range(65)]
        try:
            with pytest.raises(ih.IrisError):
                ih.prepare_shares(tdb, many, m, n=3)    # more than 64 parties
            assert [len(db) for db in many] == [0] * 65 and len(m) == 0
            # 64 parties are accepted
            t = oc.gen_templates(1, 0, 10)
            want_s, want_m = oc.prepare_shares(t[2:5], KEY, nonce=11, parties=64, index_base=1000 + 2)
            ih.prepare_shares(tdb, many[:64], m, key=KEY, nonce=11, first=2, n=3, index_base=1000)
            assert len(m) == 3 and (m.read(0, 3) == want_m).all()
            for j, db in enumerate(many[:64]):
                assert len(db) == 3 and (db.read(0, 3) == want_s[j]).all()
            assert len(many[64]) == 0
            # a share database with room for fewer than n more records: nothing changes
            # (capacities are rounded up to whole tiles, so fill one to its real capacity less 1)
            full = many[64]
            old = oc.gen_shares(3, 0, full.capacity - 1)
            full.append(old)
            with pytest.raises(ih.IrisError):
                ih.prepare_shares(tdb, [s, many[0], full], m, n=2)
            assert len(s) == 0 and len(m) == 3 and len(many[0]) == 3 and len(full) == len(old)
            assert (m.read(0, 3) == want_m).all() and (many[0].read(0, 3) == want_s[0]).all()
            assert (full.read(0, len(old)) == old).all()
            ih.prepare_shares(tdb, [s, many[0], full], m, n=1)  # exactly fills it
            assert len(full) == full.capacity and (full.read(0, len(old)) == old).all()
        finally:
            for db in many:
                db.close()
