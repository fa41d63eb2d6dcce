"""Shared by the resolver histogram tests (test_resolver_histogram_abi.py,
test_gpu_resolver_histogram.py): the masks, query masks and share slabs of the small and the large
case and their expected histograms, all from the CPU oracle alone and computed once per process.

Expected histogram of a slab: oc.masks_batch gives the denominators, resolver_expected
(test_gpu_matches.py) the decoded best rotation and its f64 distance -- tied there to
oc.resolver_combine -- and hist_fixtures.expected bins the distances by the header's rule.

The share slabs are built as those of test_gpu_masks_batch_matches.py: for every (query, record,
rotation) a target uneq is chosen, all parts but the last are uniform random and the last is
den - 2 uneq - the others (mod 2^16), which decode_distance (src/lib.rs:97-107) turns back into
uneq / den."""
import functools

import numpy as np

import hist_fixtures as hf
import iris_hip as ih
from oracle import oracle_c as oc
from test_gpu_masks_batch_matches import background, planted_shares
from test_gpu_matches import resolver_expected

ROT = 31
NBINS = hf.NBINS
RANGES = hf.RANGES
PARTS = (1, 3, 8)


def quarter_rotation(den_row):
    """The lowest rotation of a record whose denominator is a multiple of 4 (and at least 2048, so
    one count is less than a bin of 1024)."""
    ks = [k for k in range(ROT) if den_row[k] % 4 == 0 and den_row[k] >= 2048]
    assert ks, den_row
    return ks[0]


class SmallCase:
    """257 masks (9 tiles, the last holding one record; record ZERO written as zero), 7 query masks.
    Background uneq in [0.4 den, 0.6 den); in every slab record 0 holds the exact fraction 0, records
    31 and 256 exactly 1/4 and record 32 one count less than 1/4 -- the tile edges and the ragged
    tail.  Slab GARBAGE has uniform random shares in its last part: uneq > den occurs.  The same uneq
    is shared out among 1, 3 and 8 parts (shares[parts]: [parts, 7, 257, 31])."""

    N, NQ, ZERO, GARBAGE = 257, 7, 77, 6
    PLANTS = {0: "zero", 31: "quarter", 32: "below", 256: "quarter"}

    def __init__(self):
        rng = np.random.default_rng(2025)
        self.masks = oc.gen_masks(8, 0, self.N).copy()
        self.masks[self.ZERO] = 0
        self.qmasks = rng.integers(0, 2**64, (self.NQ, ih.LIMBS), dtype=np.uint64)
        self.den = np.stack([oc.masks_batch(q, self.masks) for q in self.qmasks])
        d = self.den.astype(np.int64)
        uneq = background(rng, self.den, 0.4, 0.6)
        self.plant_rot = np.zeros((self.NQ, self.N), np.int64)
        for q in range(self.NQ):
            for rec, what in self.PLANTS.items():
                k = quarter_rotation(d[q, rec])
                self.plant_rot[q, rec] = k
                uneq[q, rec, k] = {"zero": 0, "quarter": d[q, rec, k] // 4, "below": d[q, rec, k] // 4 - 1}[what]
        self.shares, self.exp = {}, {}
        for parts in PARTS:
            s = planted_shares(rng, self.den, uneq, parts)
            s[parts - 1, self.GARBAGE] = rng.integers(0, 2**16, (self.N, ROT), dtype=np.uint16)
            self.shares[parts] = s
            self.exp[parts] = [resolver_expected(s[:, q], self.den[q]) for q in range(self.NQ)]

    def db(self, dev, layout):
        db = ih.Database(dev, ih.KIND_MASKS, 300, layout)
        db.generate(self.N, 8)
        db.write(self.ZERO, self.masks[self.ZERO][None, :])
        return db

    def want(self, parts, q, nbins, first=0, n=None):
        return hf.expected(self.exp[parts][q].dist, nbins, first, n)


class LargeCase:
    """6 query masks over 4098 * 32 + 27 generated masks: the batch kernel's waves walk more than one
    tile group and the last tile is ragged.  Record ZERO (in the second tile group of a wave at four
    tiles per wave) is written as zero; background uneq in [0.05 den, 0.95 den); slab 5 has uniform
    random shares in its last part."""

    N, NQ, SEED, PARTS = hf.LARGE_N, 6, 21, 3
    ZERO = 4096 * 32 + 5
    GARBAGE = 5

    def __init__(self):
        rng = np.random.default_rng(7)
        self.masks = oc.gen_masks(self.SEED, 0, self.N).copy()
        self.masks[self.ZERO] = 0
        self.qmasks = rng.integers(0, 2**64, (self.NQ, ih.LIMBS), dtype=np.uint64)
        self.den = np.stack([oc.masks_batch(q, self.masks) for q in self.qmasks])
        uneq = background(rng, self.den, 0.05, 0.95)
        self.shares = planted_shares(rng, self.den, uneq, self.PARTS)  # [3, 6, N, 31]
        self.shares[self.PARTS - 1, self.GARBAGE] = rng.integers(0, 2**16, (self.N, ROT), dtype=np.uint16)
        self.exp = [resolver_expected(self.shares[:, q], self.den[q]) for q in range(self.NQ)]

    def db(self, dev):
        db = ih.Database(dev, ih.KIND_MASKS, self.N, ih.LAYOUT_TILES)
        db.generate(self.N, self.SEED)
        db.write(self.ZERO, self.masks[self.ZERO][None, :])
        return db

    def want(self, q, nbins, first=0, n=None):
        return hf.expected(self.exp[q].dist, nbins, first, n)


@functools.lru_cache(maxsize=None)
def small_case():
    return SmallCase()


@functools.lru_cache(maxsize=None)
def large_case():
    return LargeCase()
