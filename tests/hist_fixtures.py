"""Shared by the histogram tests (test_histogram_abi.py, test_gpu_histogram.py,
test_gpu_template_batch_histogram.py): the two databases, their queries and the expected histograms,
all from the CPU oracle alone and computed once per process.

Expected histogram of a query over records [first, first + n): the oracle's f64 distances
(oc.template_distances: the best rotation's num / den, +inf without a valid rotation), binned by the
header's rule min(nbins - 1, floor(distance * nbins)); +inf is counted as invalid and in no bin."""
import functools

import numpy as np

from oracle import oracle_c as oc

ROT = 31
NBINS = [1, 2, 64, 1024]
RANGES = [(0, 257), (5, 200), (33, 1), (256, 1), (0, 0)]
SMALL_N = 257                # 9 tiles, the last holding one record
LARGE_N = 4098 * 32 + 27     # past the K-split form's 1024 tiles; a ragged last tile
ONES = ~np.uint64(0)


def bin_of(dist, nbins):
    """The header's f64 rule on finite distances."""
    return np.minimum(nbins - 1, np.floor(np.asarray(dist, np.float64) * nbins)).astype(np.int64)


def expected(dist, nbins, first=0, n=None):
    """(bins [nbins] uint64, invalid) of the records [first, first + n) of a distance array."""
    n = len(dist) - first if n is None else n
    d = dist[first:first + n]
    finite = np.isfinite(d)
    bins = np.bincount(bin_of(d[finite], nbins), minlength=nbins).astype(np.uint64)
    return bins, int((~finite).sum())


def best_rotation(query, templates):
    """Per record the best rotation's (num, den) in the exact fraction order, lowest rotation on
    ties (den = 0: none), from the oracle's integer counts."""
    num, den = (np.asarray(a, np.int64) for a in oc.template_counts(query, templates))
    bn, bd = np.zeros(len(num), np.int64), np.zeros(len(num), np.int64)
    for k in range(ROT):
        better = (den[:, k] != 0) & ((bd == 0) | (num[:, k] * bd < bn * den[:, k]))
        bn[better], bd[better] = num[better, k], den[better, k]
    return bn, bd


def with_pattern_bits(count):
    """A record with all-ones masks whose pattern has its `count` lowest bits set."""
    rec = np.zeros(400, np.uint64)
    rec[200:] = ONES
    rec[:count // 64] = ONES
    if count % 64:
        rec[count // 64] = np.uint64((1 << (count % 64)) - 1)
    return rec


class SingleCase:
    """257 generated records (seed 8) with the plants of the issue.  EDGE_QUERY has an all-zero
    pattern under an all-ones mask: it is its own rotation, so against a record with an all-ones
    mask every rotation gives num = popcount(pattern), den = 12800 -- distances known exactly.
    GEN_QUERY is a generated template (seed 99), whose rotations differ."""

    PLANTS = {0: 0, 31: 3200, 32: 3199, 256: 12800}  # record -> pattern bits set (den = 12800)
    ZERO_MASK = 100

    def __init__(self):
        self.edge_query = with_pattern_bits(0)
        self.gen_query = oc.gen_templates(99, 0, 1)[0].copy()
        self.templates = oc.gen_templates(8, 0, SMALL_N).copy()
        self.planted = {i: with_pattern_bits(c) for i, c in self.PLANTS.items()}
        zero = self.templates[self.ZERO_MASK].copy()
        zero[200:] = 0
        self.planted[self.ZERO_MASK] = zero
        for i, rec in self.planted.items():
            self.templates[i] = rec
        self.queries = {"edge": self.edge_query, "gen": self.gen_query}
        self.dist = {k: oc.template_distances(q, self.templates) for k, q in self.queries.items()}

    def fill(self, db):
        db.generate(SMALL_N, 8)
        for i, rec in self.planted.items():
            db.write(i, rec[None, :])


class LargeCase:
    """4098 * 32 + 27 generated records (seed 77) with a few plants at tile edges and in the ragged
    tail; queries generated with seed 99, queries 3 and 10 with zero masks."""

    NQ = 17
    ZERO_MASK = (3, 10)
    SPOTS = [0, 127, 128, 4095 * 32, LARGE_N - 1]

    def __init__(self):
        self.queries = batch_queries()
        self.templates = oc.gen_templates(77, 0, LARGE_N).copy()
        self.planted = {}
        for j, s in enumerate(self.SPOTS):
            self.planted[s] = planted(self.queries[(0, 1, 5, 16, 2)[j]], (-15, 0, 15, 7, -3)[j], 9 + j)
        for s, rec in self.planted.items():
            self.templates[s] = rec

    @functools.lru_cache(maxsize=None)
    def dist(self, q):
        return oc.template_distances(self.queries[q], self.templates)

    def fill(self, db):
        db.generate(LARGE_N, 77)
        for s, rec in self.planted.items():
            db.write(s, rec[None, :])


def planted(q, rotation, flip_limb=9, flips=0x0F0F00000F0F):
    """The query rotated, a few pattern bits flipped."""
    rec = np.concatenate([oc.bits_rotated(q[:200], rotation), oc.bits_rotated(q[200:], rotation)])
    rec[flip_limb] ^= np.uint64(flips)
    return rec


@functools.lru_cache(maxsize=None)
def batch_queries():
    q = oc.gen_templates(99, 0, LargeCase.NQ).copy()
    for z in LargeCase.ZERO_MASK:
        q[z, 200:] = 0
    q.setflags(write=False)
    return q


class SmallBatchCase:
    """The 257 generated records (seed 8) against the batch queries: near-copies of chosen queries at
    tile edges and in the ragged tail (as SmallCase of test_gpu_template_batch_matches.py), and a
    zero-mask record that is invalid for every query."""

    ZERO_MASK_RECORD = 100

    def __init__(self):
        q = self.queries = batch_queries()
        t = self.templates = oc.gen_templates(8, 0, SMALL_N).copy()
        t[0] = planted(q[1], -15)
        t[31] = planted(q[5], 0, 11)
        t[32] = planted(q[5], 15, 12, 0xFFFFFFFFFF)
        t[256] = planted(q[5], -15, 13, 0xF)
        t[130] = planted(q[6], 0)
        t[200] = t[130]
        t[64] = planted(q[8], 15)
        t[224] = planted(q[16], -15)
        t[255] = planted(q[16], 0, 20)
        t[self.ZERO_MASK_RECORD, 200:] = 0
        self.dist = [oc.template_distances(qq, t) for qq in q]

    def fill(self, db):
        db.append(self.templates)


@functools.lru_cache(maxsize=None)
def single_case():
    return SingleCase()


@functools.lru_cache(maxsize=None)
def large_case():
    return LargeCase()


@functools.lru_cache(maxsize=None)
def small_batch_case():
    return SmallBatchCase()
