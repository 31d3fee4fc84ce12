"""Repeat families (mimeo_link_regions, kernel K12; engine.link_regions; `mimeo self --families`) against a plain Python / numpy
restatement of "family linking v1" (include/mimeo_hip.h), written here from the rule alone: per alignment a map from every
target base of [tstart, tend) to its query coordinate (-1 under a deletion), the projection of a window as the min and max of
the map over it, a dict as the union-find, the family as the min of the component.  Equality is exact, for family and links."""
import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi
from mimeo_amd.synth import _ACGT, _COMP, _mutate, make_families, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


# ---- the restatement -------------------------------------------------------------------------------------------------------

def restate(L, chrom_of_scaf, recs, first, blocks, regions, items, pct):
    """(family, links) of the rule.  L: scaffold lengths; chrom_of_scaf: None = identity; regions: rows of (chrom, start, end);
    items: rows of (aln, region, w0, w1)."""
    nreg = len(regions)
    chrom = list(range(len(L))) if chrom_of_scaf is None else [int(c) for c in chrom_of_scaf]
    rc, rs, re_ = (np.array([int(r[k]) for r in regions], dtype=np.int64) for k in range(3))
    by_chrom = {c: np.flatnonzero(rc == c) for c in set(rc.tolist())}
    maps, cache = {}, {}

    def base_map(a):
        if a not in maps:
            b = blocks[int(first[a]):int(first[a + 1])]
            if len(b) == 0:
                maps[a] = (0, np.zeros(0, dtype=np.int64))
            else:
                t0, t1 = int(b['t'][0]), int(b['t'][-1]) + int(b['len'][-1])
                m = np.full(t1 - t0, -1, dtype=np.int64)
                for t, q, ln in b.tolist():
                    m[t - t0:t - t0 + ln] = np.arange(q, q + ln)
                maps[a] = (t0, m)
        return maps[a]

    def linked(a, r, w0, w1):
        if 100 * (w1 - w0) < pct * int(re_[r] - rs[r]):   # A
            return []
        t0, m = base_map(a)                                # B
        seg = m[max(w0 - t0, 0):max(w1 - t0, 0)]
        cols = seg[seg >= 0]
        if cols.size == 0:
            return []
        q_lo, q_hi = int(cols.min()), int(cols.max()) + 1
        qid, Lq = int(recs[a]['qid']), L[int(recs[a]['qid'])]
        p0, p1 = (Lq - q_hi, Lq - q_lo) if int(recs[a]['qstrand']) else (q_lo, q_hi)
        idx = by_chrom.get(chrom[qid], np.zeros(0, dtype=np.int64))   # C
        ov = np.minimum(re_[idx], p1) - np.maximum(rs[idx], p0)
        return idx[(ov > 0) & (100 * ov >= pct * (re_[idx] - rs[idx])) & (idx != r)].tolist()

    parent = {i: i for i in range(nreg)}

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    links = np.zeros(nreg, dtype=np.uint64)
    for it in np.asarray(items, dtype=np.int64).reshape(-1, 4).tolist():
        key = tuple(it)
        if key not in cache:   # what an item links depends on the item alone
            cache[key] = linked(*key)
        for s in cache[key]:
            parent[find(it[1])] = find(s)
            links[it[1]] += np.uint64(1)
    smallest = {}
    for i in range(nreg):   # ascending: the first member seen of a component is its smallest
        smallest.setdefault(find(i), i)
    return np.array([smallest[find(i)] for i in range(nreg)], dtype=np.uint32), links


def make_paths(L, paths):
    """paths: (tid, qid, qstrand, [(t, q, len), ...]) -> records, first, blocks; the contract of mimeo_path_block is asserted
    here so that a slip in a table is not taken for the kernel's"""
    recs = np.zeros(len(paths), dtype=_ffi.ALIGNMENT)
    first, blocks = [0], []
    for i, (tid, qid, strand, blk) in enumerate(paths):
        t_end = q_end = 0
        for t, q, ln in blk:
            assert ln >= 1 and t >= t_end and q >= q_end and t + ln <= L[tid] and q + ln <= L[qid], (i, t, q, ln)
            t_end, q_end = t + ln, q + ln
        recs[i]['tid'], recs[i]['qid'], recs[i]['qstrand'] = tid, qid, strand
        blocks.extend(blk)
        first.append(len(blocks))
    return recs, np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK).reshape(-1)


def regions_of(rows):
    r = np.zeros(len(rows), dtype=_ffi.INTERVAL)
    for i, row in enumerate(rows):
        r[i] = tuple(row)
    return r


class Small:
    """three scaffolds of a few kbp on the device; the sequences do not matter to K12"""
    L = [5000, 4000, 3000]
    names = ['s0', 's1', 's2']

    def __init__(self, eng):
        rng = np.random.default_rng(70)
        self.eng = eng
        self.G = eng.Genome(self.names, [_ACGT[rng.integers(0, 4, n)] for n in self.L])

    def check(self, paths, regions, items, pct=80, chrom=None):
        """one call against the restatement: (family, links) as lists"""
        recs, first, blocks = make_paths(self.L, paths)
        reg = regions_of(regions)
        fam, lnk = self.eng.link_regions(self.G, recs, first, blocks, reg, chrom, np.array(items, dtype=np.uint32).reshape(-1, 4), pct)
        efam, elnk = restate(self.L, chrom, recs, first, blocks, regions, items, pct)
        assert fam.dtype == np.uint32 and lnk.dtype == np.uint64 and fam.shape == lnk.shape == (len(regions),)
        assert fam.tolist() == efam.tolist() and lnk.tolist() == elnk.tolist(), (fam.tolist(), efam.tolist(), lnk.tolist(), elnk.tolist())
        assert (fam <= np.arange(len(regions))).all()
        return fam.tolist(), lnk.tolist()

    def projects_to(self, path, tregion, P, pct=100):
        """The region `tregion` of scaffold 0, as a whole window, projects through `path` (onto scaffold 1) to exactly P: at
        100 per cent the region [p0, p1) of scaffold 1 is linked, and the one-base regions on either side of it are not — a
        projection one base longer on either side would link them.  P None: nothing is linked, whatever lies on scaffold 1."""
        assert path[0] == 0 and path[1] == 1
        if P is None:
            regions = [(0,) + tregion, (1, 0, 2000), (1, 2000, 4000)]
            fam, lnk = self.check([path], regions, [(0, 0) + tregion], 1)
            assert fam == [0, 1, 2] and lnk == [0, 0, 0]
            return
        p0, p1 = P
        regions = [(0,) + tregion] + ([(1, p0 - 1, p0)] if p0 else []) + [(1, p0, p1)] + ([(1, p1, p1 + 1)] if p1 < self.L[1] else [])
        k = 2 if p0 else 1
        fam, lnk = self.check([path], regions, [(0, 0) + tregion], pct)
        assert fam == [0 if i in (0, k) else i for i in range(len(regions))] and lnk == [1] + [0] * (len(regions) - 1), (P, fam, lnk)


@pytest.fixture(scope='module')
def small(eng):
    s = Small(eng)
    yield s
    s.G.close()


# an insertion of 5 query bases in front of target base 350, then target bases [400, 410) deleted
PATH3 = [(300, 1300, 50), (350, 1355, 50), (410, 1405, 90)]


def test_restatement_on_paper():
    """The restatement itself on numbers small enough to do by hand"""
    L = [5000, 4000, 3000]
    recs, first, blocks = make_paths(L, [(0, 1, 0, PATH3), (0, 1, 1, PATH3)])
    regions = [(0, 320, 400), (1, 1320, 1405), (1, 2595, 2680), (1, 2680, 2780)]
    # [320, 400) under the plus-strand path: columns 320 .. 399 -> q 1320 .. 1404: P = [1320, 1405), all of region 1
    fam, lnk = restate(L, None, recs, first, blocks, regions, [(0, 0, 320, 400)], 100)
    assert fam.tolist() == [0, 0, 2, 3] and lnk.tolist() == [1, 0, 0, 0]
    # the minus-strand path: [4000 - 1405, 4000 - 1320) = [2595, 2680), all of region 2 and nothing of region 3
    fam, lnk = restate(L, None, recs, first, blocks, regions, [(1, 0, 320, 400)], 100)
    assert fam.tolist() == [0, 1, 0, 3] and lnk.tolist() == [1, 0, 0, 0]
    # 79 of 80 bases: rule A says no at 99 per cent and yes at 98; then P = [1320, 1404): 84 of region 1's 85 bases: 98.8 per cent
    assert restate(L, None, recs, first, blocks, regions, [(0, 0, 320, 399)], 99)[1].tolist() == [0, 0, 0, 0]
    assert restate(L, None, recs, first, blocks, regions, [(0, 0, 320, 399)], 98)[1].tolist() == [1, 0, 0, 0]
    # both items, twice each: links counts every one, the family is the smallest member
    fam, lnk = restate(L, None, recs, first, blocks, regions, [(1, 0, 320, 400), (0, 0, 320, 400)] * 2, 100)
    assert fam.tolist() == [0, 0, 0, 3] and lnk.tolist() == [4, 0, 0, 0]


def test_windows_and_blocks(small):
    plus = (0, 1, 0, PATH3)
    small.projects_to(plus, (310, 340), (1310, 1340))     # a window inside one block
    small.projects_to(plus, (320, 400), (1320, 1405))     # w0 mid-block, w1 exactly on a block's end; the insertion lies inside
    small.projects_to(plus, (404, 484), (1405, 1479))     # a window that starts in the deletion: the first column is base 410
    small.projects_to(plus, (360, 405), (1365, 1405))     # ... and one that ends in it: the last column is base 399
    small.projects_to(plus, (401, 409), None)             # wholly inside the deletion: no column, no link
    small.projects_to(plus, (400, 410), None)             # the deletion exactly
    small.projects_to(plus, (350, 400), (1355, 1405))     # the insertion at the window's edge is not part of the projection
    small.projects_to(plus, (300, 350), (1300, 1350))
    small.projects_to(plus, (300, 351), (1300, 1356))     # one column further: the insertion is spanned
    small.projects_to(plus, (250, 520), (1300, 1495))     # a region larger than the alignment, covered whole by the window: the path's ends
    small.projects_to(plus, (100, 300), None)             # a region that abuts the alignment
    small.projects_to(plus, (500, 600), None)
    small.projects_to((0, 1, 0, [(100, 1000, 100)]), (100, 200), (1000, 1100))   # a one-block path
    small.projects_to((0, 1, 0, [(100, 1000, 100)]), (150, 151), (1050, 1051))   # one base
    small.projects_to((0, 1, 0, []), (150, 151), None)                           # an alignment without blocks
    small.projects_to((0, 1, 0, [(0, 0, 4000)]), (0, 4000), (0, 4000))           # from base 0 to the query's last base


def test_minus_strand(small):
    Lq = small.L[1]
    small.projects_to((0, 1, 1, [(100, Lq - 100, 100)]), (100, 200), (0, 100))        # reaches base 0 of the query
    small.projects_to((0, 1, 1, [(300, 0, 100)]), (300, 400), (Lq - 100, Lq))         # ... and base Lq - 1
    small.projects_to((0, 1, 1, [(300, 0, 100)]), (399, 400), (Lq - 100, Lq - 99))    # the window's LAST base lands on the projection's first
    small.projects_to((0, 1, 1, [(0, 0, Lq)]), (0, 1), (Lq - 1, Lq))
    minus = (0, 1, 1, PATH3)
    small.projects_to(minus, (320, 400), (Lq - 1405, Lq - 1320))
    small.projects_to(minus, (404, 484), (Lq - 1479, Lq - 1405))
    small.projects_to(minus, (401, 409), None)


def test_binary_search_in_a_path_of_200_blocks(small):
    """windows deep inside a path of 200 short blocks, every block boundary and gap among their ends; the query scaffold is
    tiled with 7-base regions, so a projection that is off by a base links another set of tiles"""
    rng = np.random.default_rng(71)
    for strand in (0, 1):
        blk, t, q = [], 3, 17
        for _ in range(200):
            ln = int(rng.integers(1, 16))
            blk.append((t, q, ln))
            kind = int(rng.integers(0, 3))   # an insertion, a deletion, or both
            t, q = t + ln + (int(rng.integers(1, 4)) if kind != 0 else 0), q + ln + (int(rng.integers(1, 4)) if kind != 1 else 0)
        assert len(blk) == 200 and t < small.L[0] and q < small.L[1]
        tiles = [(1, s, min(s + 7, small.L[1])) for s in range(0, small.L[1], 7)]
        # disjoint target regions between sorted cuts, many of them on a block's start, a block's end or inside a gap
        edges = sorted({b[0] for b in blk[60:190:3]} | {b[0] + b[2] for b in blk[61:190:4]} | {b[0] + b[2] + 1 for b in blk[62:190:5]})
        tregions = [(0, a, b) for a, b in zip(edges[:-1], edges[1:])]
        regions = tregions + tiles
        items = [(0, i, r[1], r[2]) for i, r in enumerate(tregions)]
        items += [(0, i, r[1] + (r[2] - r[1]) // 3, r[2]) for i, r in enumerate(tregions)]   # part of the region: rule A at 1 per cent lets it through
        assert len(tregions) > 60
        for pct in (1, 50, 100):
            fam, lnk = small.check([(0, 1, strand, blk)], regions, items, pct)
            assert sum(lnk) > 30 and sum(lnk[len(tregions):]) == 0
        assert fam != list(range(len(regions)))


def test_rules_a_and_c_at_their_boundary(small):
    one = [(0, 1, 0, [(100, 1000, 100)])]
    # A: a region of 100 bases at 80 per cent: a window of 80 links, a window of 79 does not
    regions = [(0, 100, 200), (1, 1000, 1079)]
    assert small.check(one, regions, [(0, 0, 100, 180)], 80) == ([0, 0], [1, 0])
    assert small.check(one, regions, [(0, 0, 100, 179)], 80) == ([0, 1], [0, 0])
    assert small.check(one, regions, [(0, 0, 121, 200)], 80) == ([0, 1], [0, 0])
    # C: the projection [1000, 1100) over 80 and over 79 bases of a region of 100
    assert small.check(one, [(0, 100, 200), (1, 1020, 1120)], [(0, 0, 100, 200)], 80) == ([0, 0], [1, 0])
    assert small.check(one, [(0, 100, 200), (1, 1021, 1121)], [(0, 0, 100, 200)], 80) == ([0, 1], [0, 0])
    assert small.check(one, [(0, 100, 200), (1, 920, 1020), (1, 1021, 1121)], [(0, 0, 100, 200)], 80) == ([0, 1, 2], [0, 0, 0])
    assert small.check(one, [(0, 100, 200), (1, 920, 1020), (1, 1020, 1120)], [(0, 0, 100, 200)], 20) == ([0, 0, 0], [2, 0, 0])
    # 1 per cent: one base of 100 on either side; one base of 101 is not 1 per cent; an empty window never links
    assert small.check(one, [(0, 100, 200), (1, 1050, 1150)], [(0, 0, 199, 200)], 1) == ([0, 0], [1, 0])   # base 199 -> 1099: 1 of 100
    assert small.check(one, [(0, 100, 200), (1, 1099, 1199)], [(0, 0, 199, 200)], 1) == ([0, 0], [1, 0])
    assert small.check(one, [(0, 100, 200), (1, 1099, 1200)], [(0, 0, 199, 200)], 1) == ([0, 1], [0, 0])
    assert small.check(one, [(0, 100, 201), (1, 1099, 1199)], [(0, 0, 199, 200)], 1) == ([0, 1], [0, 0])
    assert small.check(one, [(0, 100, 200), (1, 1000, 1100)], [(0, 0, 150, 150)], 1) == ([0, 1], [0, 0])
    # 100 per cent: everything of both
    assert small.check(one, [(0, 100, 200), (1, 1000, 1100)], [(0, 0, 100, 200)], 100) == ([0, 0], [1, 0])
    assert small.check(one, [(0, 100, 200), (1, 1000, 1100)], [(0, 0, 100, 199)], 100) == ([0, 1], [0, 0])
    assert small.check(one, [(0, 100, 200), (1, 1000, 1101)], [(0, 0, 100, 200)], 100) == ([0, 1], [0, 0])
    assert small.check(one, [(0, 100, 200), (1, 999, 1100)], [(0, 0, 100, 200)], 100) == ([0, 1], [0, 0])


def test_region_table(small):
    # a projection [1000, 2000) over five regions of scaffold 1, the outer two half covered; region 6 has the coordinates of a
    # covered one on scaffold 2 and must not link
    wide = [(0, 1, 0, [(0, 1000, 1000)])]
    regions = [(0, 0, 1000), (1, 950, 1050), (1, 1100, 1200), (1, 1300, 1500), (1, 1700, 1800), (1, 1950, 2050), (2, 1100, 1200)]
    item = [(0, 0, 0, 1000)]
    assert small.check(wide, regions, item, 80) == ([0, 1, 0, 0, 0, 5, 6], [3, 0, 0, 0, 0, 0, 0])
    assert small.check(wide, regions, item, 50) == ([0, 0, 0, 0, 0, 0, 6], [5, 0, 0, 0, 0, 0, 0])
    assert small.check(wide, regions, item, 51) == ([0, 1, 0, 0, 0, 5, 6], [3, 0, 0, 0, 0, 0, 0])
    # the first and the last region of the query scaffold's share of the table, and a query scaffold without regions
    assert small.check(wide, [(0, 0, 1000), (1, 1000, 1001), (1, 1999, 2000)], item, 100) == ([0, 0, 0], [2, 0, 0])
    assert small.check([(0, 2, 0, [(0, 1000, 1000)])], [(0, 0, 1000), (1, 1000, 1001)], item, 1) == ([0, 1], [0, 0])
    assert small.check([(0, 2, 0, [(0, 1000, 1000)])], [(0, 0, 1000), (1, 1000, 1100), (2, 1000, 1100)], item, 1) == ([0, 1, 0], [1, 0, 0])
    # s == r neither links nor counts: a tandem copy inside the region; the next region of the same scaffold does both
    tandem = [(0, 0, 0, [(100, 150, 100)])]
    assert small.check(tandem, [(0, 100, 200)], [(0, 0, 100, 200)], 50) == ([0], [0])
    assert small.check(tandem, [(0, 100, 200), (0, 200, 300)], [(0, 0, 100, 200)], 50) == ([0, 0], [1, 0])
    assert small.check(tandem, [(0, 100, 200), (0, 200, 300), (0, 300, 301)], [(0, 0, 100, 200)] * 3, 50) == ([0, 0, 2], [3, 0, 0])
    # links[] is the linking region's: the partner's stays zero unless an item of its own links back
    back = [(0, 1, 0, [(100, 1000, 100)]), (1, 0, 0, [(1000, 100, 100)])]
    regions = [(0, 100, 200), (1, 1000, 1100)]
    assert small.check(back, regions, [(0, 0, 100, 200)], 80) == ([0, 0], [1, 0])
    assert small.check(back, regions, [(0, 0, 100, 200), (1, 1, 1000, 1100), (1, 1, 1010, 1100)], 80) == ([0, 0], [1, 2])


def test_chrom_of_scaf_is_not_the_identity(small):
    """FASTA order is not the sorted order: chromosome 0 is scaffold 1 (4000 bases), 1 is scaffold 2 (3000), 2 is scaffold 0
    (5000).  The target region lies where only scaffold 0 has bases; the minus-strand flip needs the query scaffold's length,
    and region 1 sits where the flip would land with scaffold 2's."""
    chrom = [2, 0, 1]
    paths = [(0, 1, 1, [(4800, 0, 100)])]   # scaffold 0 [4800, 4900) onto the last 100 bases of scaffold 1's plus strand
    regions = [(0, 3900, 4000), (1, 2900, 3000), (2, 3900, 4000), (2, 4800, 4900)]
    assert small.check(paths, regions, [(0, 3, 4800, 4900)], 80, chrom) == ([0, 1, 2, 0], [0, 0, 0, 1])
    # the same call under the identity is refused: chromosome 0 would be scaffold 0, and the item's region another scaffold's
    recs, first, blocks = make_paths(small.L, paths)
    with pytest.raises(RuntimeError, match=r'mimeo_link_regions: region 2 \(chrom 2, \[3900, 4000\)\): end is beyond its scaffold'):
        small.eng.link_regions(small.G, recs, first, blocks, regions_of(regions), None, [(0, 3, 4800, 4900)], 80)
    # every scaffold in every role
    paths = [(0, 1, 0, [(100, 1000, 100)]), (1, 2, 0, [(1000, 2000, 100)]), (2, 0, 1, [(2000, 5000 - 200, 100)])]
    regions = [(0, 1000, 1100), (1, 2000, 2100), (2, 100, 200)]
    items = [(0, 2, 100, 200), (1, 0, 1000, 1100), (2, 1, 2000, 2100)]
    assert small.check(paths, regions, items[:1], 80, chrom) == ([0, 1, 0], [0, 0, 1])
    assert small.check(paths, regions, items[1:2], 80, chrom) == ([0, 0, 2], [1, 0, 0])
    assert small.check(paths, regions, items[2:], 80, chrom) == ([0, 1, 1], [0, 1, 0])
    assert small.check(paths, regions, items, 80, chrom) == ([0, 0, 0], [1, 1, 1])


# ---- union-find ------------------------------------------------------------------------------------------------------------

UF_L = [600_000, 300_000, 150_000]
UF_CHAIN, UF_STAR, UF_PAIRS = 4000, 2000, 500


def uf_case(repeats):
    """7000 regions of 100 bases, every 150 bases: a chain of 4000 on scaffold 0 linked i <-> i + 1, a star of 2000 on scaffold
    1 all linked with its LAST region (on the minus strand), 500 separate pairs on scaffold 2.  Every link is an alignment of
    one 100-column block from the one region onto its partner, and one in the other direction; every item comes `repeats`
    times.  The chain's items come first, in reverse order."""
    start = lambda k: 150 * k + 20
    regions = [(0, start(k), start(k) + 100) for k in range(UF_CHAIN)] + [(1, start(k), start(k) + 100) for k in range(UF_STAR)] + \
              [(2, start(k), start(k) + 100) for k in range(2 * UF_PAIRS)]
    paths, items = [], []

    def link(scaf, base, i, j, strand):
        for a, b in ((i, j), (j, i)):
            q = UF_L[scaf] - (start(b) + 100) if strand else start(b)
            items.append((len(paths), base + a, start(a), start(a) + 100))
            paths.append((scaf, scaf, strand, [(start(a), q, 100)]))
    for i in range(UF_CHAIN - 1):
        link(0, 0, i, i + 1, i & 1)
    items.reverse()
    for j in range(UF_STAR - 1):
        link(1, UF_CHAIN, j, UF_STAR - 1, 1)
    for k in range(UF_PAIRS):
        link(2, UF_CHAIN + UF_STAR, 2 * k, 2 * k + 1, 0)
    recs, first, blocks = make_paths(UF_L, paths)
    return recs, first, blocks, regions, np.array(items * repeats, dtype=np.uint32)


@pytest.fixture(scope='module')
def uf(eng):
    rng = np.random.default_rng(72)
    G = eng.Genome(['u0', 'u1', 'u2'], [_ACGT[rng.integers(0, 4, n)] for n in UF_L])
    recs, first, blocks, regions, items = uf_case(8)
    exp = restate(UF_L, None, recs, first, blocks, regions, items, 80)
    yield G, recs, first, blocks, regions, items, exp
    G.close()


def test_union_find_chain_star_and_pairs(eng, uf):
    G, recs, first, blocks, regions, items, (efam, elnk) = uf
    nreg = len(regions)
    assert 100_000 <= items.shape[0] <= 110_000 and nreg == 7000
    # the restatement, on paper: the chain is family 0, the star the number of ITS first region, a pair its even member
    want = [0] * UF_CHAIN + [UF_CHAIN] * UF_STAR + [UF_CHAIN + UF_STAR + 2 * (k // 2) for k in range(2 * UF_PAIRS)]
    assert efam.tolist() == want
    assert elnk[:3].tolist() == [8, 16, 16] and int(elnk[UF_CHAIN + UF_STAR - 1]) == 8 * (UF_STAR - 1) and int(elnk.sum()) == items.shape[0]
    reg = regions_of(regions)
    rng = np.random.default_rng(73)
    for order in (np.arange(items.shape[0]), rng.permutation(items.shape[0]), rng.permutation(items.shape[0])):
        fam, lnk = eng.link_regions(G, recs, first, blocks, reg, None, items[order], 80)
        assert fam.tolist() == want and lnk.tolist() == elnk.tolist()
        assert (fam <= np.arange(nreg)).all()
    # at 100 per cent nothing changes: every region is aligned whole
    fam, lnk = eng.link_regions(G, recs, first, blocks, reg, None, items, 100)
    assert fam.tolist() == want and lnk.tolist() == elnk.tolist()


CHILD = '''
import json
import os
import sys
import numpy as np
from mimeo_amd import engine
engine.init(0)
z = np.load(sys.argv[1])
G = engine.Genome(['u0', 'u1', 'u2'], [np.full(int(n), ord('A'), dtype=np.uint8) for n in z['L']])
out = {}
for e, env in enumerate(json.loads(sys.argv[3])):   # the switches are read by every call
    os.environ.update(env)
    for k in range(int(z['ncases'])):
        fam, lnk = engine.link_regions(G, z['recs%d' % k], z['first%d' % k], z['blocks%d' % k], z['regions%d' % k], None, z['items%d' % k], int(z['pct%d' % k]))
        out['fam%d_%d' % (e, k)], out['lnk%d_%d' % (e, k)] = fam, lnk
    for name in env:
        del os.environ[name]
np.savez(sys.argv[2], **out)
'''


def test_every_alignment_a_slice_of_its_own(eng, uf, tmp_path):
    """MIMEO_LINK_SLICE_BLOCKS=1 in a child process: the same arrays — the union-find lives across the slices.  Two cases: the
    chain, star and pairs with every item once (13 000 slices of one block), and a few paths of many blocks.  Then the same two
    cases under MIMEO_PATH_LAUNCH_JOBS: one job and three jobs per launch give the same arrays — the union-find lives across
    the launches — and the statistics line counts the launches; zero and a word mean the default."""
    G, _, _, _, _, _, _ = uf
    recs, first, blocks, regions, items = uf_case(1)
    rng = np.random.default_rng(74)
    paths = []
    for a in range(12):   # paths of 1 .. 60 blocks from scaffold 0 onto scaffold 1, on either strand
        blk, t, q = [], 1000 * a + int(rng.integers(0, 50)), 900 * a + int(rng.integers(0, 50))
        for _ in range(int(rng.integers(1, 61))):
            ln = int(rng.integers(1, 12))
            blk.append((t, q, ln))
            t, q = t + ln + int(rng.integers(0, 3)), q + ln + int(rng.integers(1, 3))
        paths.append((0, 1, a & 1, blk))
    r2, f2, b2 = make_paths(UF_L, paths)
    tregions = [(0, 250 * k, 250 * k + 200) for k in range(48)]
    regions2 = tregions + [(1, 61 * k, 61 * k + 50) for k in range(200)]
    items2 = np.array([(a, k, 250 * k, 250 * k + 200) for a in range(12) for k in range(4 * a, 4 * a + 4)], dtype=np.uint32)
    cases = [(recs, first, blocks, regions_of(regions), items, 80), (r2, f2, b2, regions_of(regions2), items2, 30)]
    here = [eng.link_regions(G, c[0], c[1], c[2], c[3], None, c[4], c[5]) for c in cases]
    assert here[1][1].sum() > 5 and (here[1][0] != np.arange(len(regions2))).sum() > 5   # the second case links something
    efam, elnk = restate(UF_L, None, r2, f2, b2, regions2, items2, 30)
    assert here[1][0].tolist() == efam.tolist() and here[1][1].tolist() == elnk.tolist()
    z = {'L': np.array(UF_L), 'ncases': np.array(len(cases))}
    for k, c in enumerate(cases):
        for name, v in zip(('recs', 'first', 'blocks', 'regions', 'items', 'pct'), c):
            z['%s%d' % (name, k)] = np.asarray(v)
    np.savez(tmp_path / 'in.npz', **z)
    (tmp_path / 'child.py').write_text(CHILD)
    envs = [{'MIMEO_LINK_SLICE_BLOCKS': '1'}, {}, {'MIMEO_PATH_LAUNCH_JOBS': '1'}, {'MIMEO_PATH_LAUNCH_JOBS': '3'}, {'MIMEO_PATH_LAUNCH_JOBS': '0'},
            {'MIMEO_PATH_LAUNCH_JOBS': 'abc'}]
    env = dict(os.environ, MIMEO_LINK_STATS='1', PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get('PYTHONPATH')) if p))
    for e in envs:
        for name in e:
            env.pop(name, None)
    r = subprocess.run([sys.executable, str(tmp_path / 'child.py'), str(tmp_path / 'in.npz'), str(tmp_path / 'out.npz'), json.dumps(envs)], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.load(tmp_path / 'out.npz')
    for e in range(len(envs)):
        for k, (fam, lnk) in enumerate(here):
            assert got['fam%d_%d' % (e, k)].tobytes() == fam.tobytes() and got['lnk%d_%d' % (e, k)].tobytes() == lnk.tobytes(), (envs[e], k)
    # the statistics line says what was done: every alignment that an item asks for a slice of its own
    lines = [l for l in r.stderr.splitlines() if l.startswith('[k12]')]
    assert len(lines) == 2 * len(envs), r.stderr
    assert '%d items' % items.shape[0] in lines[0] and 'slices %d of %d' % (recs.size, recs.size) in lines[0], r.stderr
    assert 'slices 12 of 12' in lines[1] and 'kernels' in lines[1]
    # ... and how many launches it took: k12_init, k12_flatten and the launches of the jobs.  A job is an item that passes
    # rule A (every path here has blocks): all 48 of the second case
    jobs2 = sum(1 for a, k, w0, w1 in items2.tolist() if 100 * (w1 - w0) >= 30 * (regions2[k][2] - regions2[k][1]))
    assert jobs2 == 48
    said = [tuple(int(x) for x in re.search(r'(\d+) jobs, .* launches (\d+),', l).groups()) for l in lines]
    assert all(j == jobs2 for j, _ in said[1::2]), r.stderr
    launches = {json.dumps(e): (said[2 * i][1], said[2 * i + 1][1]) for i, e in enumerate(envs)}
    assert launches['{}'][1] == 1 + 2                                               # one slice, one launch
    assert launches[json.dumps({'MIMEO_LINK_SLICE_BLOCKS': '1'})][1] == 12 + 2     # a launch per slice
    assert launches[json.dumps({'MIMEO_PATH_LAUNCH_JOBS': '1'})] == (said[0][0] + 2, jobs2 + 2)
    assert launches[json.dumps({'MIMEO_PATH_LAUNCH_JOBS': '3'})] == ((said[0][0] + 2) // 3 + 2, (jobs2 + 2) // 3 + 2)
    assert launches[json.dumps({'MIMEO_PATH_LAUNCH_JOBS': '0'})] == launches['{}'] == launches[json.dumps({'MIMEO_PATH_LAUNCH_JOBS': 'abc'})]


# ---- edge inputs -----------------------------------------------------------------------------------------------------------

def test_no_items_and_one_region(small):
    paths = [(0, 1, 0, [(100, 1000, 100)]), (0, 0, 0, [(100, 120, 80)])]
    recs, first, blocks = make_paths(small.L, paths)
    regions = [(0, 100, 200), (1, 1000, 1100), (2, 5, 6)]
    fam, lnk = small.eng.link_regions(small.G, recs, first, blocks, regions_of(regions), None, np.zeros((0, 4)), 80)
    assert fam.dtype == np.uint32 and fam.tolist() == [0, 1, 2] and lnk.dtype == np.uint64 and lnk.tolist() == [0, 0, 0]
    fam, lnk = small.eng.link_regions(small.G, recs[:0], first[:1], blocks[:0], regions_of(regions), None, np.zeros((0, 4)), 80)
    assert fam.tolist() == [0, 1, 2] and lnk.tolist() == [0, 0, 0]
    fam, lnk = small.eng.link_regions(small.G, recs, first, blocks, regions_of([]), None, np.zeros((0, 4)), 80)
    assert fam.size == 0 and lnk.size == 0
    # one region: the only thing a projection can hit is the region itself
    assert small.check(paths, [(0, 100, 200)], [(1, 0, 100, 200), (1, 0, 100, 180)], 50) == ([0], [0])
    # items that fail rule A, and nothing else: the kernels run over no job at all
    assert small.check(paths, regions, [(0, 0, 100, 150), (1, 0, 150, 150)], 80) == ([0, 1, 2], [0, 0, 0])


def test_rejected_input(small):
    eng = small.eng
    paths = [(0, 1, 0, PATH3), (1, 0, 1, [(1000, 0, 100)]), (2, 2, 0, [])]
    recs, first, blocks = make_paths(small.L, paths)
    regions = [(0, 320, 400), (0, 4900, 5000), (1, 1000, 1100), (1, 1320, 1405), (2, 0, 3000)]
    items = [(0, 0, 320, 400), (1, 2, 1000, 1100), (2, 4, 0, 3000)]
    ok = small.check(paths, regions, items, 80)
    assert ok == ([0, 1, 1, 0, 4], [1, 0, 1, 0, 0])   # region 0 onto region 3, region 2 onto region 1 through the minus strand

    def bad(match, regions=regions, items=items, pct=80, chrom=None, recs=recs, first=first, blocks=blocks):
        with pytest.raises(RuntimeError, match=r'mimeo_link_regions: ' + match) as e:
            eng.link_regions(small.G, recs, first, blocks, regions_of(regions), chrom, np.array(items, dtype=np.uint32).reshape(-1, 4), pct)
        assert '(code -1)' in str(e.value)   # MIMEO_ERR_ARG

    def edit(rows, i, **kw):
        names = ('chrom', 'start', 'end') if len(rows[0]) == 3 else ('aln', 'group', 'w0', 'w1')
        rows = [list(r) for r in rows]
        for k, v in kw.items():
            rows[i][names.index(k)] = v
        return [tuple(r) for r in rows]

    # min_cover_pct
    bad(r'min_cover_pct 0 is not in 1 \.\. 100', pct=0)
    bad(r'min_cover_pct 101 is not in 1 \.\. 100', pct=101)
    # everything mimeo_path_stats checks, under this name
    blk = blocks.copy()
    blk['len'][1] = 0
    bad(r'record 0, block 1 .*len is 0', blocks=blk)
    blk = blocks.copy()
    blk['q'][3] = small.L[0] - 99
    bad(r'record 1, block 3 .*q \+ len is beyond the query scaffold', blocks=blk)   # a self job: the query scaffold is T's scaffold 0
    r2 = recs.copy()
    r2['qid'][1] = 3
    bad(r'record 1: qid is not a scaffold', recs=r2)
    f2 = first.copy()
    f2[-1] += 1
    bad(r'record 2: path_first\[n\] is not nblocks', first=f2)
    # items
    bad(r'item 1 \(aln 3, region 2, window \[1000, 1100\)\): aln is not a record', items=edit(items, 1, aln=3))
    bad(r'item 2 \(aln 2, region 5, .*region is not below nreg', items=edit(items, 2, group=5))
    bad(r"item 0 \(aln 0, region 3, .*does not lie on the record's target scaffold", items=[(0, 3, 1320, 1405)])
    bad(r'item 0 .*window \[401, 400\)\): w0 is beyond w1', items=edit(items, 0, w0=401))
    bad(r'item 0 .*the window does not lie inside the region', items=edit(items, 0, w0=319))
    bad(r'item 1 .*the window does not lie inside the region', items=edit(items, 1, w1=1101))
    bad(r'item 2 .*the window does not lie inside the region', items=edit(items, 2, w1=0xFFFFFFFF))
    # regions: sorted, disjoint, inside their scaffolds
    bad(r'region 1 \(chrom 0, \[320, 400\)\): lies in front of the region before it', regions=[regions[1], regions[0]] + regions[2:])
    bad(r'region 3 \(chrom 1, \[1099, 1405\)\): lies in front of the region before it or overlaps it', regions=edit(regions, 3, start=1099))
    bad(r'region 4 \(chrom 0, .*lies in front of the region before it', regions=edit(regions, 4, chrom=0))
    bad(r'region 4 \(chrom 2, \[0, 3001\)\): end is beyond its scaffold', regions=edit(regions, 4, end=3001))
    bad(r'region 4 \(chrom 3, .*chrom is not a chromosome', regions=edit(regions, 4, chrom=3))
    bad(r'region 2 \(chrom 1, \[1000, 1000\)\): start is not below end', regions=edit(regions, 2, end=1000))
    # chrom_of_scaf
    bad(r'chrom_of_scaf\[1\] = 0 is also the chromosome of scaffold 0', chrom=[0, 0, 2])
    bad(r'chrom_of_scaf\[2\] = 3 is not below the number of scaffolds', chrom=[0, 1, 3])
    with pytest.raises(ValueError):
        eng.link_regions(small.G, recs, first[:-1], blocks, regions_of(regions), None, items, 80)
    with pytest.raises(ValueError):
        eng.link_regions(small.G, recs, first, blocks, regions_of(regions), [0, 1], items, 80)
    # nothing was launched and nothing is broken: the valid call answers as before
    assert small.check(paths, regions, items, 80) == ok


# ---- CLI end to end --------------------------------------------------------------------------------------------------------

PLANT_SEED = 9
COPIES = (6, 5, 4)
# depth 2 is the scaffold's own diagonal and one more row: under --chain a copy is aligned with at most one copy per scaffold and
# strand, so the default depth of 3 would ask every copy for partners on two scaffolds or strands
MIN_COV = ['--minCov', '2']


def planted_genome(seed):
    """Three scaffolds of 60 kbp of random sequence with three unrelated families of 6, 5 and 4 copies planted: consensus
    sequences of 800 to 1500 bp (synth.make_families), every copy with 5 % substitutions against its consensus — about 10 %
    between two copies — and a few short indels (synth._mutate), two copies in five reverse-complemented.  Copy j of family f
    lies on scaffold (j + f) % 3, in one of eight slots 6500 bp apart, drawn at random.  The FASTA order of the names is not
    their sorted order.  The engine chains like lastz --chain: of the HSPs of a scaffold pair and strand only the best collinear
    set becomes alignments, so which copies are aligned with which depends on their order along the scaffolds and on their
    strands, and a family falls apart where no chain bridges two of its parts.  PLANT_SEED is a layout in which the rule,
    restated, joins every planted family (test_cli_families (iii)).
    Returns (names, seqs, [(scaffold, start, end, family)])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    cons = make_families(rng, 3, cons_len=(800, 1500))
    codes = [rng.integers(0, 4, size=60_000, dtype=np.uint8) for _ in range(3)]
    slots = [rng.permutation(8).tolist() for _ in range(3)]
    planted = []
    for f, n in enumerate(COPIES):
        for j in range(n):
            cp = _mutate(rng, cons[f], 0.05, 0.003)
            if rng.random() < 0.4:
                cp = _COMP[cp[::-1]]
            s = (j + f) % 3
            p = 3000 + 6500 * slots[s].pop() + int(rng.integers(0, 500))
            codes[s][p:p + cp.size] = cp
            planted.append((s, p, p + cp.size, f))
    return ['zeta', 'alpha', 'mid'], [_ACGT[c] for c in codes], planted


def _cli(d, fa, extra, ranks=1):
    cmd = ['-m', 'mimeo_amd', 'self', '--afasta', fa, '-d', str(d)] + extra
    env = dict(os.environ)
    if ranks > 1:
        s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
        env.update(MIMEO_DIST_BACKEND='gloo', MIMEO_FORCE_DEVICE='0')
        cmd = ['-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', str(ranks), '--master-addr', '127.0.0.1', '--master-port', str(port)] + cmd
    r = subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return d


@pytest.fixture(scope='module')
def planted(tmp_path_factory):
    d = tmp_path_factory.mktemp('fam')
    names, seqs, copies = planted_genome(PLANT_SEED)
    fa = str(d / 'a.fa')
    write_fasta(fa, names, seqs)
    one = _cli(d / 'one', fa, MIN_COV + ['--families', str(d / 'one' / 'fam.tsv'), '--regionStats', str(d / 'one' / 'rs.tsv')])
    return d, names, seqs, copies, fa, one


def _expected_file(eng, names, seqs, strict, min_cov=3, intra_cov=5, cover=80):
    """The --families file from the engine's own records, paths and regions (workflow.align_blocks, engine.coverage_collapse as
    workflow.collapse_to_gff calls it, formats.region_items) and the restatement."""
    from mimeo_amd import formats, workflow
    A = eng.Genome(names, seqs)
    pairs = workflow.all_pairs(len(names))
    _, _, kept, _, (recs, first, blk) = workflow.align_blocks(A, None, pairs, workflow.gapped_params(3000, 'box', False), 100, 60, paths=True, paf_rows=False)
    names_sorted = sorted(names, key=lambda s: s.encode())
    chrom_of_tid = [names_sorted.index(n) for n in names]
    L = [int(s.size) for s in seqs]
    intra = kept[:, 0] == kept[:, 1]
    lines, nitems = [], 0
    for sel, cov, suffix in ((~intra, min_cov, ''), (intra, intra_cov, '_intra')) if strict else ((np.ones(intra.size, bool), min_cov, ''),):
        rows = np.flatnonzero(sel)
        iv = np.stack([np.array(chrom_of_tid, dtype=np.uint32)[kept[rows, 0]], kept[rows, 2].astype(np.uint32), kept[rows, 3].astype(np.uint32)], axis=1)
        regions = eng.coverage_collapse(iv, [L[names.index(n)] for n in names_sorted], cov, 100) if rows.size else np.zeros(0, dtype=_ffi.INTERVAL)
        f2, b2 = formats.select_paths(first, blk, rows)
        items, _ = formats.region_items(recs[rows], regions, chrom_of_tid, first=f2, blocks=b2, self_job=True)
        fam, lnk = restate(L, chrom_of_tid, recs[rows], f2, b2, regions.tolist(), [tuple(int(x) for x in it) for it in items], cover)
        lines += formats.family_lines(regions, names_sorted, 'Self_Repeat', fam, lnk, suffix=suffix, header=not suffix)
        nitems += items.size
    A.close()
    return lines, nitems


def test_cli_families(eng, planted, tmp_path):
    d, names, seqs, copies, fa, one = planted
    plain = _cli(tmp_path / 'plain', fa, MIN_COV + ['--regionStats', str(tmp_path / 'plain' / 'rs.tsv')])
    # (iv) nothing else changes
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3', 'rs.tsv'):
        assert (one / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(os.listdir(one)) == sorted(os.listdir(plain) + ['fam.tsv'])
    lines = (one / 'fam.tsv').read_text().splitlines()
    gff = [l.split('\t') for l in (one / 'mimeo-self_repeats.gff3').read_text().splitlines() if not l.startswith('#')]
    # (i) one line per feature, in the order and with the numbers of the GFF3
    assert lines[0] == '#ID\tseqid\tstart\tend\tfamily\tmembers\tfamily_bases\tlinks'
    rows = [l.split('\t') for l in lines[1:]]
    assert len(rows) == len(gff) >= sum(COPIES) and all(len(r) == 8 for r in rows)
    assert [r[:4] for r in rows] == [[g[8][3:], g[0], g[3], g[4]] for g in gff]
    # (ii) the families are the restatement's, on the engine's own records, paths and regions
    exp, nitems = _expected_file(eng, names, seqs, strict=False, min_cov=2)
    assert nitems >= 2 * sum(COPIES) and lines == exp
    check_planted(rows, names, copies)
    assert all(int(r[7]) > 0 for r in rows)


def check_planted(rows, names, copies):
    """(iii) the features of a planted family's copies share one family, and share it with nobody else.  rows: the fields of
    the lines of the --families file, without the header."""
    label = {}
    for r in rows:
        s, a, b = names.index(r[1]), int(r[2]), int(r[3])
        over = [c for c in copies if c[0] == s and a < c[2] and c[1] < b]
        assert len(over) == 1, (r, over)
        label.setdefault(over[0][3], []).append((over[0], r[4], int(r[5])))
    assert sorted(label) == [0, 1, 2]
    for f, got in label.items():
        assert len({g[1] for g in got}) == 1, (f, got)                              # one name
        assert {g[0] for g in got} == {c for c in copies if c[3] == f}, (f, got)    # every copy has a feature
        assert {g[2] for g in got} == {len(got)}, (f, got)                          # `members` counts exactly these features
    assert len({got[0][1] for got in label.values()}) == 3


def test_cli_families_strict_self(eng, planted, tmp_path):
    d, names, seqs, copies, fa, one = planted
    # depth 1 on the same-scaffold rows is every scaffold's own diagonal: the intra block has regions whatever the layout (three
    # scaffold-long ones, which nothing covers to 70 per cent but the diagonal, and that is left out: three families of one)
    extra = ['--strictSelf', '--minCov', '2', '--intraCov', '1']
    plain = _cli(tmp_path / 'plain', fa, extra)
    fam = _cli(tmp_path / 'fam', fa, extra + ['--families', str(tmp_path / 'fam' / 'fam.tsv'), '--familyCover', '70'])
    for f in ('mimeo_alignment.tab', 'mimeo_alignment.tab_intra.tab', 'mimeo-self_repeats.gff3'):
        assert (fam / f).read_bytes() == (plain / f).read_bytes(), f
    lines = (fam / 'fam.tsv').read_text().splitlines()
    gff = [l.split('\t') for l in (fam / 'mimeo-self_repeats.gff3').read_text().splitlines() if not l.startswith('#')]
    rows = [l.split('\t') for l in lines[1:]]
    assert [r[:4] for r in rows] == [[g[8][3:], g[0], g[3], g[4]] for g in gff]
    # the intra block follows the main one, linked on its own: restarted IDs, names of its own
    n_intra = sum(g[2].endswith('_intra') for g in gff)
    assert 0 < n_intra < len(rows) and [r[4].endswith('_intra') for r in rows] == [g[2].endswith('_intra') for g in gff]
    assert rows[0][4] == 'F1' and rows[len(rows) - n_intra][4] == 'F1_intra' and rows[len(rows) - n_intra][0] == 'Self_Repeat_00001'
    exp, _ = _expected_file(eng, names, seqs, strict=True, min_cov=2, intra_cov=1, cover=70)
    assert lines == exp


def test_cli_families_two_ranks(planted, tmp_path):
    d, names, seqs, copies, fa, one = planted
    two = _cli(tmp_path / 'two', fa, MIN_COV + ['--families', str(tmp_path / 'two' / 'fam.tsv'), '--regionStats', str(tmp_path / 'two' / 'rs.tsv')], ranks=2)
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3', 'rs.tsv', 'fam.tsv'):
        assert (two / f).read_bytes() == (one / f).read_bytes(), f


def test_cli_recycled_tab_writes_nothing(planted, tmp_path):
    d, names, seqs, copies, fa, one = planted
    out = tmp_path / 'again'
    out.mkdir()
    (out / 'mimeo_alignment.tab').write_bytes((one / 'mimeo_alignment.tab').read_bytes())
    r = subprocess.run([sys.executable, '-m', 'mimeo_amd', 'self', '--afasta', fa, '-d', str(out), '--recycle', '--families', str(out / 'fam.tsv')] + MIN_COV,
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert not (out / 'fam.tsv').exists() and "--families needs the alignments' paths" in r.stderr
    assert (out / 'mimeo-self_repeats.gff3').read_bytes() == (one / 'mimeo-self_repeats.gff3').read_bytes()
