"""Window-clipped column statistics (mimeo_path_window_stats, kernel K10; engine.window_stats; `--regionStats`) against a plain
numpy restatement of the rules in include/mimeo_hip.h, written here from the sequences and the blocks alone: per target base
of [tstart, tend) what its column is (match / transition / transversion / ambiguous, or a deleted base under no block), per
gap where it starts and what it inserts; a window is a difference of prefix sums.  Equality is exact, field by field."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi
from mimeo_amd.synth import make_families, synth_genome, tandem_genome, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_runs', 'ins_bases', 'del_runs', 'del_bases')
CODE = np.full(256, 4, dtype=np.int64)
COMP = np.full(256, ord('N'), dtype=np.uint8)
for _k, (_c, _d) in enumerate(zip(b'ACGT', b'TGCA')):
    CODE[_c] = _k
    CODE[_c + 32] = _k
    COMP[_c] = _d
    COMP[_c + 32] = _d + 32


def revcomp(a):
    return COMP[a][::-1].copy()


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


# ---- the restatement -------------------------------------------------------------------------------------------------------

class PathOracle:
    """One alignment: T / Q the target scaffold and the query scaffold on the aligned strand (uint8 bases), blk its blocks."""

    def __init__(self, T, Q, blk):
        t, q, ln = (blk[f].astype(np.int64) for f in ('t', 'q', 'len'))
        self.t0 = self.t1 = 0
        self.cum = np.zeros((8, 1), dtype=np.int64)
        if t.size == 0:
            return
        self.t0, self.t1 = int(t[0]), int(t[-1] + ln[-1])
        n = self.t1 - self.t0
        cat = np.full(n, 4, dtype=np.int64)   # a target base of [tstart, tend) under no block is a deleted base
        for k in range(t.size):
            x, y = CODE[T[int(t[k]):int(t[k] + ln[k])]], CODE[Q[int(q[k]):int(q[k] + ln[k])]]
            assert x.size == y.size == int(ln[k])
            cat[int(t[k]) - self.t0:int(t[k] + ln[k]) - self.t0] = np.where((x == 4) | (y == 4), 3, np.where(x == y, 0, np.where((x ^ y) == 2, 1, 2)))
        per_base = np.zeros((8, n), dtype=np.int64)
        for field, c in ((0, 0), (1, 1), (2, 2), (3, 3), (7, 4)):
            per_base[field] = cat == c
        # a gap belongs to target base p = the end of the block before it: the insertion sits in front of that base, the deletion
        # run starts on it
        p = t[:-1] + ln[:-1]
        dt, dq = t[1:] - p, q[1:] - (q[:-1] + ln[:-1])
        assert ((dt >= 0) & (dq >= 0)).all()
        per_base[4][p - self.t0] = dq > 0
        per_base[5][p - self.t0] = dq
        per_base[6][p - self.t0] = dt > 0
        self.cum = np.zeros((8, n + 1), dtype=np.int64)
        self.cum[:, 1:] = np.cumsum(per_base, axis=1)

    def windows(self, w0, w1):
        """(n, 8) counts of the windows [w0[i], w1[i])"""
        a = np.clip(np.asarray(w0, dtype=np.int64), self.t0, self.t1) - self.t0
        b = np.clip(np.asarray(w1, dtype=np.int64), self.t0, self.t1) - self.t0
        return (self.cum[:, b] - self.cum[:, a]).T

    def whole(self):
        return self.cum[:, -1]


class Case:
    """A genome on the device, made-up paths over it and their restatement"""

    def __init__(self, names, seqs):
        self.names, self.seqs = names, seqs
        self.L = [int(s.size) for s in seqs]
        self.rc = {}
        self.recs, self.first, self.blocks, self.what = [], [0], [], {}

    def strand(self, qid, strand):
        if not strand:
            return self.seqs[qid]
        if qid not in self.rc:
            self.rc[qid] = revcomp(self.seqs[qid])
        return self.rc[qid]

    def add(self, what, tid, qid, strand, blk):
        t_end = q_end = 0
        for t, q, ln in blk:   # the contract of mimeo_path_block, so that a slip in a table is not taken for a kernel's
            assert ln >= 1 and t >= t_end and q >= q_end and t + ln <= self.L[tid] and q + ln <= self.L[qid], (what, t, q, ln)
            t_end, q_end = t + ln, q + ln
        self.what.setdefault(what, []).append(len(self.recs))
        self.recs.append((tid, qid, strand))
        self.blocks.extend(blk)
        self.first.append(len(self.blocks))

    def finish(self):
        r = np.zeros(len(self.recs), dtype=_ffi.ALIGNMENT)
        r['tid'], r['qid'], r['qstrand'] = [x[0] for x in self.recs], [x[1] for x in self.recs], [x[2] for x in self.recs]
        self.recs, self.first, self.blocks = r, np.array(self.first, dtype=np.uint64), np.array(self.blocks, dtype=_ffi.PATH_BLOCK)
        self.oracle = [PathOracle(self.seqs[int(a['tid'])], self.strand(int(a['qid']), int(a['qstrand'])), self.blk(i)) for i, a in enumerate(r)]
        return self

    def blk(self, i):
        return self.blocks[int(self.first[i]):int(self.first[i + 1])]

    def expected(self, items, ngroups):
        items = np.asarray(items, dtype=np.int64).reshape(-1, 4)
        exp = np.zeros((ngroups, 8), dtype=np.int64)
        for a in np.unique(items[:, 0]).tolist():
            it = items[items[:, 0] == a]
            np.add.at(exp, it[:, 1], self.oracle[a].windows(it[:, 2], it[:, 3]))
        return exp


def same(got, exp, tag):
    assert got.dtype == _ffi.WINDOW_STATS and got.shape == (exp.shape[0],), tag
    for k, f in enumerate(FIELDS):
        bad = np.flatnonzero(got[f].astype(np.int64) != exp[:, k])
        assert bad.size == 0, (tag, f, bad[:5], got[f][bad[:5]], exp[bad[:5], k])


N_RUNS = ((5000, 5400), (12_000, 12_001), (19_990, 19_999))   # of scaffold 1; the last one ends the scaffold
MODS = (0, 1, 31, 32, 33, 63)
EDGES = (-1, 0, 1, 31, 32, 33, 63, 64, 65, 199, 200, 201)
CHAINS = (1, 64, 65, 200)


def _genome():
    rng = np.random.default_rng(30)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    s = [acgt[rng.integers(0, 4, n)].copy() for n in (20_000, 19_999, 20_345)]
    for a, b in N_RUNS:
        s[1][a:b] = ord('N')
    s[1][7000:7300] += 32    # soft-masked stretches, one running into an N
    s[1][11_990:12_010] = np.where(s[1][11_990:12_010] == ord('N'), ord('n'), s[1][11_990:12_010] + 32)
    s[1][100] = ord('R')     # an IUPAC code is an N to the engine
    s[0][230] = ord('Y')
    return ['w0', 'w1', 'w2'], s


def _chain(rng, nb, t, q, max_len):
    blk = []
    for _ in range(nb):
        ln = int(rng.integers(1, max_len + 1))
        blk.append((t, q, ln))
        kind = int(rng.integers(0, 3))   # an insertion, a deletion, or both
        t, q = t + ln + (int(rng.integers(1, 4)) if kind != 0 else 0), q + ln + (int(rng.integers(1, 4)) if kind != 1 else 0)
    return blk


@pytest.fixture(scope='module')
def made(eng):
    names, s = _genome()
    c = Case(names, s)
    rng = np.random.default_rng(31)
    # 1: four blocks of 20-70 columns with an insertion, a deletion and both at once between them, over the IUPAC letters of
    # both scaffolds (target base 100 of scaffold 1, query base 230 of scaffold 0), on either strand
    c.add('small', 1, 0, 0, [(80, 200, 45), (125, 252, 70), (200, 322, 20), (223, 345, 33)])
    c.add('small', 1, 0, 1, [(80, c.L[0] - 300, 45), (125, c.L[0] - 248, 70), (200, c.L[0] - 178, 20), (223, c.L[0] - 155, 33)])
    # 2: one block of 200 columns at every t mod 64 and q mod 64 of MODS
    for i, tm in enumerate(MODS):
        for j, qm in enumerate(MODS):
            c.add('mods', (i + j) % 3, (i + 2 * j + 1) % 3, (i * 6 + j) & 1, [(64 * (3 + i) + tm, 64 * (9 + j) + qm, 200)])
    # 3: chains of 1, 64, 65 and 200 blocks; the last block of a second set ends on the last base of the target, on either strand
    for nb in CHAINS:
        for strand in (0, 1):
            c.add('chain %d' % nb, 0, 1, strand, _chain(rng, nb, 3, 17, 90))
    for strand in (0, 1):
        blk = _chain(rng, 70, 11_000, 9000, 90)
        blk.append((c.L[2] - 150, blk[-1][1] + blk[-1][2] + 2, 150))
        c.add('to the end', 2, 1, strand, blk)
        c.add('to the end', 1, 2, strand, [(c.L[1] - 40, c.L[2] - 40, 40)])   # inside the N run that ends scaffold 1
    # 5: a block of 10 000 columns, and a path with two long blocks around a deletion
    for strand in (0, 1):
        c.add('long', 0, 1, strand, [(33, 1, 10_000)])
        c.add('long', 1, 0, strand, [(64, 127, 9000), (9070, 9127, 10_000)])
    # blocks lying wholly in N; T and Q the same scaffold on and off the main diagonal; no blocks at all
    a, b = N_RUNS[0]
    c.add('in N', 1, 0, 0, [(a + 10, 700, 300)])
    c.add('in N', 0, 1, 1, [(700, c.L[1] - b + 10, 300)])
    for strand in (0, 1):
        c.add('same', 0, 0, strand, [(100, 100, 500), (1000, 3000, 500)])
    c.add('empty', 2, 1, 0, [])
    c.add('diagonal', 0, 0, 0, [(0, 0, 20_000)])   # a whole scaffold against itself: every column but the IUPAC letter's a match
    # many short paths: several workgroups
    for _ in range(1500):
        tid, qid = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        c.add('many', tid, qid, int(rng.integers(0, 2)), _chain(rng, int(rng.integers(1, 6)), int(rng.integers(0, 5000)), int(rng.integers(0, 5000)), 200))
    c.finish()
    c.G = eng.Genome(names, s)
    yield c
    c.G.close()


def run(eng, c, items, ngroups):
    return eng.window_stats(c.G, None, c.recs, c.first, c.blocks, np.asarray(items, dtype=np.uint32).reshape(-1, 4), ngroups)


def test_restatement_on_paper():
    """The restatement itself, on a path small enough to count by hand: T = AAAAACCCCCGGGGG..., three blocks."""
    T = np.frombuffer(b'AAAAACCCCCGGGGGTTTTTAAAAANNNNN', dtype=np.uint8)
    Q = np.frombuffer(b'AAGAACCTTACGTGGGGGTTCCAAAAA', dtype=np.uint8)
    #  block 0: t 0..5  AAAAA / q 0..5 AAGAA: 4 matches, A/G a transition
    #  then 2 inserted query bases (CC) in front of target base 5
    #  block 1: t 5..9  CCCC  / q 7..11 TTAC: C/T C/T transitions, C/A transversion, C/C match
    #  then target bases 9 and 10 deleted (C, G) and query base 11 (G) inserted: both jump, p = 9
    #  block 2: t 11..15 GGGG / q 12..16 TGGG: G/T transversion, 3 matches
    blk = np.array([(0, 0, 5), (5, 7, 4), (11, 12, 4)], dtype=_ffi.PATH_BLOCK)
    o = PathOracle(T, Q, blk)
    assert o.whole().tolist() == [8, 3, 2, 0, 2, 3, 1, 2]
    w = lambda a, b: o.windows([a], [b])[0].tolist()
    assert w(0, 5) == [4, 1, 0, 0, 0, 0, 0, 0]      # the insertion in front of base 5 is not in [0, 5)
    assert w(5, 6) == [0, 1, 0, 0, 1, 2, 0, 0]      # ... it is in the window that holds base 5, whole
    assert w(5, 9) == [1, 2, 1, 0, 1, 2, 0, 0]
    assert w(9, 10) == [0, 0, 0, 0, 1, 1, 1, 1]     # the deletion run and the insertion at p = 9; one deleted base of two
    assert w(10, 11) == [0, 0, 0, 0, 0, 0, 0, 1]    # the second deleted base: a base, no run
    assert w(10, 40) == [3, 0, 1, 0, 0, 0, 0, 1] and w(15, 40) == [0] * 8 and w(7, 7) == [0] * 8


def test_exhaustive_windows_on_a_small_path(eng, made):
    """Every window [w0, w1) with tstart - 2 <= w0 <= w1 <= tend + 2 of the four-block path, a group each, in one call: every
    edge of the rules — a window that ends on, starts on or lies inside a gap, one base, empty, outside."""
    c = made
    items = []
    for a in c.what['small']:
        t0, t1 = c.oracle[a].t0, c.oracle[a].t1
        assert (t0, t1) == (80, 256)
        items += [(a, 0, w0, w1) for w0 in range(t0 - 2, t1 + 3) for w1 in range(w0, t1 + 3)]
    items = np.array(items, dtype=np.int64)
    items[:, 1] = np.arange(items.shape[0])
    assert items.shape[0] > 10_000
    exp = c.expected(items, items.shape[0])
    # not vacuous, on the restatement's side: both strands differ, every field occurs, the gaps are what the table says
    whole = [c.oracle[a].whole() for a in c.what['small']]
    assert [w[4:].tolist() for w in whole] == [[2, 10, 2, 8]] * 2 and whole[0][:4].tolist() != whole[1][:4].tolist()
    assert all(w[3] >= 1 for w in whole) and (exp.sum(axis=0) > 0).all()
    same(run(eng, c, items, items.shape[0]), exp, 'exhaustive')


def test_word_boundaries(eng, made):
    """200-column blocks starting at every t mod 64 and q mod 64 of MODS, clipped at block start + EDGES on either side"""
    c = made
    items = []
    for a in c.what['mods']:
        t = int(c.blk(a)['t'][0])
        items += [(a, len(items), t + e0, t + e1) for e0 in EDGES for e1 in EDGES if e0 <= e1]
    for a in c.what['mods']:
        assert len(c.blk(a)) == 1
    assert {(int(c.blk(a)['t'][0]) % 64, int(c.blk(a)['q'][0]) % 64) for a in c.what['mods']} == {(x, y) for x in MODS for y in MODS}
    items = np.array(items, dtype=np.int64)
    items[:, 1] = np.arange(items.shape[0])
    same(run(eng, c, items, items.shape[0]), c.expected(items, items.shape[0]), 'word boundaries')


def test_block_search_and_passes(eng, made):
    c = made
    items = []
    for nb in CHAINS:
        for a in c.what['chain %d' % nb]:
            b = c.blk(a)
            assert len(b) == nb
            t, ln = b['t'].astype(np.int64), b['len'].astype(np.int64)
            tend, L = int(t[-1] + ln[-1]), c.L[0]
            for k in (0, 1, 62, 63, 64, 65, 128, 199):
                if k >= nb:
                    continue
                p = int(t[k - 1] + ln[k - 1]) if k else int(t[0])
                for w0 in sorted({max(p - 1, 0), p, int(t[k]), int(t[k] + ln[k] // 2), int(t[k] + ln[k] - 1)}):
                    ends = {w0, w0 + 1, w0 + 100, tend - 1, tend, tend + 5, int(t[min(k + 70, nb - 1)]) + 3}   # one base; over more than 64 blocks
                    items += [(a, 0, w0, w1) for w1 in sorted(ends) if w0 <= w1 <= L]
    for a in c.what['to the end']:
        b = c.blk(a)
        tid = int(c.recs[a]['tid'])
        tend = int(b['t'][-1]) + int(b['len'][-1])
        assert tend == c.L[tid]
        items += [(a, 0, w0, tend) for w0 in (0, int(b['t'][0]), int(b['t'][-1]) - 1, int(b['t'][-1]), tend - 1, tend)]
        items += [(a, 0, tend - 1, tend - 1), (a, 0, max(tend - 5000, 0), tend - 1)]
    items = np.array(items, dtype=np.int64)
    items[:, 1] = np.arange(items.shape[0])
    exp = c.expected(items, items.shape[0])
    assert items.shape[0] > 1000 and (exp.sum(axis=0) > 0).all()
    # windows over more than 64 blocks are among them
    a = c.what['chain 200'][0]
    t = c.blk(a)['t'].astype(np.int64)
    it = items[items[:, 0] == a]
    assert (np.searchsorted(t, it[:, 3]) - np.searchsorted(t, it[:, 2]) > 64).sum() > 10
    same(run(eng, c, items, items.shape[0]), exp, 'block search')


def _partition_items(rng, recs_t0_t1):
    """random partitions of every [tstart, tend): (alignment, group = alignment, consecutive windows)"""
    items = []
    for a, (t0, t1) in enumerate(recs_t0_t1):
        if t1 <= t0:
            continue
        cuts = np.unique(np.r_[t0, rng.integers(t0, t1 + 1, size=int(rng.integers(0, 7))), t1])
        items += [(a, a, int(x), int(y)) for x, y in zip(cuts[:-1], cuts[1:])]
    order = rng.permutation(len(items))
    return np.array(items, dtype=np.int64)[order]


def _against_k9(eng, G, recs, first, blocks, seed, tag):
    """over a partition of [tstart, tend) the eight fields sum to what K9, an independently written kernel, counts for the path"""
    k9 = eng.path_stats(G, None, recs, first, blocks)
    b0, b1 = first[:-1].astype(np.int64), first[1:].astype(np.int64)
    has = b1 > b0
    i0, i1 = np.where(has, b0, 0), np.where(has, b1 - 1, 0)   # an alignment without blocks has no [tstart, tend)
    t0 = np.where(has, blocks['t'][i0], 0).astype(np.int64)
    t1 = np.where(has, blocks['t'][i1].astype(np.int64) + blocks['len'][i1], 0)
    items = _partition_items(np.random.default_rng(seed), list(zip(t0.tolist(), t1.tolist())))
    got = eng.window_stats(G, None, recs, first, blocks, items.astype(np.uint32), recs.size)
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != k9[f].astype(np.uint64))
        assert bad.size == 0, (tag, f, bad[:5], got[f][bad[:5]], k9[f][bad[:5]])
    return items.shape[0], int(got['matches'].sum()), int((got['ins_runs'] + got['del_runs']).sum())


def test_additivity_against_k9_made_up(eng, made):
    c = made
    nitems, matches, runs = _against_k9(eng, c.G, c.recs, c.first, c.blocks, 41, 'made-up')
    assert nitems > 2 * c.recs.size and matches > 50_000 and runs > 2000
    # ... and the restatement agrees with K9 on the whole paths
    k9 = eng.path_stats(c.G, None, c.recs, c.first, c.blocks)
    whole = np.array([o.whole() for o in c.oracle])
    for k, f in enumerate(FIELDS):
        assert (k9[f].astype(np.int64) == whole[:, k]).all(), f


@pytest.mark.parametrize('rule', [0, 1], ids=['box', 'path'])
@pytest.mark.parametrize('which', ['synth', 'tandem'])
def test_additivity_against_k9_engine_paths(eng, which, rule):
    names, seqs = synth_genome(50, 300_000, 3, repeat_frac=0.2, families=5) if which == 'synth' else tandem_genome(3, 2, 60_000)
    G = eng.Genome(names, seqs)
    n = len(names)
    recs, first, blocks = eng.align_pairs(G, None, [(a, b) for a in range(n) for b in range(n)], eng.default_params(anchor_rule=rule), paths=True)
    assert not eng.failed_pairs()
    nitems, matches, runs = _against_k9(eng, G, recs, first, blocks, 42 + rule, (which, rule))
    G.close()
    print(which, rule, recs.size, nitems, matches, runs)
    assert recs.size > 10 and nitems > 2 * recs.size and runs > 30
    assert which == 'tandem' or set(recs['qstrand'].tolist()) == {0, 1}   # the tandem genome's copies all lie on the plus strand


def _layout_call(c):
    """items over every kind of made-up path, a few groups shared by many items, the long blocks whole and in pieces"""
    rng = np.random.default_rng(51)
    items = []
    for a in range(c.recs.size):
        o = c.oracle[a]
        for _ in range(3):
            w0 = int(rng.integers(max(o.t0 - 3, 0), o.t1 + 1))
            items.append((a, int(rng.integers(0, 37)), w0, min(w0 + int(rng.integers(0, 400)), c.L[int(c.recs[a]['tid'])])))
    for a in c.what['long']:
        o = c.oracle[a]
        items += [(a, 37, 0, c.L[int(c.recs[a]['tid'])]), (a, 38, o.t0 + 1, o.t1 - 1), (a, 39, o.t0 + 4321, o.t0 + 4321 + 2500)]
    return np.array(items, dtype=np.int64)


def test_layout_independence(eng, made, monkeypatch):
    """the same call under every split of the windows, with every alignment a slice of its own, and with the items shuffled:
    the same bytes"""
    c = made
    items = _layout_call(c)
    exp = c.expected(items, 41)
    assert exp[40].sum() == 0 and exp[37, :4].sum() >= 2 * (10_000 + 19_000)   # a group without items; the 10 000-column blocks whole
    ref = run(eng, c, items, 41)
    same(ref, exp, 'default')
    for env in ({'MIMEO_WINDOW_STATS_SPLIT_BASES': '64'}, {'MIMEO_WINDOW_STATS_SPLIT_BASES': '1000'}, {'MIMEO_WINDOW_STATS_SPLIT_BASES': '0'},
                {'MIMEO_WINDOW_STATS_SLICE_BLOCKS': '1'}, {'MIMEO_WINDOW_STATS_SLICE_BLOCKS': '70', 'MIMEO_WINDOW_STATS_SPLIT_BASES': '100'},
                {'MIMEO_WINDOW_STATS_STATS': '1'},
                # one job per launch (a workgroup with three idle wavefronts) and three (a partial last workgroup); the pieces of a
                # cut window in different launches; a launch cap that is no number or zero is the default
                {'MIMEO_PATH_LAUNCH_JOBS': '1'}, {'MIMEO_PATH_LAUNCH_JOBS': '3'}, {'MIMEO_WINDOW_STATS_SPLIT_BASES': '64', 'MIMEO_PATH_LAUNCH_JOBS': '3'},
                {'MIMEO_PATH_LAUNCH_JOBS': '0'}, {'MIMEO_PATH_LAUNCH_JOBS': 'abc'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        assert run(eng, c, items, 41).tobytes() == ref.tobytes(), env
        for k in env:
            monkeypatch.delenv(k)
    shuffled = items[np.random.default_rng(52).permutation(items.shape[0])]
    assert run(eng, c, shuffled, 41).tobytes() == ref.tobytes()
    assert run(eng, c, items[::-1], 41).tobytes() == ref.tobytes()
    # the same paths in another order of the records
    from mimeo_amd import formats
    rev = np.arange(c.recs.size)[::-1]
    f2, b2 = formats.select_paths(c.first, c.blocks, rev)
    it2 = items.copy()
    it2[:, 0] = c.recs.size - 1 - items[:, 0]
    assert eng.window_stats(c.G, None, c.recs[rev], f2, b2, it2.astype(np.uint32), 41).tobytes() == ref.tobytes()
    # Q given as a genome of its own, with the query scaffolds in another order
    B = eng.Genome(['w2', 'w0', 'w1'], [c.seqs[2], c.seqs[0], c.seqs[1]])
    r2 = c.recs.copy()
    r2['qid'] = (c.recs['qid'] + 1) % 3
    assert eng.window_stats(c.G, B, r2, c.first, c.blocks, items.astype(np.uint32), 41).tobytes() == ref.tobytes()
    assert eng.window_stats(c.G, c.G, c.recs, c.first, c.blocks, items.astype(np.uint32), 41).tobytes() == ref.tobytes()
    B.close()


def test_64_bit_accumulation(eng, made):
    """one group receives the 10 000-column window 430 000 times: 4.3e9 columns, beyond 2^32, exact.  No single field of that
    group passes 2^32, so a second group receives a scaffold's self diagonal 250 000 times: 5e9 matches in one counter."""
    c = made
    a, d = c.what['long'][0], c.what['diagonal'][0]
    o, od = c.oracle[a], c.oracle[d]
    assert o.t1 - o.t0 == 10_000 and od.t1 - od.t0 == 20_000
    times, times_d = 430_000, 250_000
    items = np.zeros(times + times_d, dtype=_ffi.WINDOW_ITEM)
    items['aln'][:times], items['group'][:times], items['w0'][:times], items['w1'][:times] = a, 1, o.t0, o.t1
    items['aln'][times:], items['group'][times:], items['w0'][times:], items['w1'][times:] = d, 2, 0, c.L[0]
    got = eng.window_stats(c.G, None, c.recs, c.first, c.blocks, items, 4)
    exp = np.zeros((4, 8), dtype=np.int64)
    exp[1], exp[2] = o.whole() * times, od.whole() * times_d
    assert exp[1, :4].sum() == 4_300_000_000 > 2 ** 32 and exp[2, 0] == 19_999 * times_d > 2 ** 32 and exp[2, 3] == times_d
    same(got, exp, '64 bits')


def test_rejected_input(eng, made):
    c = made
    ok = np.array([(0, 0, 80, 256), (1, 1, 100, 100), (5, 2, 0, 20_000)], dtype=np.int64)
    exp = c.expected(ok, 3)

    def bad(row, col, value, match, ngroups=3):
        it = ok.copy()
        it[row, col] = value
        with pytest.raises(RuntimeError, match=match):
            run(eng, c, it, ngroups)

    bad(1, 0, c.recs.size, r'item 1 \(aln %d, .*aln is not a record' % c.recs.size)
    bad(2, 1, 3, r'item 2 \(aln 5, group 3, .*group is not below ngroups')
    bad(0, 1, 0, r'item 0 .*group is not below ngroups', ngroups=0)
    bad(0, 2, 257, r'item 0 \(aln 0, group 0, window \[257, 256\)\): w0 is beyond w1')
    bad(0, 3, c.L[1] + 1, r'item 0 .*w1 is beyond the target scaffold')   # record 0 lies on scaffold 1 of 19 999 bases
    bad(2, 3, 0xFFFFFFFF, r'item 2 .*w1 is beyond the target scaffold')
    # a bad path is refused like mimeo_path_stats refuses it, whatever the items
    blk = c.blocks.copy()
    blk['len'][2] = 0
    with pytest.raises(RuntimeError, match=r'record 0, block 2 .*len is 0'):
        eng.window_stats(c.G, None, c.recs, c.first, blk, ok.astype(np.uint32), 3)
    with pytest.raises(ValueError):
        eng.window_stats(c.G, None, c.recs, c.first[:-1], c.blocks, ok.astype(np.uint32), 3)
    # nothing was launched and nothing is broken: the valid call answers; an empty window (item 1) counted nothing
    got = run(eng, c, ok, 3)
    same(got, exp, 'after the refusals')
    assert exp[1].sum() == 0 and exp[0].sum() > 0
    # nitems == 0: zeros, also without a single record
    none = run(eng, c, np.zeros((0, 4)), 5)
    assert none.dtype == _ffi.WINDOW_STATS and none.size == 5 and not none.tobytes().strip(b'\0')
    none = eng.window_stats(c.G, None, c.recs[:0], c.first[:1], c.blocks[:0], np.zeros((0, 4)), 2)
    assert none.size == 2 and not none.tobytes().strip(b'\0')
    assert run(eng, c, np.zeros((0, 4)), 0).size == 0
    # windows that miss their alignment, and the alignment without blocks
    e = c.what['empty'][0]
    miss = np.array([(0, 0, 0, 80), (0, 1, 256, 19_999), (e, 2, 0, 20_345)], dtype=np.int64)
    assert not run(eng, c, miss, 3).tobytes().strip(b'\0')


# ---- CLI end to end --------------------------------------------------------------------------------------------------------

def _cli(tmp_path, tag, cmd, extra):
    d = tmp_path / tag
    r = subprocess.run([sys.executable, '-m', 'mimeo_amd'] + cmd + ['-d', str(d)] + [str(d / x) if x.endswith(('.tsv', '.paf')) else x for x in extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return d


def _line(rid, seqid, start, end, rows, c):
    m, ts, tv, amb, ir, ib, dr, db = (int(x) for x in c)
    cols, runs, mism, kd = m + ts + tv + amb, ir + dr, ts + tv + amb, '.'
    n = m + ts + tv
    if n:
        a, b = 1.0 - 2.0 * ts / n - tv / n, 1.0 - 2.0 * tv / n
        if a > 0.0 and b > 0.0:
            kd = '%.4f' % (0.0 - 0.5 * math.log(a * math.sqrt(b)))
    return '\t'.join([rid, seqid, str(start), str(end), str(rows), str(cols + db), str(cols), str(m), str(ts), str(tv), str(amb), str(ir), str(ib), str(dr),
                      str(db), '%.4f' % (m / cols) if cols else '.', '%.4f' % ((mism + runs) / (m + mism + runs)) if m + mism + runs else '.', kd])


def _restate_tsv(eng, gff, A, B, min_cov_rows=None, strict=False):
    """The --regionStats file from the GFF3 rows and the engine's alignments: (names, seqs) of A and of B (None: a self job)."""
    from mimeo_amd import formats
    (an, aseq), (bn, bseq) = A, B if B is not None else A
    GA = eng.Genome(an, aseq)
    GB = eng.Genome(bn, bseq) if B is not None else None
    recs, first, blocks = eng.align_pairs(GA, GB, [(a, b) for a in range(len(an)) for b in range(len(bn))], eng.default_params(hspthresh=3000), paths=True)
    GA.close()
    if GB is not None:
        GB.close()
    rows = []
    formats.tab_blocks(recs, an, bn, 100, 60, rows=rows)
    rc = {}
    out, dropped, clipped = ['#ID\tseqid\tstart\tend\trows\tcovered\tcolumns\t' + '\t'.join(FIELDS) + '\tidentity\tde\tkd'], 0, 0
    kept = []
    for i in rows[0].tolist():
        r, b = recs[i], blocks[int(first[i]):int(first[i + 1])]
        if B is None and int(r['tid']) == int(r['qid']) and not int(r['qstrand']) and len(b) == 1 and int(b['t'][0]) == int(b['q'][0]):
            dropped += 1   # a scaffold against itself
            continue
        qid = int(r['qid'])
        if int(r['qstrand']) and qid not in rc:
            rc[qid] = revcomp(bseq[qid])
        kept.append((r, PathOracle(aseq[int(r['tid'])], rc[qid] if int(r['qstrand']) else bseq[qid], b)))
    for g in gff.splitlines():
        if g.startswith('#'):
            continue
        f = g.split('\t')
        tid, start, end, intra = an.index(f[0]), int(f[3]), int(f[4]), f[2].endswith('_intra')
        c, n = np.zeros(8, dtype=np.int64), 0
        for r, o in kept:
            if int(r['tid']) != tid or int(r['tend']) <= start or int(r['tstart']) >= end:
                continue
            if strict and (int(r['tid']) == int(r['qid'])) != intra:
                continue
            assert (o.t0, o.t1) == (int(r['tstart']), int(r['tend']))
            c += o.windows([start], [end])[0]
            n += 1
            clipped += int(r['tstart']) < start or int(r['tend']) > end
        out.append(_line(f[8][3:], f[0], start, end, n, c))
    return out, dropped, clipped


@pytest.fixture(scope='module')
def cli_genome(tmp_path_factory):
    names, seqs = synth_genome(50, 300_000, 3, repeat_frac=0.2, families=5)
    fa = str(tmp_path_factory.mktemp('ws') / 'a.fa')
    write_fasta(fa, names, seqs)
    return names, seqs, fa


def _same_files(d, plain, files):
    for f in files:
        assert (d / f).read_bytes() == (plain / f).read_bytes(), f


def test_cli_self_region_stats(eng, cli_genome, tmp_path):
    names, seqs, fa = cli_genome
    cmd = ['self', '--afasta', fa]
    plain = _cli(tmp_path, 'plain', cmd, ['--paf', 'a.paf', '--divergence'])
    alone = _cli(tmp_path, 'alone', cmd, ['--regionStats', 'r.tsv'])
    both = _cli(tmp_path, 'both', cmd, ['--regionStats', 'r.tsv', '--paf', 'a.paf', '--divergence'])
    outs = ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3')
    _same_files(alone, plain, outs)
    _same_files(both, plain, outs + ('a.paf',))
    assert sorted(os.listdir(both)) == sorted(os.listdir(plain) + ['r.tsv']) and not (alone / 'a.paf').exists()
    gff = (plain / outs[1]).read_text()
    exp, dropped, clipped = _restate_tsv(eng, gff, (names, seqs), None)
    assert len(exp) > 4 and dropped == 3 and clipped > 3   # regions; the three self diagonals; alignments that run past a region's end
    assert (alone / 'r.tsv').read_text().splitlines() == exp
    assert (both / 'r.tsv').read_bytes() == (alone / 'r.tsv').read_bytes()
    assert any(l.split('\t')[11] != '0' for l in exp[1:]) and all(int(l.split('\t')[4]) >= 1 for l in exp[1:])


def test_cli_strict_self_region_stats(eng, cli_genome, tmp_path):
    names, seqs, fa = cli_genome
    cmd = ['self', '--afasta', fa, '--strictSelf', '--minCov', '2', '--intraCov', '2']
    plain = _cli(tmp_path, 'plain', cmd, [])
    stats = _cli(tmp_path, 'stats', cmd, ['--regionStats', 'r.tsv'])
    outs = ('mimeo_alignment.tab', 'mimeo_alignment.tab_intra.tab', 'mimeo-self_repeats.gff3')
    _same_files(stats, plain, outs)
    gff = (plain / outs[2]).read_text()
    exp, dropped, _ = _restate_tsv(eng, gff, (names, seqs), None, strict=True)
    ids = [l.split('\t')[0] for l in exp[1:]]
    assert len(set(ids)) < len(ids) and ids.count('Self_Repeat_00001') == 2   # the intra block's IDs restart
    assert (stats / 'r.tsv').read_text().splitlines() == exp


def test_cli_x_region_stats(eng, tmp_path):
    fams = make_families(7, 5, cons_len=(300, 3000))
    an, aseq = synth_genome(51, 300_000, 3, repeat_frac=0.2, shared_families=fams, prefix='a')
    bn, bseq = synth_genome(52, 300_000, 3, repeat_frac=0.2, shared_families=fams, prefix='b')
    fa, fb = str(tmp_path / 'a.fa'), str(tmp_path / 'b.fa')
    write_fasta(fa, an, aseq)
    write_fasta(fb, bn, bseq)
    cmd = ['x', '--afasta', fa, '--bfasta', fb, '--minCov', '3']
    plain = _cli(tmp_path, 'plain', cmd, ['--paf', 'a.paf', '--divergence'])
    both = _cli(tmp_path, 'both', cmd, ['--regionStats', 'r.tsv', '--paf', 'a.paf', '--divergence'])
    alone = _cli(tmp_path, 'alone', cmd, ['--regionStats', 'r.tsv'])
    outs = ('mimeo_alignment.tab', 'mimeo_B_in_A.gff3')
    _same_files(alone, plain, outs)
    _same_files(both, plain, outs + ('a.paf',))
    exp, dropped, clipped = _restate_tsv(eng, (plain / outs[1]).read_text(), (an, aseq), (bn, bseq))
    assert len(exp) > 4 and dropped == 0
    assert (alone / 'r.tsv').read_text().splitlines() == exp
    assert (both / 'r.tsv').read_bytes() == (alone / 'r.tsv').read_bytes()
