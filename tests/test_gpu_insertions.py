"""Insertion columns of the pileup (mimeo_path_insertions, kernels K14; engine.insertions; `mimeo self --consensus
--consensusInsertions`) against a plain numpy restatement of "pileup v2, insertion columns" (include/mimeo_hip.h), written here
from the header's rules alone: per item and site the block whose gap starts at the site, the inserted query letters left-aligned
in the site's columns, the four sums of the site; the call from the counts of a column and the site's voters.  Equality is
exact, counter by counter and byte by byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi, formats
from mimeo_amd.synth import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_FIELDS = ('runs', 'bases', 'longer', 'max_len')
COL_FIELDS = ('a', 'c', 'g', 't', 'n')
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
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

def site_rows(sites):
    """sites as an (n, 4) int64 array of (window, x, ncols, voters), from rows or from _ffi.INSERT_SITE"""
    a = np.asarray(sites)
    if a.dtype == _ffi.INSERT_SITE:
        a = np.stack([a[f].astype(np.int64) for f in _ffi.INSERT_SITE.names], axis=1) if a.size else np.zeros((0, 4), dtype=np.int64)
    return np.asarray(a, dtype=np.int64).reshape(-1, 4)


def restate(seqs, recs, first, blocks, items, sites):
    """(res (nsites, 4) in the order of mimeo_insert_result, icols (nicols, 5) in the order of mimeo_insert_column).  seqs: the
    scaffolds as uint8 letters; items: rows of (aln, window, w0, w1); sites: rows of (window, x, ncols, voters)."""
    st = site_rows(sites)
    icol_first = np.concatenate([[0], np.cumsum(st[:, 2])])
    res = np.zeros((st.shape[0], 4), dtype=np.int64)
    icols = np.zeros((int(icol_first[-1]), 5), dtype=np.int64)
    rc = {}
    for a, g, w0, w1 in np.asarray(items, dtype=np.int64).reshape(-1, 4).tolist():
        qid, strand = int(recs[a]['qid']), int(recs[a]['qstrand'])
        if strand and qid not in rc:
            rc[qid] = revcomp(seqs[qid])
        Q = rc[qid] if strand else seqs[qid]
        blk = blocks[int(first[a]):int(first[a + 1])].tolist()
        for s, (sw, x, ncols, _) in enumerate(st.tolist()):
            if sw != g or not w0 <= x < w1:
                continue
            for k in range(1, len(blk)):
                p, qs = blk[k - 1][0] + blk[k - 1][2], blk[k - 1][1] + blk[k - 1][2]
                dq = blk[k][1] - qs
                if p == x and dq > 0:
                    res[s, 0] += 1
                    res[s, 1] += dq
                    res[s, 2] += dq > ncols
                    res[s, 3] = max(res[s, 3], dq)
                    m = min(dq, ncols)
                    np.add.at(icols, (int(icol_first[s]) + np.arange(m), CODE[Q[qs:qs + m]]), 1)
    return res, icols


def restate_call(sites, icols):
    """the call byte of every insertion column, from its five counts and the site's voters"""
    out = []
    at = 0
    for _, _, ncols, voters in site_rows(sites).tolist():
        for _ in range(ncols):
            a, c, g, t, n = (int(v) for v in icols[at])
            at += 1
            top = max(a, c, g, t)
            total = a + c + g + t + n
            vg = voters - total if voters > total else 0
            if top > vg:
                out.append(b'ACGT'[[a, c, g, t].index(top)])
            elif top == 0 and n > vg:
                out.append(ord('N'))
            else:
                out.append(ord('-'))
    return np.array(out, dtype=np.uint8)


def restate_pileup_ins(recs, first, blocks, windows, items):
    """ins_runs, ins_bases and the depth a + c + g + t + n + del of "pileup v1" per column, as far as the sites need them"""
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 3)
    col_first = np.concatenate([[0], np.cumsum(win[:, 2] - win[:, 1])])
    runs, bases, depth = (np.zeros(int(col_first[-1]), dtype=np.int64) for _ in range(3))
    for a, g, w0, w1 in np.asarray(items, dtype=np.int64).reshape(-1, 4).tolist():
        blk = blocks[int(first[a]):int(first[a + 1])].tolist()
        base = int(col_first[g]) - int(win[g, 1])
        if blk:
            lo, hi = max(w0, blk[0][0]), min(w1, blk[-1][0] + blk[-1][2])
            if hi > lo:
                depth[base + lo:base + hi] += 1
        for k in range(1, len(blk)):
            p, dq = blk[k - 1][0] + blk[k - 1][2], blk[k][1] - (blk[k - 1][1] + blk[k - 1][2])
            if dq > 0 and w0 <= p < w1:
                runs[base + p] += 1
                bases[base + p] += dq
    return runs, bases, depth


def test_restatement_on_paper():
    """The restatement itself, on the 30-base path of tests/test_gpu_pileup.py, small enough to count by hand"""
    T = np.frombuffer(b'AAAAACCCCCGGGGGTTTTTAAAAANNNNN', dtype=np.uint8)
    Q = np.frombuffer(b'AAGAACCTTACGTGNGGGTTCCAAAAA', dtype=np.uint8)
    #  block 0: t 0..5 over q 0..5; the 2 query bases CC inserted in front of target base 5
    #  block 1: t 5..9 over q 7..11; then target bases 9 and 10 deleted and query base 11, a G, inserted: both jump, p = 9
    #  block 2: t 11..15 over q 12..16
    recs = np.zeros(1, dtype=_ffi.ALIGNMENT)
    recs['qid'] = 1
    blk = np.array([(0, 0, 5), (5, 7, 4), (11, 12, 4)], dtype=_ffi.PATH_BLOCK)
    first = np.array([0, 3], dtype=np.uint64)
    windows, items = [(0, 0, 20)], [(0, 0, 0, 20)] * 2
    # the record twice: depth 2, 2 runs, 2 * 2 > 2 + 1 — the sites are 5 and 9 (once it would be 2 > 2: none)
    runs, bases, depth = restate_pileup_ins(recs, first, blk, windows, items)
    cols = np.zeros(20, dtype=_ffi.PILEUP_COLUMN)
    cols['ins_runs'], cols['ins_bases'], cols['a'] = runs, bases, depth
    win = np.zeros(1, dtype=_ffi.PILEUP_WINDOW)
    win[0] = (0, 0, 20)
    sites = formats.insertion_sites(win, cols)
    assert sites.tolist() == [(0, 5, 3, 3), (0, 9, 1, 3)]   # ncols = 4 - 2 + 1 and 2 - 2 + 1
    cols['ins_runs'], cols['ins_bases'] = runs // 2, bases // 2
    cols['a'] = depth // 2
    assert formats.insertion_sites(win, cols).size == 0
    res, icols = restate([T, Q], recs, first, blk, items, sites)
    assert res.tolist() == [[2, 4, 0, 2], [2, 2, 0, 1]]
    assert icols.tolist() == [[0, 2, 0, 0, 0], [0, 2, 0, 0, 0], [0, 0, 0, 0, 0], [0, 0, 2, 0, 0]]
    assert restate_call(sites, icols).tobytes() == b'CC-G'   # 2 against the own copy's gap vote; nobody has a third base
    # a site inside the deletion (10), at the first block's start (0), inside a block (7), off the alignment (17): nothing
    res, icols = restate([T, Q], recs, first, blk, items, [(0, 0, 1, 3), (0, 7, 1, 3), (0, 10, 1, 3), (0, 17, 1, 3)])
    assert not res.any() and not icols.any()
    # an item that ends at the site does not hold it, one that starts there does; one column for two bases: truncated
    res, icols = restate([T, Q], recs, first, blk, [(0, 0, 0, 5), (0, 0, 5, 9)], [(0, 5, 1, 1), (0, 9, 1, 1)])
    assert res.tolist() == [[1, 2, 1, 2], [0, 0, 0, 0]] and icols.tolist() == [[0, 1, 0, 0, 0], [0, 0, 0, 0, 0]]
    assert restate_call([(0, 5, 1, 1), (0, 9, 1, 1)], icols).tobytes() == b'C-'


# ---- made-up paths ---------------------------------------------------------------------------------------------------------

L = (6000, 5000, 4000)
PATH4 = [(500, 300, 100), (600, 405, 100), (720, 505, 80), (830, 600, 60)]   # an insertion of 5 at 600, a deletion [700, 720), both at 800: 15 / 30
DQS = (1, 63, 64, 65, 129)
MANY = 150   # blocks of the long record: 149 insertions of 2 bases, ten target bases apart


def _genome():
    rng = np.random.default_rng(140)
    s = [ACGT[rng.integers(0, 4, n)].copy() for n in L]
    s[1][402] = ord('N')           # N inside PATH4's inserted run [400, 405) on the plus strand ...
    s[1][4596:4598] = ord('n')     # ... and on the minus strand (reverse-complement bases 402 and 403)
    s[1][1500:1503] = ord('R')     # an IUPAC code is an N to the engine: inside the run of 129 on the plus strand
    s[2][1500:1520] += 32          # soft-masked
    s[1][4900:4905] = np.frombuffer(b'ACGTN', dtype=np.uint8)   # the designed piles of test_call_rule
    return ['p0', 'p1', 'p2'], s


def dq_path():
    """blocks of 50 on scaffold 2 from 100 on, over scaffold 1 from 1000 on, with DQS bases inserted between them"""
    blk, q = [(100, 1000, 50)], 1050
    for k, dq in enumerate(DQS, 1):
        q += dq
        blk.append((100 + 50 * k, q, 50))
        q += 50
    return blk


class Case:
    def __init__(self):
        self.names, self.seqs = _genome()
        self.recs, self.first, self.blocks = [], [0], []
        self.windows, self.items, self.sites, self.what = [], [], [], {}

    def add(self, tid, qid, strand, blk):
        t_end = q_end = 0
        for t, q, ln in blk:   # the contract of mimeo_path_block, so that a slip in a table is not taken for a kernel's
            assert ln >= 1 and t >= t_end and q >= q_end and t + ln <= L[tid] and q + ln <= L[qid], (t, q, ln)
            t_end, q_end = t + ln, q + ln
        self.recs.append((tid, qid, strand))
        self.blocks.extend(blk)
        self.first.append(len(self.blocks))
        return len(self.recs) - 1

    def window(self, what, tid, start, end, items, sites):
        """a window, its items (aln, w0, w1) and its sites (x, ncols, voters), x rising; `what` names the case of the issue's list"""
        g = len(self.windows)
        self.windows.append((tid, start, end))
        for a, w0, w1 in items:
            assert self.recs[a][0] == tid and start <= w0 <= w1 <= end
            self.items.append((a, g, w0, w1))
        for x, ncols, voters in sites:
            assert start <= x < end and 1 <= ncols <= 1024
            self.what.setdefault(what, []).append(len(self.sites))
            self.sites.append((g, x, ncols, voters))
        return g

    def finish(self):
        r = np.zeros(len(self.recs), dtype=_ffi.ALIGNMENT)
        r['tid'], r['qid'], r['qstrand'] = [x[0] for x in self.recs], [x[1] for x in self.recs], [x[2] for x in self.recs]
        self.recs, self.first, self.blocks = r, np.array(self.first, dtype=np.uint64), np.array(self.blocks, dtype=_ffi.PATH_BLOCK)
        self.windows = np.array(self.windows, dtype=np.int64)
        self.items = np.array(self.items, dtype=np.int64)
        self.sites = np.array(self.sites, dtype=np.int64)
        self.icol_first = np.concatenate([[0], np.cumsum(self.sites[:, 2])])
        return self

    def cols_of(self, icols, s):
        return icols[int(self.icol_first[s]):int(self.icol_first[s + 1])]


def made_case():
    c = Case()
    rng = np.random.default_rng(141)
    plus, minus = c.add(0, 1, 0, PATH4), c.add(0, 1, 1, PATH4)
    both = lambda s, e: [(plus, s, e), (minus, s, e)]
    c.window('an insertion at p_k == w0, counted', 0, 600, 650, both(600, 650), [(600, 5, 3)])
    c.window('an insertion at p_k == w1, not counted', 0, 560, 700, both(560, 600), [(600, 5, 3)])
    # 500: the record's first block start; 700: the junction in front of the deletion, dq == 0; 710: inside the deletion; 650:
    # inside a block; 950: off the alignment
    c.window('sites that get nothing', 0, 400, 1000, both(400, 1000), [(500, 2, 3), (650, 1, 3), (700, 3, 3), (710, 4, 3), (950, 1, 3)])
    c.window('a both-jump gap', 0, 790, 840, both(790, 840), [(800, 15, 3)])
    c.window('N inside an inserted run', 0, 520, 720, both(520, 720), [(600, 5, 2)])
    # dq of 1, 63, 64, 65 and 129, ncols == dq, on both strands; and in a second window (the same columns again, sites of its
    # own) ncols > dq (64 in 70 columns: the trailing six are zero) and dq > ncols (129 in 100: truncated)
    dq = dq_path()
    dplus, dminus = c.add(2, 1, 0, dq), c.add(2, 1, 1, dq)
    c.window('dq of 1, 63, 64, 65 and 129', 2, 50, 500, [(dplus, 50, 500), (dminus, 50, 500)], [(100 + 50 * k, d, 3) for k, d in enumerate(DQS, 1)])
    c.window('ncols > dq', 2, 50, 500, [(dplus, 50, 500), (dminus, 50, 500)], [(250, 70, 3)])
    c.window('dq > ncols', 2, 50, 500, [(dplus, 60, 450)], [(350, 100, 2)])
    # a run of 70 bases from every query start mod 32, on both strands: 64 records of two blocks of 20, 40 target bases apart, a
    # site each with 70 columns — 4480 columns in one window: 14 sites fill a tile of 1024 to 980, so the sites straddle tile ends
    recs = []
    for k in range(64):
        t, q = 1000 + 40 * k, 1600 + 97 * (k // 2) - 20   # the run starts at q + 20 = 1600 + 97 (k // 2): every residue mod 32
        recs.append((c.add(2, 1, k & 1, [(t, q, 20), (t + 20, q + 90, 20)]), t))
    c.window('a run from every residue mod 32', 2, 1000, 3600, [(a, 1000, 3600) for a, _ in recs], [(t + 20, 70, 1) for _, t in recs])
    # a record without blocks
    e = c.add(1, 2, 0, [])
    c.window('a record without blocks', 1, 100, 300, [(e, 100, 300)], [(200, 3, 1)])
    # more than 64 blocks and more than 64 sites under one item: the lanes take a second and a third pass.  Every junction a site,
    # and between them sites inside the blocks, which get nothing
    long_blk = [(100 + 10 * k, 100 + 12 * k, 10) for k in range(MANY)]
    lng = c.add(1, 2, 0, long_blk)
    c.window('more than 64 sites under one item', 1, 50, 1700, [(lng, 50, 1700), (lng, 400, 1000)],
             sorted([(100 + 10 * k, 2, 2) for k in range(1, MANY)] + [(105 + 50 * k, 1, 2) for k in range(30)]))
    # 300 items on one site, of both strands: most hold base 600, some start behind it
    c.window('300 items on one site', 0, 480, 900, [((plus, minus)[k & 1], int(rng.integers(480, 620)), int(rng.integers(620, 901))) for k in range(300)],
             [(600, 5, 301), (800, 15, 301)])
    # sites whose ncols straddle a site-tile boundary: 1000 + 24 columns fill a tile exactly, the next site has 1024 of its own
    c.window('ncols at a tile boundary', 0, 400, 1000, both(400, 1000), [(600, 1000, 3), (700, 24, 3), (800, 1024, 3), (830, 1, 3)])
    # overlapping and repeated windows, each with sites of its own; one record in two windows
    c.window('overlapping windows', 0, 550, 650, [(plus, 550, 650)], [(600, 6, 1)])
    c.window('overlapping windows', 0, 600, 810, [(plus, 600, 700), (minus, 650, 810), (minus, 600, 650)], [(600, 4, 9), (800, 20, 0)])
    c.window('overlapping windows', 0, 550, 650, [(minus, 550, 650)], [(600, 5, 2)])
    # a window with a site that nobody names
    c.window('no item', 1, 4890, 4910, [], [(4900, 2, 0)])
    return c.finish()


LIST = ('an insertion at p_k == w0, counted', 'an insertion at p_k == w1, not counted', 'sites that get nothing', 'a both-jump gap', 'N inside an inserted run',
        'dq of 1, 63, 64, 65 and 129', 'ncols > dq', 'dq > ncols', 'a run from every residue mod 32', 'a record without blocks',
        'more than 64 sites under one item', '300 items on one site', 'ncols at a tile boundary', 'overlapping windows', 'no item')


@pytest.fixture(scope='module')
def made(eng):
    c = made_case()
    c.exp_res, c.exp_cols = restate(c.seqs, c.recs, c.first, c.blocks, c.items, c.sites)   # once, shared, and left as it is
    c.exp_res.setflags(write=False)
    c.exp_cols.setflags(write=False)
    c.exp_call = restate_call(c.sites, c.exp_cols)
    c.G = eng.Genome(c.names, c.seqs)
    c.res, c.icols, c.icall = eng.insertions(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites)
    yield c
    c.G.close()


def same(got, exp, dtype, fields, tag):
    assert got.dtype == dtype and got.shape == (exp.shape[0],), tag
    for k, f in enumerate(fields):
        bad = np.flatnonzero(got[f].astype(np.int64) != exp[:, k])
        assert bad.size == 0, (tag, f, bad[:5], got[f][bad[:5]], exp[bad[:5], k])


def test_made_up_paths_against_the_restatement(made):
    c = made
    assert set(LIST) == set(c.what)
    same(c.res, c.exp_res, _ffi.INSERT_RESULT, RES_FIELDS, 'made-up paths: results')
    same(c.icols, c.exp_cols, _ffi.INSERT_COLUMN, COL_FIELDS, 'made-up paths: columns')
    assert c.icall.dtype == np.uint8 and c.icall.tobytes() == c.exp_call.tobytes()
    # not vacuous: every counter occurs, every byte is called
    assert (c.exp_res.sum(axis=0) > 0).all() and (c.exp_cols.sum(axis=0) > 0).all() and set(c.exp_call.tobytes()) == set(b'ACGTN-')
    res = lambda what, k=0: c.exp_res[c.what[what][k]].tolist()
    cols = lambda what, k=0: c.cols_of(c.exp_cols, c.what[what][k])
    call = lambda what, k=0: c.cols_of(c.exp_call, c.what[what][k]).tobytes()
    # the list, item by item, on the restatement's side: each case is what its name says
    assert res('an insertion at p_k == w0, counted') == [2, 10, 0, 5] and res('an insertion at p_k == w1, not counted') == [0, 0, 0, 0]
    assert call('an insertion at p_k == w1, not counted') == b'-----'
    assert [res('sites that get nothing', k) for k in range(5)] == [[0] * 4] * 5 and sum(cols('sites that get nothing', k).sum() for k in range(5)) == 0
    assert res('a both-jump gap') == [2, 30, 0, 15] and cols('a both-jump gap').sum(axis=1).tolist() == [2] * 15
    n_run = cols('N inside an inserted run')
    assert n_run[:, 4].tolist() == [0, 0, 2, 1, 0] and call('N inside an inserted run')[2:3] == b'N'   # plus: base 402; minus: 402 and 403.  n 2 > vg 0
    assert [res('dq of 1, 63, 64, 65 and 129', k) for k in range(5)] == [[2, 2 * d, 0, d] for d in DQS]
    assert all(cols('dq of 1, 63, 64, 65 and 129', k).sum(axis=1).tolist() == [2] * d for k, d in enumerate(DQS))
    assert cols('dq of 1, 63, 64, 65 and 129', 4)[:, 4].sum() >= 3   # the IUPAC codes inside the run of 129
    wide = cols('ncols > dq')
    assert res('ncols > dq') == [2, 128, 0, 64] and wide.sum(axis=1).tolist() == [2] * 64 + [0] * 6 and call('ncols > dq')[64:] == b'------'
    assert res('dq > ncols') == [1, 129, 1, 129] and cols('dq > ncols').sum(axis=1).tolist() == [1] * 100
    starts = [int(c.blocks[int(c.first[a])]['q']) + 20 for a in range(4, 68)]
    assert {q % 32 for q in starts[0::2]} == set(range(32)) == {q % 32 for q in starts[1::2]} and len(c.what['a run from every residue mod 32']) == 64
    assert all(res('a run from every residue mod 32', k) == [1, 70, 0, 70] for k in range(64))
    assert res('a record without blocks') == [0] * 4 and res('no item') == [0] * 4 and call('no item') == b'--'
    many = c.what['more than 64 sites under one item']
    got = [c.exp_res[s].tolist() for s in many]
    at_junction = [int(c.sites[s][1]) % 10 == 0 for s in many]
    assert len(many) == MANY - 1 + 30 and sum(at_junction) == MANY - 1 > 128
    # the second item [400, 1000) holds the junctions 400 .. 990 once more
    assert all(g == ([2 if 400 <= int(c.sites[s][1]) < 1000 else 1] * 1 + [4 if 400 <= int(c.sites[s][1]) < 1000 else 2, 0, 2] if j else [0] * 4)
               for g, j, s in zip(got, at_junction, many))
    crowd = res('300 items on one site')
    assert 200 < crowd[0] < 300 and crowd[1] == 5 * crowd[0] and 0 < res('300 items on one site', 1)[0] < 300
    assert sum(1 for it in c.items if it[1] == c.sites[c.what['300 items on one site'][0]][0]) == 300
    edge = c.what['ncols at a tile boundary']
    assert [int(c.sites[s][2]) for s in edge] == [1000, 24, 1024, 1] and res('ncols at a tile boundary') == [2, 10, 0, 5]
    assert cols('ncols at a tile boundary').sum() == 10 and cols('ncols at a tile boundary', 2).sum() == 30 and cols('ncols at a tile boundary', 3).sum() == 0
    assert [res('overlapping windows', k) for k in range(4)] == [[1, 5, 0, 5], [2, 10, 2, 5], [1, 15, 0, 15], [1, 5, 0, 5]]
    # what a caller may rely on: a column's total is the number of runs with dq > j, so it does not increase with j; where no
    # run was longer than the columns, the totals sum to `bases`
    tot = c.exp_cols.sum(axis=1)
    for s in range(c.sites.shape[0]):
        t = c.cols_of(tot, s)
        assert (np.diff(t) <= 0).all() and (t[0] if t.size else 0) == c.exp_res[s, 0]
        assert c.exp_res[s, 2] > 0 or t.sum() == c.exp_res[s, 1]


CHILD = '''
import sys
import numpy as np
from mimeo_amd import engine
engine.init(0)
z = np.load(sys.argv[1])
G = engine.Genome(['p0', 'p1', 'p2'], [z['s0'], z['s1'], z['s2']])
args = (G, None, z['recs'], z['first'], z['blocks'], z['windows'], z['items'], z['sites'])
res, icols, icall = engine.insertions(*args)
for k in range(3):   # each output alone, the other two NULL
    only = engine.insertions(*args, results=k == 0, counts=k == 1, call=k == 2)
    assert [o is None for o in only] == [j != k for j in range(3)] and only[k].tobytes() == (res, icols, icall)[k].tobytes()
assert engine.insertions(*args, results=False, counts=False, call=False) == (None, None, None)
np.savez(sys.argv[2], res=res, icols=icols, icall=icall)
'''
SETTINGS = ({}, {'MIMEO_INSERT_JOB_ITEMS': '7'}, {'MIMEO_INSERT_SLICE_BLOCKS': '1'}, {'MIMEO_INSERT_COLUMNS': '1500'}, {'MIMEO_PATH_LAUNCH_JOBS': '3'})


def test_every_setting_gives_the_same_bytes(made, tmp_path):
    """the whole case under the defaults, 7 entries per job, every alignment a slice of its own, batches of 1500 columns and three
    jobs per launch, each in a fresh child process: the bytes of this process's call"""
    c = made
    np.savez(tmp_path / 'in.npz', s0=c.seqs[0], s1=c.seqs[1], s2=c.seqs[2], recs=c.recs, first=c.first, blocks=c.blocks, windows=c.windows, items=c.items,
             sites=c.sites)
    (tmp_path / 'child.py').write_text(CHILD)
    base = dict(os.environ, MIMEO_INSERT_STATS='1', PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get('PYTHONPATH')) if p))
    for e in SETTINGS:
        for name in e:
            base.pop(name, None)
    procs = [subprocess.Popen([sys.executable, str(tmp_path / 'child.py'), str(tmp_path / 'in.npz'), str(tmp_path / ('out%d.npz' % k))], cwd=ROOT,
                              env=dict(base, **e), stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True) for k, e in enumerate(SETTINGS)]
    said = []
    for k, p in enumerate(procs):
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, (SETTINGS[k], out[-2000:], err[-3000:])
        got = np.load(tmp_path / ('out%d.npz' % k))
        assert got['res'].tobytes() == c.res.tobytes() and got['icols'].tobytes() == c.icols.tobytes() and got['icall'].tobytes() == c.icall.tobytes(), SETTINGS[k]
        lines = [l for l in err.splitlines() if l.startswith('[k14]')]
        assert len(lines) == 4 and '%d items' % c.items.shape[0] in lines[0] and 'kernels' in lines[0], err   # the call where all three are NULL does nothing
        m = re.search(r'(\d+) items, (\d+) sites, (\d+) columns, (\d+) tiles, (\d+) jobs, slices (\d+) of (\d+), batches (\d+), launches (\d+), kernels', lines[0])
        assert m, lines[0]
        said.append(dict(zip(('items', 'sites', 'columns', 'tiles', 'jobs', 'slices', 'of', 'batches', 'launches'), (int(x) for x in m.groups()))))
    # the statistics line says what each setting did
    plain, jobs7, slice1, cols1500, launch3 = said
    assert plain['sites'] == c.sites.shape[0] and plain['columns'] == int(c.icol_first[-1]) and plain['tiles'] >= 10
    assert plain['batches'] == 1 and plain['slices'] == 1 and cols1500['batches'] >= 3 and slice1['slices'] > 60
    assert jobs7['jobs'] >= plain['jobs'] + 20 and launch3['launches'] >= plain['jobs'] // 3
    assert plain['tiles'] == cols1500['tiles'] == slice1['tiles']


def test_second_witness_k13(eng, made):
    """runs and bases of every site are ins_runs and ins_bases of K13, an existing kernel, at the site's column for the same items"""
    c = made
    cols, _ = eng.pileup(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, call=False)
    col_first = np.concatenate([[0], np.cumsum(c.windows[:, 2] - c.windows[:, 1])])
    at = col_first[c.sites[:, 0]] + c.sites[:, 1] - c.windows[c.sites[:, 0], 1]
    assert (c.res['runs'] == cols['ins_runs'][at]).all() and (c.res['bases'] == cols['ins_bases'][at]).all()
    assert int(c.res['runs'].sum()) > 400 and int((c.res['runs'] == 0).sum()) >= 30
    tot = sum(c.icols[f].astype(np.int64) for f in COL_FIELDS)
    for s in np.flatnonzero(c.res['longer'] == 0).tolist():
        assert int(c.cols_of(tot, s).sum()) == int(c.res['bases'][s])
    assert int((c.res['longer'] > 0).sum()) >= 2
    # and formats.insertion_sites, from K13's counts, asks for columns enough: no run of a site it picks is longer than its ncols
    sites = formats.insertion_sites(np.array([tuple(w) for w in c.windows.tolist()], dtype=_ffi.PILEUP_WINDOW), cols)
    assert sites.size > 50
    res, _, _ = eng.insertions(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, sites, counts=False, call=False)
    assert not res['longer'].any() and (res['runs'] > 0).all() and (res['max_len'] <= sites['ncols']).all()


def test_call_rule(eng, made):
    """designed one-column piles on scaffold 2 [3500, 3540): runs of one base, the letters A C G T N at scaffold 1 [4900, 4905)"""
    c = made
    q = {b: 4900 + k for k, b in enumerate('ACGTN')}
    recs, first, blocks, items, sites, want = [], [0], [], [], [], []

    def pile(x, letters, voters, byte):
        for b in letters:   # a record that inserts the one base b in front of target base x
            blocks.extend([(x - 1, q[b] - 1, 1), (x, q[b] + 1, 1)])
            first.append(len(blocks))
            items.append((len(recs), 0, 3500, 3540))
            recs.append((2, 1, 0))
        sites.append((0, x, 1, voters))
        want.append(byte)

    pile(3502, 'AA', 4, '-')        # top 2 == vg 2: a tie goes to the gap
    pile(3504, 'AA', 3, 'A')        # top 2 == vg 1 + 1
    pile(3506, 'CA', 0, 'A')        # ties between letters go in the order A, C, G, T
    pile(3508, 'TG', 0, 'G')
    pile(3510, 'TC', 0, 'C')
    pile(3512, 'TTGGCC', 6, 'C')    # top 2 > vg 0
    pile(3514, 'NN', 3, 'N')        # top 0 and n 2 > vg 1
    pile(3516, 'NN', 4, '-')        # top 0 and n 2 == vg 2
    pile(3518, 'ANN', 0, 'A')       # a letter beats any number of N
    pile(3520, 'ANN', 4, '-')       # top 1 == vg 1, and top != 0: no N either
    pile(3522, 'AC', 1, 'A')        # voters < total: vg = 0
    pile(3524, 'G', 0, 'G')         # voters == 0
    pile(3526, '', 0, '-')          # voters == 0 and nobody inserts: 0 > 0 is false
    pile(3528, 'T', 2, '-')         # 1 against the gap vote of 1
    pile(3530, 'T', 0xFFFFFFFF, '-')
    r = np.zeros(len(recs), dtype=_ffi.ALIGNMENT)
    r['tid'], r['qid'], r['qstrand'] = [x[0] for x in recs], [x[1] for x in recs], [x[2] for x in recs]
    first, blocks = np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK)
    res, icols, icall = eng.insertions(c.G, None, r, first, blocks, [(2, 3500, 3540)], items, sites)
    assert icall.tobytes() == ''.join(want).encode()
    exp_res, exp_cols = restate(c.seqs, r, first, blocks, items, sites)
    same(res, exp_res, _ffi.INSERT_RESULT, RES_FIELDS, 'call rule')
    same(icols, exp_cols, _ffi.INSERT_COLUMN, COL_FIELDS, 'call rule')
    assert restate_call(sites, exp_cols).tobytes() == ''.join(want).encode()
    assert icols[5].tolist() == (0, 2, 2, 2, 0) and icols[9].tolist() == (1, 0, 0, 0, 2) and res[5].tolist() == (6, 6, 0, 1)


def test_errors_and_edge_inputs(eng, made):
    c = made
    recs, first, blocks = c.recs[:4], c.first[:5], c.blocks[:int(c.first[4])]
    windows = [(0, 500, 900), (0, 1000, 1000), (2, 0, 4000)]
    items = [(0, 0, 550, 650), (1, 0, 500, 900), (2, 2, 50, 500)]
    sites = [(0, 600, 5, 3), (0, 800, 7, 3), (2, 250, 64, 2), (2, 350, 1024, 2)]
    assert [int(x) for x in recs['tid']] == [0, 0, 2, 2]
    ok = eng.insertions(c.G, None, recs, first, blocks, windows, items, sites)
    exp_res, exp_cols = restate(c.seqs, recs, first, blocks, items, sites)
    same(ok[0], exp_res, _ffi.INSERT_RESULT, RES_FIELDS, 'the valid call')
    same(ok[1], exp_cols, _ffi.INSERT_COLUMN, COL_FIELDS, 'the valid call')
    assert ok[2].tobytes() == restate_call(sites, exp_cols).tobytes() and exp_res[:, 0].tolist() == [2, 1, 1, 1]

    def bad(match, windows=windows, items=items, sites=sites, recs=recs, first=first, blocks=blocks):
        with pytest.raises(RuntimeError, match=r'libmimeo_hip: mimeo_path_insertions: ' + match) as e:
            eng.insertions(c.G, None, recs, first, blocks, windows, items, sites)
        assert '(code -1)' in str(e.value)   # MIMEO_ERR_ARG

    def edit(rows, i, k, v):
        rows = [list(r) for r in rows]
        rows[i][k] = v
        return rows

    # everything mimeo_path_pileup checks, under this name and in its order: the paths ...
    blk = blocks.copy()
    blk['len'][1] = 0
    bad(r'record 0, block 1 .*len is 0', blocks=blk)
    r2 = recs.copy()
    r2['qid'][1] = 3
    bad(r'record 1: qid is not a scaffold', recs=r2)
    f2 = first.copy()
    f2[-1] += 1
    bad(r'record 3: path_first\[n\] is not nblocks', first=f2)
    # ... the windows ...
    bad(r'window 2 \(tid 3, \[0, 4000\)\): tid is not a scaffold', windows=edit(windows, 2, 0, 3))
    bad(r'window 1 \(tid 0, \[1001, 1000\)\): start is beyond end', windows=edit(windows, 1, 1, 1001))
    bad(r'window 2 \(tid 2, \[0, 4001\)\): end is beyond its scaffold', windows=edit(windows, 2, 2, 4001))
    # ... the items ...
    bad(r'item 1 \(aln 4, window 0, \[500, 900\)\): aln is not a record', items=edit(items, 1, 0, 4))
    bad(r'item 2 \(aln 2, window 3, .*window is not below nwin', items=edit(items, 2, 1, 3))
    bad(r"item 2 \(aln 2, window 0, .*does not lie on the record's target scaffold", items=edit(items, 2, 1, 0))
    bad(r'item 0 \(aln 0, window 0, \[651, 650\)\): w0 is beyond w1', items=edit(items, 0, 2, 651))
    bad(r'item 0 .*\[499, 650\)\): \[w0, w1\) does not lie inside the window', items=edit(items, 0, 2, 499))
    bad(r'item 1 .*\[500, 901\)\): \[w0, w1\) does not lie inside the window', items=edit(items, 1, 3, 901))
    # ... and then the sites
    bad(r'site 3 \(window 3, x 350, ncols 1024\): window is not below nwin', sites=edit(sites, 3, 0, 3))
    bad(r'site 0 \(window 0, x 499, ncols 5\): x does not lie inside the window', sites=edit(sites, 0, 1, 499))
    bad(r'site 1 \(window 0, x 900, ncols 7\): x does not lie inside the window', sites=edit(sites, 1, 1, 900))
    bad(r'site 1 \(window 1, x 1000, ncols 7\): x does not lie inside the window', sites=edit(edit(sites, 1, 0, 1), 1, 1, 1000))   # an empty window holds no site
    bad(r'site 2 \(window 2, x 250, ncols 0\): ncols is not in 1 \.\. 1024', sites=edit(sites, 2, 2, 0))
    bad(r'site 3 \(window 2, x 350, ncols 1025\): ncols is not in 1 \.\. 1024', sites=edit(sites, 3, 2, 1025))
    bad(r'site 1 \(window 0, x 600, ncols 7\): the sites are not strictly increasing', sites=edit(sites, 1, 1, 600))
    bad(r'site 3 \(window 2, x 249, .*the sites are not strictly increasing', sites=edit(sites, 3, 1, 249))
    bad(r'site 2 \(window 0, x 850, .*the sites are not strictly increasing', sites=[sites[0], sites[2], (0, 850, 1, 1), sites[3]])
    bad(r'item 1 .*aln is not a record', items=edit(items, 1, 0, 4), sites=edit(sites, 0, 2, 0))   # a bad item is named before a bad site
    with pytest.raises(ValueError):
        eng.insertions(c.G, None, recs, first[:-1], blocks, windows, items, sites)
    # nothing was launched and nothing is broken: the valid call answers as before
    again = eng.insertions(c.G, None, recs, first, blocks, windows, items, sites)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ok))
    # nsites == 0: MIMEO_OK at once, nothing is looked at, not even a bad item
    res, icols, icall = eng.insertions(c.G, None, recs, first, blocks, windows, [(99, 0, 0, 0)], np.zeros((0, 4)))
    assert res.size == 0 and res.dtype == _ffi.INSERT_RESULT and icols.size == 0 and icols.dtype == _ffi.INSERT_COLUMN and icall.size == 0 and icall.dtype == np.uint8
    # nitems == 0: zero counts and '-' bytes — also without a single record
    for r, f, b in ((recs, first, blocks), (recs[:0], first[:1], blocks[:0])):
        res, icols, icall = eng.insertions(c.G, None, r, f, b, windows, np.zeros((0, 4)), sites)
        assert res.size == 4 and not res.tobytes().strip(b'\0') and icols.size == 1100 and not icols.tobytes().strip(b'\0') and icall.tobytes() == b'-' * 1100
    # Q given as a genome of its own, with the query scaffolds in another order
    B = eng.Genome(['p2', 'p0', 'p1'], [c.seqs[2], c.seqs[0], c.seqs[1]])
    r2 = recs.copy()
    r2['qid'] = (recs['qid'] + 1) % 3
    other = eng.insertions(c.G, B, r2, first, blocks, windows, items, sites)
    B.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(other, ok))


# ---- end to end ------------------------------------------------------------------------------------------------------------

E2E_SEED = 5
# (family, reverse-complemented) of the six slots of either scaffold, 3000 bp apart: the layout of tests/test_gpu_pileup.py, where
# the reasons for it are written down (the engine chains like lastz --chain, so a copy has at most four rows over it).
E2E_LAYOUT = (((0, False), (0, False), (1, False), (1, True), (0, True), (0, True)),
              ((0, False), (0, False), (1, True), (0, True), (0, False), (1, False)))
DEL_LEN, FLANK = 12, 15


def consensus_genome(seed=E2E_SEED, layout=E2E_LAYOUT, div=0.08):
    """The genome of tests/test_gpu_pileup.py — two scaffolds of 20 kbp of random sequence; a family of 600 bp planted 8 times,
    three of them reverse-complemented, and one of 400 bp planted 4 times; every copy with independent substitutions at 8 per
    cent — changed so that every copy of family 0 carries one private deletion of DEL_LEN bases at a family offset of its own.
    The FLANK bases on either side of every such segment are free of substitutions in every copy, the segment's first base
    differs from the base that follows the segment and its last base from the base in front of it: any shifted gap costs a
    mismatch, so the placement of the gap in an alignment is unique.  Returns (names, seqs, families as codes 0..3, [(scaffold,
    start, end, family, reversed, offset of the deleted segment or None)])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    codes = [rng.integers(0, 4, size=20_000, dtype=np.uint8) for _ in range(2)]
    fams = [rng.integers(0, 4, size=600, dtype=np.uint8), rng.integers(0, 4, size=400, dtype=np.uint8)]
    ncopies = sum(1 for slots in layout for f, _ in slots if f == 0)
    offs, clean = [], np.zeros(600, dtype=bool)
    for k in range(ncopies):   # 60 bases apart from 60 on: the clean stretches of FLANK + DEL_LEN + FLANK = 42 do not meet
        o = 60 + 60 * k
        while fams[0][o] == fams[0][o + DEL_LEN] or fams[0][o + DEL_LEN - 1] == fams[0][o - 1]:
            o += 1
        assert o < 60 + 60 * k + 15
        offs.append(o)
        clean[o - FLANK:o + DEL_LEN + FLANK] = True
    planted, k0 = [], 0
    for s, slots in enumerate(layout):
        for k, (f, rev) in enumerate(slots):
            cp = fams[f].copy()
            sub = rng.random(cp.size) < div
            if f == 0:
                sub &= ~clean
            cp[sub] = (cp[sub] + rng.integers(1, 4, size=int(sub.sum()), dtype=np.uint8)) % 4
            off = None
            if f == 0:
                off = offs[k0]
                k0 += 1
                cp = np.concatenate([cp[:off], cp[off + DEL_LEN:]])
            if rev:
                cp = (3 - cp)[::-1]
            p = 1500 + 3000 * k + int(rng.integers(0, 300))
            codes[s][p:p + cp.size] = cp
            planted.append((s, p, p + cp.size, f, rev, off))
    return ['cs0', 'cs1'], [ACGT[c] for c in codes], fams, planted


def _fasta(path):
    recs = []
    for line in open(path).read().splitlines():
        if line.startswith('>'):
            recs.append([line, ''])
        else:
            assert 0 < len(line) <= 60 and (len(recs[-1][1]) % 60 == 0), line
            recs[-1][1] += line
    return recs


def test_cli_consensus_insertions_end_to_end(eng, tmp_path):
    """Rows per representative observed on the MI355X with this layout: family 0 comes out as one record of 7 members, its
    representative the first copy of scaffold cs0 with three rows over every column (mean_depth=3.00), all three inserting the
    twelve bases at its private deletion: 3 against the own copy's gap vote of 1, ins_sites=1, inserted=12.  Family 1 (3 members
    linked, two rows) has no site."""
    from mimeo_amd import run_self
    names, seqs, fams, planted = consensus_genome()
    assert sum(1 for p in planted if p[3] == 0) == 8 and len({p[5] for p in planted if p[3] == 0}) == 8
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    plain, ins = tmp_path / 'plain', tmp_path / 'ins'
    run_self.main(['--afasta', fa, '-d', str(plain), '--loglevel', 'WARNING', '--consensus', str(plain / 'lib.fa')])
    run_self.main(['--afasta', fa, '-d', str(ins), '--loglevel', 'WARNING', '--consensus', str(ins / 'lib.fa'), '--consensusInsertions'])
    # nothing else changes
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3'):
        assert (ins / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(os.listdir(ins)) == sorted(os.listdir(plain))
    # the plain library is what a run without the flag writes: byte-identical to the library of a third run that never heard of it
    from mimeo_amd import workflow
    A = eng.Genome.from_fasta([fa], None)
    args = run_self.mainArgs(['--afasta', fa])
    try:
        workflow.self_repeats(A, workflow.all_pairs(len(A.names)), str(tmp_path / 'c.tab'), str(tmp_path / 'c.gff3'), prefix=args.prefix, label=args.label,
                              consensus=str(tmp_path / 'c.fa'))
        workflow.self_repeats(A, workflow.all_pairs(len(A.names)), str(tmp_path / 'b.tab'), str(tmp_path / 'b.gff3'), prefix=args.prefix, label=args.label,
                              consensus=str(tmp_path / 'b.fa'), consensus_budget=700, consensus_insertions=True)
    finally:
        A.close()
    assert (tmp_path / 'c.fa').read_bytes() == (plain / 'lib.fa').read_bytes()
    assert (tmp_path / 'b.fa').read_bytes() == (ins / 'lib.fa').read_bytes()   # a budget of 700 cuts the windows into runs and changes no byte
    assert (tmp_path / 'b.gff3').read_bytes() == (plain / 'mimeo-self_repeats.gff3').read_bytes()
    old, new = _fasta(plain / 'lib.fa'), _fasta(ins / 'lib.fa')
    assert len(old) == len(new) >= 2
    restored = 0
    for (h0, s0), (h1, s1) in zip(old, new):
        assert h1.startswith(h0.split(' length=')[0] + ' length=') and ' inserted=' in h1 and ' inserted=' not in h0
        f0, f1 = (dict(x.split('=') for x in h.split()[1:] if '=' in x) for h in (h0, h1))
        assert {k: v for k, v in f1.items() if k not in ('length', 'inserted')} == {k: v for k, v in f0.items() if k != 'length'}
        assert int(f0['length']) == len(s0) and int(f1['length']) == len(s1) == len(s0) + int(f1['inserted'])   # length grows by exactly `inserted`
        assert set(s1) <= set('ACGTN')
        seqid, span = h0.split()[2].split(':')
        start, end = (int(x) for x in span.split('-'))
        s = names.index(seqid)
        over = [p for p in planted if p[0] == s and p[1] < end and start < p[2]]
        assert len(over) == 1, (h0, over)   # a region is one planted copy
        _, p0, p1, fam, rev, off = over[0]
        print(h1)
        if fam != 0:
            continue
        # the columns at the OTHER copies' private deletions are still called: one deleting row never outvotes the rest
        assert len(s0) == end - start, h0
        if int(f0['members']) < 2:
            continue
        # segment plus its clean flanks, as the representative's strand reads it
        mer = fams[0][off - FLANK:off + DEL_LEN + FLANK]
        mer = ACGT[(3 - mer)[::-1] if rev else mer].tobytes().decode()
        assert len(mer) == 42 and mer in s1 and mer not in s0, (h1, mer)
        restored += 1
    assert restored >= 1
