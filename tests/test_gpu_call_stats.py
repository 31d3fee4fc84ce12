"""The rows of a pile against the call (mimeo_path_call_stats, kernel K16; engine.call_stats; `mimeo self --copyDivergence
--landscape`) against a plain numpy restatement of "pileup v4, rows against the call" (include/mimeo_hip.h), written here from
the header's rules alone: per item the target columns of [lo, hi) one by one, a dict of its runs, the bases of every run against
the columns of its site, and the sites that the item spans.  Equality is exact, field by field."""
import os
import re

import numpy as np
import pytest

from mimeo_amd import _ffi
from mimeo_amd.synth import write_fasta
from tests.test_gpu_stack import ACGT, LONG, PATH, _stockholm, family_genome, letter, paper, revcomp

pytestmark = pytest.mark.gpu

FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_bases', 'del_bases', 'q_lo', 'q_hi')


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


# ---- the restatement -------------------------------------------------------------------------------------------------------

def classify(n, c, y):
    if c == 'N' or y == 'N':
        n[3] += 1
    elif c == y:
        n[0] += 1
    elif {c, y} in ({'A', 'G'}, {'C', 'T'}):
        n[1] += 1
    else:
        n[2] += 1


def restate(seqs, recs, first, blocks, windows, items, sites, call, icall):
    """(nitems, 8) in the order of mimeo_call_stats.  seqs: the scaffolds as uint8 letters; windows: rows of (tid, start, end);
    items: rows of (aln, window, w0, w1); sites: rows of (window, x, ncols, voters); call / icall: bytes."""
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 3).tolist()
    st = np.asarray(sites, dtype=np.int64).reshape(-1, 4).tolist()
    col_first = np.concatenate([[0], np.cumsum([e - s for _, s, e in win])]).astype(np.int64).tolist()
    icol_first = np.concatenate([[0], np.cumsum([s[2] for s in st])]).astype(np.int64).tolist()
    call, icall = bytes(call), bytes(icall)
    out, rc, under_of = [], {}, {}
    for a, g, w0, w1 in np.asarray(items, dtype=np.int64).reshape(-1, 4).tolist():
        qid, strand = int(recs[a]['qid']), int(recs[a]['qstrand'])
        if strand and qid not in rc:
            rc[qid] = revcomp(seqs[qid])
        Q = rc[qid] if strand else seqs[qid]
        blk = blocks[int(first[a]):int(first[a + 1])].tolist()
        if a not in under_of:   # target base -> the query base under it, for the bases under a block
            under_of[a] = {t + i: q + i for t, q, ln in blk for i in range(ln)}
        under = under_of[a]
        _, start, end = win[g]
        lo = max(w0, blk[0][0]) if blk else 0
        hi = min(w1, blk[-1][0] + blk[-1][2]) if blk else 0
        if lo >= hi:
            out.append([0] * 8)
            continue
        runs = {}   # p_k -> (first inserted base, dq_k), for the runs that belong to the item: w0 <= p_k < w1
        for k in range(1, len(blk)):
            p, qs = blk[k - 1][0] + blk[k - 1][2], blk[k - 1][1] + blk[k - 1][2]
            if blk[k][1] - qs > 0 and w0 <= p < w1:
                runs[p] = (qs, blk[k][1] - qs)
        n, qbases = [0] * 6, []
        for x in range(lo, hi):
            c = chr(call[col_first[g] + x - start])
            if x in under:
                qbases.append(under[x])
                if c == '-':
                    n[4] += 1   # the copy holds a base where the consensus has none
                else:
                    classify(n, c, letter(Q[under[x]]))
            elif c != '-':
                n[5] += 1
        site_at = {x: (s, nc) for s, (sw, x, nc, _) in enumerate(st) if sw == g}
        for p, (qs, dq) in runs.items():
            qbases += range(qs, qs + dq)
            for j in range(dq):
                s, nc = site_at.get(p, (0, 0))
                if j < nc and icall[icol_first[s] + j] != ord('-'):
                    classify(n, chr(icall[icol_first[s] + j]), letter(Q[qs + j]))
                else:
                    n[4] += 1   # no site, a run beyond ncols, or '-' in the consensus
        for x, (s, nc) in site_at.items():   # the sites that the item spans
            if w0 <= x < w1 and blk[0][0] < x < blk[-1][0] + blk[-1][2]:
                dq = runs.get(x, (0, 0))[1]
                n[5] += sum(1 for j in range(nc) if j >= dq and icall[icol_first[s] + j] != ord('-'))
        q_lo, q_hi = (min(qbases), max(qbases) + 1) if qbases else (0, 0)
        assert sum(n[:5]) == q_hi - q_lo and (not qbases or sorted(qbases) == list(range(q_lo, q_hi)))
        out.append(n + [q_lo, q_hi])
    return np.array(out, dtype=np.int64).reshape(-1, 8)


PAPER_CALL = b'ACA-A' + b'TCAN' + b'-G' + b'TGGG' + b'TTTTT'
PAPER_SITES = [(0, 5, 2, 0), (0, 12, 1, 0)]
PAPER_ICALL = b'C-' + b'A'
PAPER_ITEMS = [(0, 0, 0, 20), (0, 0, 5, 9), (0, 0, 0, 5), (0, 0, 9, 11), (0, 0, 15, 20)]
# item 0, [0, 15): block 0 AAGAA under ACA-A: A/A, C/A a transversion, A/G a transition, a base under '-', A/A; the run CC in front
# of 5 under the site's C-: a match and a base the consensus lacks; block 1 TTAC under TCAN: T/T, C/T a transition, A/A, N/C
# ambiguous; the deletion [9, 11) under -G: one letter of the consensus that the copy lacks; the run G in front of 9 has no site;
# block 2 TGNG under TGGG: T/T, G/G, G/N ambiguous, G/G; the site in front of 12 lies inside block 2: its letter A is a base the
# copy lacks.  Item 1 starts at the run's p_k and holds it; item 2 ends there and does not; item 3 is the deletion from its first
# base on: the run G and the consensus' G; item 4 lies off the alignment.
PAPER_EXP = [[8, 2, 1, 2, 3, 2, 0, 16], [3, 1, 0, 1, 1, 0, 5, 11], [2, 1, 1, 0, 1, 0, 0, 5], [0, 0, 0, 0, 1, 1, 11, 12], [0] * 8]


def test_restatement_on_paper():
    seqs, recs, first, blk = paper()
    got = restate(seqs, recs, first, blk, [(0, 0, 20)], PAPER_ITEMS, PAPER_SITES, PAPER_CALL, PAPER_ICALL)
    assert got.tolist() == PAPER_EXP


def test_kernel_on_paper(eng):
    seqs, recs, first, blk = paper()
    G = eng.Genome(['t', 'q'], seqs)
    try:
        got = eng.call_stats(G, None, recs, first, blk, [(0, 0, 20)], PAPER_ITEMS, PAPER_SITES, PAPER_CALL, PAPER_ICALL)
        assert got.dtype == _ffi.CALL_STATS and [list(r) for r in got.tolist()] == PAPER_EXP
    finally:
        G.close()


# ---- made-up paths ---------------------------------------------------------------------------------------------------------

L = (6000, 8000, 300, 4000)
# 64 blocks of 40 whose starts take every residue mod 64 on the target (65 k) and on the query (16 + 3 k): 25 target bases deleted
# and 27 query bases inserted between two of them
MOD64 = [(300 + 65 * k, 2000 + 67 * k, 40) for k in range(64)]
# 150 blocks of 10 .. 16 bases, 20 target bases and 25 query bases from start to start: every gap is a both-jump gap
BIG = [(20 + 20 * k, 50 + 25 * k, 10 + k % 7) for k in range(150)]
BIG_SITES = sorted([(BIG[k - 1][0] + BIG[k - 1][2], 1 + k % 5) for k in range(1, 150)] + [(BIG[k][0] + 3, 1 + k % 3) for k in range(30)])


def _genome():
    rng = np.random.default_rng(160)
    s = [ACGT[rng.integers(0, 4, n)].copy() for n in L]
    s[1][110] = ord('N')             # under PATH's first block on the plus strand ...
    s[1][132] = ord('R')             # ... inside the run [130, 135): an IUPAC code is an N to the engine ...
    s[1][8000 - 1 - 112] = ord('n')  # ... and the same on the minus strand
    s[1][8000 - 1 - 131] = ord('N')
    s[1][500:520] = ord('N')         # inside the long run
    s[0][66] = ord('N')              # the target's own N under PATH's first block
    return ['p0', 'p1', 'p2', 'p3'], s


class Case:
    def __init__(self):
        self.names, self.seqs = _genome()
        self.recs, self.first, self.blocks = [], [0], []
        self.windows, self.items, self.sites, self.what = [], [], {}, {}

    def add(self, tid, qid, strand, blk):
        t_end = q_end = 0
        for t, q, ln in blk:   # the contract of mimeo_path_block, so that a slip in a table is not taken for a kernel's
            assert ln >= 1 and t >= t_end and q >= q_end and t + ln <= L[tid] and q + ln <= L[qid], (t, q, ln)
            t_end, q_end = t + ln, q + ln
        self.recs.append((tid, qid, strand))
        self.blocks.extend(blk)
        self.first.append(len(self.blocks))
        return len(self.recs) - 1

    def window(self, tid, start, end, sites=()):
        g = len(self.windows)
        self.windows.append((tid, start, end))
        self.sites[g] = [(g, x, n, 7) for x, n in sites]
        assert all(start <= x < end and 1 <= n <= 1024 for x, n in sites) and [x for x, _ in sites] == sorted({x for x, _ in sites})
        return g

    def item(self, what, a, g, w0, w1):
        tid, start, end = self.windows[g]
        assert self.recs[a][0] == tid and start <= w0 <= w1 <= end
        self.what.setdefault(what, []).append(len(self.items))
        self.items.append((a, g, w0, w1))

    def finish(self):
        r = np.zeros(len(self.recs), dtype=_ffi.ALIGNMENT)
        r['tid'], r['qid'], r['qstrand'] = [x[0] for x in self.recs], [x[1] for x in self.recs], [x[2] for x in self.recs]
        self.recs, self.first, self.blocks = r, np.array(self.first, dtype=np.uint64), np.array(self.blocks, dtype=_ffi.PATH_BLOCK)
        self.windows = np.array(self.windows, dtype=np.int64)
        self.items = np.array(self.items, dtype=np.int64)
        self.sites = np.array([s for g in sorted(self.sites) for s in self.sites[g]], dtype=np.int64)
        # the two calls: three bytes of four the target's own letter (so that every class occurs often), the others any of the
        # six; insertion columns any of the six, '-' one in four
        rng = np.random.default_rng(161)
        own = np.concatenate([np.frombuffer(''.join(letter(b) for b in self.seqs[t][s:e]).encode(), dtype=np.uint8) for t, s, e in self.windows.tolist()])
        self.own = own
        any6 = np.frombuffer(b'ACGTN-', dtype=np.uint8)
        self.call = np.where(rng.random(own.size) < 0.75, own, any6[rng.integers(0, 6, own.size)]).astype(np.uint8)
        self.icall = np.frombuffer(b'ACGTN---', dtype=np.uint8)[rng.integers(0, 8, int(self.sites[:, 2].sum()))].copy()
        return self


def made_case():
    c = Case()
    plus, minus = c.add(0, 1, 0, PATH), c.add(0, 1, 1, PATH)
    empty = c.add(0, 1, 0, [])
    lng = c.add(2, 1, 0, LONG)
    m_plus, m_minus = c.add(0, 1, 0, MOD64), c.add(0, 1, 1, MOD64)
    big = c.add(3, 1, 1, BIG)
    # windows of 1, 3 and 17 columns in front of windows of 1, 63, 64, 65 and 129: a window's first column at odd offsets of the planes
    widths = {}
    for lead, w in ((1, 1), (17, 63), (0, 64), (3, 65), (17, 129)):
        if lead:
            g = c.window(0, 70, 70 + lead)
            c.item('windows in front', plus, g, 70, 70 + lead)
        widths[w] = c.window(0, 60, 60 + w)
    # PATH is [50, 212): a site off the alignment (40, 229), at the first block's t (50: not spanned), inside a block (60), at runs
    # of 5 (80: fewer bases than columns) and 10 bases (135, where both jump), at a junction without a run (100), inside a deletion
    # (105), at x and x + 1 (171, 172); 1, 63, 64 and 65 columns
    A = c.window(0, 40, 230, [(40, 2), (50, 3), (60, 1), (80, 63), (100, 3), (105, 64), (135, 65), (171, 2), (172, 3), (229, 17)])
    # the same window again with sites of its own: as many columns as bases (5), fewer (4 for 10), and no site at 171
    B = c.window(0, 40, 230, [(80, 5), (135, 4), (172, 17)])
    nothing = c.window(0, 100, 100)
    C = c.window(2, 0, 100, [(30, 1024)])
    D = c.window(2, 20, 40, [(30, 16)])
    E = c.window(0, 130, 180, [(135, 10)])   # overlaps A and B
    M = c.window(0, 250, 4500, [(MOD64[k][0] + 40, 1 + 9 * (k % 4)) for k in range(0, 63, 3)])
    W = c.window(3, 0, 3100, BIG_SITES)
    for w, g in widths.items():
        c.item('windows of 1, 63, 64, 65 and 129 columns', plus, g, 60, 60 + w)
        c.item('windows of 1, 63, 64, 65 and 129 columns', minus, g, 60, 60 + w)
    c.item('a minus-strand record', minus, A, 40, 230)
    c.item('an item clipped inside a block', plus, A, 60, 70)
    c.item('w0 == p_k and w1 == p_k', plus, A, 80, 120)
    c.item('w0 == p_k and w1 == p_k', plus, A, 81, 120)    # one base on: the run is not the item's
    c.item('w0 == p_k and w1 == p_k', plus, A, 60, 80)     # the run is not counted, the site not spanned
    c.item('w0 == p_k and w1 == p_k', minus, A, 135, 150)  # where both jump
    c.item('a site at lo', plus, A, 60, 75)
    c.item('a site at lo', plus, A, 105, 108)              # inside the deletion: the site's letters are bases the copy lacks
    c.item('a site at lo', plus, A, 45, 60)                # at the first block's t: not spanned
    c.item('w1 inside a deletion', plus, A, 90, 105)
    c.item('a record without blocks', empty, A, 40, 230)
    c.item('an empty window', plus, nothing, 100, 100)
    c.item('an empty window', plus, A, 120, 120)
    c.item('the same item twice', plus, A, 40, 230)
    c.item('dq below, equal to and above ncols', plus, B, 40, 230)
    c.item('the same item twice', plus, A, 40, 230)
    c.item('a run at a base without a site', minus, B, 150, 212)
    c.item('a site of 1024 columns', lng, C, 0, 100)
    c.item('dq below, equal to and above ncols', lng, D, 20, 40)
    c.item('w0 == p_k and w1 == p_k', lng, D, 30, 31)
    c.item('overlapping and repeated windows', plus, E, 130, 180)
    c.item('overlapping and repeated windows', minus, B, 40, 140)
    c.item('a both-jump gap', plus, E, 135, 136)
    c.item('a both-jump gap', minus, E, 134, 141)
    for k in range(300):
        w0 = 130 + k % 47
        c.item('300 items on one window', (plus, minus)[k & 1], E, w0, min(180, w0 + 1 + (7 * k) % 50))
    c.item('block starts at every residue mod 64', m_plus, M, 250, 4500)
    c.item('block starts at every residue mod 64', m_minus, M, 250, 4500)
    c.item('block starts at every residue mod 64', m_minus, M, 1000, 3001)
    c.item('150 blocks with 179 sites', big, W, 0, 3100)
    c.item('150 blocks with 179 sites', big, W, 1500, 1503)
    c.item('150 blocks with 179 sites', big, W, 31, 2999)
    c.finish()
    # by hand: N in the call under PATH's first block; the five bases of the run in front of 80 of window A under A N C - G
    col_first = np.concatenate([[0], np.cumsum(c.windows[:, 2] - c.windows[:, 1])])
    c.call[int(col_first[A]) + 55 - 40] = ord('N')
    s80 = int(np.flatnonzero((c.sites[:, 0] == A) & (c.sites[:, 1] == 80))[0])
    c.at80 = int(c.sites[:s80, 2].sum())
    c.icall[c.at80:c.at80 + 5] = np.frombuffer(b'ANC-G', dtype=np.uint8)
    return c


LIST = ('windows in front', 'windows of 1, 63, 64, 65 and 129 columns', 'a minus-strand record', 'an item clipped inside a block', 'w0 == p_k and w1 == p_k',
        'a site at lo', 'w1 inside a deletion', 'a record without blocks', 'an empty window', 'the same item twice', 'dq below, equal to and above ncols',
        'a run at a base without a site', 'a site of 1024 columns', 'overlapping and repeated windows', 'a both-jump gap', '300 items on one window',
        'block starts at every residue mod 64', '150 blocks with 179 sites')


@pytest.fixture(scope='module')
def made(eng):
    c = made_case()
    c.exp = restate(c.seqs, c.recs, c.first, c.blocks, c.windows, c.items, c.sites, c.call, c.icall)   # once, shared, and left as it is
    c.exp.setflags(write=False)
    c.G = eng.Genome(c.names, c.seqs)
    c.got = eng.call_stats(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites, c.call, c.icall)
    yield c
    c.G.close()


def same(got, exp, tag):
    assert got.dtype == _ffi.CALL_STATS and got.shape == (exp.shape[0],), tag
    for k, f in enumerate(FIELDS):
        bad = np.flatnonzero(got[f].astype(np.int64) != exp[:, k])
        assert bad.size == 0, (tag, f, bad[:5], got[f][bad[:5]], exp[bad[:5], k])


def test_made_up_paths_against_the_restatement(made):
    c = made
    assert set(LIST) == set(c.what)
    same(c.got, c.exp, 'made-up paths')
    res = lambda what, k=0: c.exp[c.what[what][k]].tolist()
    # not vacuous, on the restatement's side: each case is what its name says
    assert sorted({int(w1 - w0) for _, _, w0, w1 in c.items[c.what['windows of 1, 63, 64, 65 and 129 columns']].tolist()}) == [1, 63, 64, 65, 129]
    col_first = np.concatenate([[0], np.cumsum(c.windows[:, 2] - c.windows[:, 1])])
    assert len({int(col_first[g]) % 64 for _, g, _, _ in c.items[c.what['windows of 1, 63, 64, 65 and 129 columns']].tolist()}) == 5
    assert {t % 64 for t, _, _ in MOD64} == set(range(64)) == {q % 64 for _, q, _ in MOD64} == {(8000 - q - 40) % 64 for _, q, _ in MOD64}
    assert sorted(set(c.sites[:, 2].tolist()) & {1, 63, 64, 65, 1024}) == [1, 63, 64, 65, 1024]
    assert len(BIG) == 150 and len(BIG_SITES) == 179 and len(c.what['300 items on one window']) == 300
    assert (c.exp[:, :6].sum(axis=0) > 100).all()   # every field is counted often
    full, again = res('the same item twice'), res('the same item twice', 1)
    assert full == again and full[6:] == [100, 267] and sum(full[:5]) == 167
    assert res('a minus-strand record')[6:] == [100, 267] and res('a minus-strand record') != full
    assert res('an item clipped inside a block')[6:] == [110, 120] and sum(res('an item clipped inside a block')[:5]) == 10
    a, b, e, d = (res('w0 == p_k and w1 == p_k', k) for k in range(4))
    assert a[6:] == [130, 165] and b[6:] == [136, 165] and sum(a[:5]) - sum(b[:5]) == 6 and e[6:] == [110, 130] and d[6:] == [180, 200]
    # the site at 80 (63 columns, A N C - G under the run's five bases): a holds the run, b and e do not span the site (x < w0, x == w1)
    l80 = bytes(c.icall[c.at80:c.at80 + 63])
    assert l80[:5] == b'ANC-G' and a[3] >= 1 and a[4] >= 1   # N inside a run and '-' in the middle of a site
    assert a[5] - b[5] >= 0 and res('a site at lo', 2)[6:] == [100, 110]
    assert res('a site at lo', 1)[:5] == [0] * 5 and res('a site at lo', 1)[5] > 3   # inside the deletion: only bases that the copy lacks
    assert res('a record without blocks') == [0] * 8 and res('an empty window') == [0] * 8 and res('an empty window', 1) == [0] * 8
    assert res('a site of 1024 columns')[6:] == [300, 1390] and res('a site of 1024 columns')[4] >= 26
    assert res('dq below, equal to and above ncols', 1)[6:] == [310, 1380] and res('dq below, equal to and above ncols', 1)[4] >= 1034
    assert res('w0 == p_k and w1 == p_k', 4)[6:] == [320, 1371]
    assert res('a both-jump gap')[6:] == [180, 190] and res('a both-jump gap', 1)[6:] == [179, 191]
    assert res('150 blocks with 179 sites')[6:] == [50, 50 + 25 * 149 + 10 + 149 % 7]
    assert b'N' in bytes(c.call) and b'N' in bytes(c.icall) and b'-' in bytes(c.call)


def test_what_a_caller_may_rely_on(eng, made):
    """the guarantees of the header and the witnesses: K10 with the own letters as call, K15's stretch and rows, K13's and K14's
    column counts — on the inputs of the restatement"""
    c = made
    got = c.got
    g64 = {f: got[f].astype(np.int64) for f in FIELDS}
    classified = g64['matches'] + g64['transitions'] + g64['transversions'] + g64['ambiguous']
    assert (classified + g64['ins_bases'] == g64['q_hi'] - g64['q_lo']).all()
    # K15: the same stretch, and bases + hidden
    res, row_first, rows = eng.stack(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites)
    assert (res['q_lo'] == got['q_lo']).all() and (res['q_hi'] == got['q_hi']).all()
    assert (res['bases'].astype(np.int64) + res['hidden'] == classified + g64['ins_bases']).all()
    # K10: with the target's own letters as the call and no site, the six fields of every item alone in a group
    _, own = eng.pileup(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items[:0], counts=False)
    assert own.tobytes() == c.own.tobytes()
    plain = eng.call_stats(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites[:0], own, None)
    alone = c.items.copy()
    alone[:, 1] = np.arange(alone.shape[0])
    k10 = eng.window_stats(c.G, None, c.recs, c.first, c.blocks, alone, alone.shape[0])
    for f in FIELDS[:6]:
        assert (plain[f].astype(np.int64) == k10[f].astype(np.int64)).all(), f
    assert int(k10['ambiguous'].sum()) > 0 and (plain['q_lo'] == got['q_lo']).all() and (plain['q_hi'] == got['q_hi']).all()
    # K13 and K14: over a window's items the classified letters are the columns' a + c + g + t + n at the letter columns of the
    # two calls, and ins_bases the bases under '-' and the inserted bases that met no letter
    cols, _ = eng.pileup(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, call=False)
    ires, icols, _ = eng.insertions(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites, call=False)
    depth5 = sum(cols[f].astype(np.int64) for f in 'acgtn')
    idepth = sum(icols[f].astype(np.int64) for f in 'acgtn')
    col_first = np.concatenate([[0], np.cumsum(c.windows[:, 2] - c.windows[:, 1])]).astype(np.int64)
    icol_first = np.concatenate([[0], np.cumsum(c.sites[:, 2])]).astype(np.int64)
    site_of_col = np.repeat(np.arange(c.sites.shape[0]), c.sites[:, 2])
    letter_col, iletter = c.call != ord('-'), c.icall != ord('-')
    seen = 0
    for g in range(c.windows.shape[0]):
        mine = c.items[:, 1] == g
        t = slice(int(col_first[g]), int(col_first[g + 1]))
        on_g = c.sites[site_of_col, 0] == g
        met = int(idepth[on_g & iletter].sum())
        assert int(classified[mine].sum()) == int(depth5[t][letter_col[t]].sum()) + met, g
        assert int(g64['ins_bases'][mine].sum()) == int(depth5[t][~letter_col[t]].sum()) + int(cols['ins_bases'][t].astype(np.int64).sum()) - met, g
        seen += met
    assert seen > 1000
    # K15's rows against the spliced call, letter column by letter column
    span = {}
    for a in set(c.items[:, 0].tolist()):
        blk = c.blocks[int(c.first[a]):int(c.first[a + 1])]
        span[a] = (int(blk['t'][0]), int(blk['t'][-1]) + int(blk['len'][-1])) if blk.size else (0, 0)
    for k, (a, g, w0, w1) in enumerate(c.items.tolist()):
        text = rows[int(row_first[k]):int(row_first[k + 1])].tobytes()
        _, start, end = c.windows[g].tolist()
        mine = {int(s[1]): (i, int(s[2])) for i, s in enumerate(c.sites.tolist()) if s[0] == g}
        n, at = [0] * 6, 0
        for x in range(start, end):
            if x in mine:
                s, nc = mine[x]
                for j in range(nc):
                    ch, cons = chr(text[at + j]), chr(c.icall[int(icol_first[s]) + j])
                    if ch != '.':
                        if cons == '-':
                            n[4] += 1
                        else:
                            classify(n, cons, ch.upper())
                    elif cons != '-' and w0 <= x < w1 and span[a][0] < x < span[a][1]:
                        n[5] += 1
                at += nc
            ch, cons = chr(text[at]), chr(c.call[int(col_first[g]) + x - start])
            at += 1
            if ch in 'ACGTN':
                if cons == '-':
                    n[4] += 1
                else:
                    classify(n, cons, ch)
            elif ch == '-' and cons != '-':
                n[5] += 1
        n[4] += int(res['hidden'][k])   # the inserted bases that have no column
        assert at == len(text) and n == [int(got[f][k]) for f in FIELDS[:6]], (k, n, got[k])


SETTINGS = ({}, {'MIMEO_CALL_STATS_SLICE_BLOCKS': '1'}, {'MIMEO_CALL_STATS_JOB_COLUMNS': '1'}, {'MIMEO_CALL_STATS_JOB_COLUMNS': '100'},
            {'MIMEO_PATH_LAUNCH_JOBS': '3'})


def test_every_setting_gives_the_same_counts(eng, made, monkeypatch, capfd):
    """the whole case under the defaults, with every alignment a slice of its own, every target column a job of its own, jobs of
    100 columns, and three jobs per launch: the counts of the restatement.  The switches are read per call."""
    c = made
    said = []
    for e in SETTINGS:
        with monkeypatch.context() as m:
            m.setenv('MIMEO_CALL_STATS_STATS', '1')
            for name, v in e.items():
                m.setenv(name, v)
            capfd.readouterr()
            got = eng.call_stats(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites, c.call, c.icall)
            err = capfd.readouterr().err
        same(got, c.exp, e)
        assert got.tobytes() == c.got.tobytes(), e
        m = re.search(r'\[k16\] call stats: (\d+) items, (\d+) sites, (\d+) jobs, slices (\d+) of (\d+), launches (\d+), kernels', err)
        assert m, err
        said.append(dict(zip(('items', 'sites', 'jobs', 'slices', 'of', 'launches'), (int(x) for x in m.groups()))))
    plain, slice1, job1, job100, launch3 = said
    reach = c.exp[:, 7] + c.exp[:, 5] > 0   # an item that reaches its alignment has a base or spans a column
    lo = np.array([max(w0, int(c.blocks['t'][int(c.first[a])])) if c.first[a + 1] > c.first[a] else 0 for a, _, w0, _ in c.items.tolist()])
    hi = np.array([min(w1, int(c.blocks['t'][int(c.first[a + 1]) - 1]) + int(c.blocks['len'][int(c.first[a + 1]) - 1])) if c.first[a + 1] > c.first[a] else 0
                   for a, _, _, w1 in c.items.tolist()])
    width = np.maximum(hi - lo, 0)
    assert plain['items'] == c.items.shape[0] and plain['sites'] == c.sites.shape[0]
    assert plain['jobs'] == int((width > 0).sum()) >= int(reach.sum()) and plain['slices'] == 1 and plain['launches'] == 2 + 1   # the two calls packed, one launch
    assert slice1['slices'] == 6 and slice1['of'] == 7 and slice1['launches'] == 2 + 6
    assert job1['jobs'] == int(width.sum()) and job100['jobs'] == int(((width + 99) // 100).sum())
    assert launch3['launches'] == 2 + (plain['jobs'] + 2) // 3


def test_errors_and_degenerate_calls(eng, made):
    c = made
    recs, first, blocks = c.recs[:4], c.first[:5], c.blocks[:int(c.first[4])]
    windows = [(0, 40, 230), (0, 100, 100), (2, 0, 100)]
    items = [(0, 0, 50, 212), (1, 0, 80, 120), (3, 2, 0, 100)]
    sites = [(0, 80, 5, 0), (0, 135, 7, 0), (2, 30, 64, 0)]
    rng = np.random.default_rng(162)
    call = np.frombuffer(b'ACGTN-', dtype=np.uint8)[rng.integers(0, 6, 290)].copy()
    icall = np.frombuffer(b'ACGTN-', dtype=np.uint8)[rng.integers(0, 6, 76)].copy()
    ok = eng.call_stats(c.G, None, recs, first, blocks, windows, items, sites, call, icall)
    same(ok, restate(c.seqs, recs, first, blocks, windows, items, sites, call, icall), 'the valid call')

    def bad(match, windows=windows, items=items, sites=sites, recs=recs, first=first, blocks=blocks, call=call, icall=icall):
        with pytest.raises(RuntimeError, match=r'libmimeo_hip: mimeo_path_call_stats: ' + match) as e:
            eng.call_stats(c.G, None, recs, first, blocks, windows, items, sites, call, icall)
        assert '(code -1)' in str(e.value)   # MIMEO_ERR_ARG

    def edit(rows, i, k, v):
        rows = [list(r) for r in rows]
        rows[i][k] = v
        return rows

    def byte(a, i, v):
        a = a.copy()
        a[i] = v
        return a

    # everything mimeo_path_stack checks, under this name and in its order: the paths, the windows, the items, the sites
    blk = blocks.copy()
    blk['len'][1] = 0
    bad(r'record 0, block 1 .*len is 0', blocks=blk)
    r2 = recs.copy()
    r2['qid'][1] = 4
    bad(r'record 1: qid is not a scaffold', recs=r2)
    bad(r'window 2 \(tid 4, \[0, 100\)\): tid is not a scaffold', windows=edit(windows, 2, 0, 4))
    bad(r'window 1 \(tid 0, \[101, 100\)\): start is beyond end', windows=edit(windows, 1, 1, 101))
    bad(r'window 2 \(tid 2, \[0, 301\)\): end is beyond its scaffold', windows=edit(windows, 2, 2, 301), call=np.concatenate([call, call[:201]]))
    bad(r'item 1 \(aln 4, window 0, \[80, 120\)\): aln is not a record', items=edit(items, 1, 0, 4))
    bad(r'item 2 \(aln 3, window 3, .*window is not below nwin', items=edit(items, 2, 1, 3))
    bad(r"item 2 \(aln 3, window 0, .*does not lie on the record's target scaffold", items=edit(items, 2, 1, 0))
    bad(r'item 0 \(aln 0, window 0, \[213, 212\)\): w0 is beyond w1', items=edit(items, 0, 2, 213))
    bad(r'item 0 .*\[39, 212\)\): \[w0, w1\) does not lie inside the window', items=edit(items, 0, 2, 39))
    bad(r'site 2 \(window 3, x 30, ncols 64\): window is not below nwin', sites=edit(sites, 2, 0, 3))
    bad(r'site 0 \(window 0, x 39, ncols 5\): x does not lie inside the window', sites=edit(sites, 0, 1, 39))
    bad(r'site 2 \(window 2, x 30, ncols 0\): ncols is not in 1 \.\. 1024', sites=edit(sites, 2, 2, 0), icall=icall[:12])
    bad(r'site 2 \(window 2, x 30, ncols 1025\): ncols is not in 1 \.\. 1024', sites=edit(sites, 2, 2, 1025), icall=np.resize(icall, 12 + 1024))
    bad(r'site 1 \(window 0, x 80, ncols 7\): the sites are not strictly increasing', sites=edit(sites, 1, 1, 80))
    bad(r'item 1 .*aln is not a record', items=edit(items, 1, 0, 4), sites=edit(sites, 0, 2, 0), icall=icall[:71])   # a bad item is named before a bad site
    # the bytes of the two calls, checked last: call before icall
    bad(r'column 0 of call \(window 0, x 40\): byte 0x61 is not one of A C G T N -', call=byte(call, 0, ord('a')))
    bad(r'column 289 of call \(window 2, x 99\): byte 0x2e', call=byte(call, 289, ord('.')))
    bad(r'column 190 of call \(window 2, x 0\): byte 0x00', call=byte(call, 190, 0), icall=byte(icall, 0, ord('x')))
    bad(r'insertion column 0 of icall \(site 0, column 0\): byte 0x6e', icall=byte(icall, 0, ord('n')))
    bad(r'insertion column 75 of icall \(site 2, column 63\): byte 0x52', icall=byte(icall, 75, ord('R')))
    bad(r'site 1 .*not strictly increasing', sites=edit(sites, 1, 1, 80), call=byte(call, 5, ord('?')))   # a bad site is named before a bad byte
    bad(r'null argument', icall=None)   # icall == NULL with nicols > 0
    bad(r'null argument', call=None)
    # the checks run for a call without items too
    bad(r'column 7 of call \(window 0, x 47\): byte 0x3f', items=np.zeros((0, 4)), call=byte(call, 7, ord('?')))
    # the binding refuses arrays that are not as long as the columns before the library reads them
    with pytest.raises(ValueError, match='call has 289 bytes for 290 columns'):
        eng.call_stats(c.G, None, recs, first, blocks, windows, items, sites, call[:289], icall)
    # voters is not read
    again = eng.call_stats(c.G, None, recs, first, blocks, windows, items, edit(edit(sites, 0, 3, 0xFFFFFFFF), 1, 3, 9), call, icall)
    assert again.tobytes() == ok.tobytes()
    # nitems == 0 — also without a single record
    for r, f, b in ((recs, first, blocks), (recs[:0], first[:1], blocks[:0])):
        got = eng.call_stats(c.G, None, r, f, b, windows, np.zeros((0, 4)), sites, call, icall)
        assert got.size == 0 and got.dtype == _ffi.CALL_STATS
    # nsites == 0: every run is bases that the consensus lacks; icall None or empty
    exp = restate(c.seqs, recs, first, blocks, windows, items, np.zeros((0, 4)), call, b'')
    for ic in (None, icall[:0]):
        same(eng.call_stats(c.G, None, recs, first, blocks, windows, items, np.zeros((0, 4)), call, ic), exp, 'no site')
    assert exp[:, 4].tolist()[2] >= 1050
    # windows without a column: call None
    got = eng.call_stats(c.G, None, recs, first, blocks, [(0, 100, 100)], [(0, 0, 100, 100)] * 2, np.zeros((0, 4)), None, None)
    assert got.size == 2 and not got.tobytes().strip(b'\0')
    # Q given as a genome of its own, with the query scaffolds in another order
    B = eng.Genome(['p2', 'p0', 'p1'], [c.seqs[2], c.seqs[0], c.seqs[1]])
    r2 = recs.copy()
    r2['qid'] = (recs['qid'] + 1) % 3
    other = eng.call_stats(c.G, B, r2, first, blocks, windows, items, sites, call, icall)
    B.close()
    assert other.tobytes() == ok.tobytes()


# ---- end to end ------------------------------------------------------------------------------------------------------------

def _tsv(path):
    lines = open(path).read().splitlines()
    return lines[0].split('\t'), [l.split('\t') for l in lines[1:]]


def test_cli_copy_divergence_and_landscape_end_to_end(eng, tmp_path, monkeypatch):
    """Observed on the MI355X with the genome of tests/test_gpu_stack.py (family_genome: five copies of three families, 8 per cent
    independent substitutions per copy): every one of the twelve copies is closer to the five-vote consensus than to the
    representative's own letters.  (ts + tv) / (m + ts + tv) against the consensus / against the representative, as this test
    prints them: F1 (593 bases; the substitution-free flanks of its private deletions lower both) 0.0542 / 0.0865, 0.0390 / 0.0675,
    0.0592 / 0.0898, 0.0573 / 0.0912; F2 0.1087 / 0.1655, 0.0868 / 0.1393, 0.1301 / 0.1872, 0.0925 / 0.1425; F3 0.1040 / 0.1720,
    0.0757 / 0.1454, 0.0729 / 0.1397, 0.0857 / 0.1534 — the smallest gap is 0.0285."""
    from mimeo_amd import engine, formats, run_self, workflow
    names, seqs = family_genome()
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    plain, div = tmp_path / 'plain', tmp_path / 'div'
    common = ['--afasta', fa, '--loglevel', 'WARNING', '--consensusInsertions']
    run_self.main(common + ['-d', str(plain), '--consensus', str(plain / 'lib.fa'), '--familyAlignments', str(plain / 'f.sto')])
    run_self.main(common + ['-d', str(div), '--consensus', str(div / 'lib.fa'), '--familyAlignments', str(div / 'f.sto'), '--copyDivergence', str(div / 'd.tsv'),
                            '--landscape', str(div / 'l.tsv')])
    # TAB, GFF3, library and Stockholm bytes are what a run without the two flags writes
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3', 'lib.fa', 'f.sto'):
        assert (div / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(os.listdir(div)) == sorted(os.listdir(plain) + ['d.tsv', 'l.tsv'])
    head, rows = _tsv(div / 'd.tsv')
    assert '\t'.join(head) == formats.COPY_DIVERGENCE_HEADER
    # one rep line and one copy line per sequence row of the Stockholm block, with the same coordinates
    blocks = _stockholm(div / 'f.sto')
    assert len(blocks) >= 3 and [b['id'] for b in blocks] == list(dict.fromkeys(r[0] for r in rows))
    for b in blocks:
        mine = [r for r in rows if r[0] == b['id']]
        assert [r[1] for r in mine] == ['rep'] + ['copy'] * (len(b['rows']) - 1) and len(mine) >= 5
        for r, (name, _) in zip(mine, b['rows']):
            s, e = int(r[3]), int(r[4])
            assert name == ('%s/%d-%d' % (r[2], s + 1, e) if r[5] == '+' else '%s/%d-%d' % (r[2], e, s + 1)), (r, name)
    count = lambda r: dict(zip(head[6:12], (int(v) for v in r[6:12])))
    for r in rows:
        n = count(r)
        # m + ts + tv + amb + ins_bases is the stretch's length (the representative's: its own bases)
        assert n['matches'] + n['transitions'] + n['transversions'] + n['ambiguous'] + n['ins_bases'] == int(r[4]) - int(r[3]), r
        d, kd = formats._copy_values(n)
        assert r[12] == '%.4f' % d and r[13] == ('%.4f' % kd if kd is not None else 'NA')
    # the landscape: bases per family are those of the family's lines, every line falls into the bin its kd says, `all` is the sum
    lhead, lrows = _tsv(div / 'l.tsv')
    assert '\t'.join(lhead) == formats.LANDSCAPE_HEADER
    want = {}
    for r in rows:
        n = count(r)
        kd = formats._copy_values(n)[1]
        k = formats.landscape_bin(kd)
        key = ('NA', 'NA') if kd is None else ('0.50', 'inf') if k == 50 else ('%.2f' % (k / 100), '%.2f' % ((k + 1) / 100))
        assert kd is None or k == 50 or float(key[0]) <= kd < float(key[1])
        for fam in (r[0], 'all'):
            acc = want.setdefault((fam,) + key, [0, 0])
            acc[0] += 1
            acc[1] += n['matches'] + n['transitions'] + n['transversions'] + n['ambiguous']
    assert {tuple(r[:3]): [int(r[3]), int(r[4])] for r in lrows} == want and len(lrows) == len(want)
    assert [r[0] for r in lrows] == sorted((r[0] for r in lrows), key=lambda f: ([b['id'] for b in blocks] + ['all']).index(f))
    for fam in [b['id'] for b in blocks] + ['all']:
        mine = [r for r in lrows if r[0] == fam]
        assert mine and [float(r[1]) if r[1] != 'NA' else 9.0 for r in mine] == sorted(float(r[1]) if r[1] != 'NA' else 9.0 for r in mine)
    # each flag alone, with small runs of windows: the same two files; on the way every engine.call_stats call is repeated with the
    # representative's own letters as the call and no site
    pairs_seen = []
    real = engine.call_stats

    def both(A, B, recs, f2, b2, win, run, sites, call, icall):
        got = real(A, B, recs, f2, b2, win, run, sites, call, icall)
        _, own = engine.pileup(A, None, recs, f2, b2, win, run[:0], counts=False)
        pairs_seen.append((got, real(A, B, recs, f2, b2, win, run, sites[:0], own, None)))
        return got

    A = eng.Genome.from_fasta([fa], None)
    args = run_self.mainArgs(['--afasta', fa])
    try:
        monkeypatch.setattr(engine, 'call_stats', both)
        workflow.self_repeats(A, workflow.all_pairs(len(A.names)), str(tmp_path / 'b.tab'), str(tmp_path / 'b.gff3'), prefix=args.prefix, label=args.label,
                              copy_divergence=str(tmp_path / 'b.tsv'), consensus_budget=700)
        monkeypatch.setattr(engine, 'call_stats', real)
        workflow.self_repeats(A, workflow.all_pairs(len(A.names)), str(tmp_path / 'c.tab'), str(tmp_path / 'c.gff3'), prefix=args.prefix, label=args.label,
                              landscape=str(tmp_path / 'c.tsv'), consensus_budget=700)
    finally:
        A.close()
    assert (tmp_path / 'b.tsv').read_bytes() == (div / 'd.tsv').read_bytes() and (tmp_path / 'c.tsv').read_bytes() == (div / 'l.tsv').read_bytes()
    assert (tmp_path / 'b.tab').read_bytes() == (plain / 'mimeo_alignment.tab').read_bytes()
    assert not os.path.exists(tmp_path / 'b.sto') and len(pairs_seen) >= 2   # a budget of 700 columns: more than one run of windows
    # the consensus is closer to every copy than the representative is: a condition of the construction, not a tuned threshold —
    # the representative carries about 40 private substitutions that the five-vote consensus does not
    cons = np.concatenate([p[0] for p in pairs_seen])
    rep = np.concatenate([p[1] for p in pairs_seen])
    keep = cons['q_hi'] > cons['q_lo']
    cons, rep = cons[keep], rep[keep]
    copies = [r for r in rows if r[1] == 'copy']
    assert len(copies) == cons.size >= 12
    for r, sc, sr in zip(copies, cons, rep):
        assert [int(sc[f]) for f in FIELDS[:6]] == [int(v) for v in r[6:12]]
        dc, dr = formats._copy_values(sc)[0], formats._copy_values(sr)[0]
        print('%s %s:%s-%s%s consensus %.4f representative %.4f' % (r[0], r[2], r[3], r[4], r[5], dc, dr))
        assert dc < dr, r
