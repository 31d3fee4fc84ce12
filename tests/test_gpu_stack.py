"""The stacked rows of a pile (mimeo_path_stack, kernel K15; engine.stack; `mimeo self --familyAlignments`) against a plain numpy
restatement of "pileup v3, the stack" (include/mimeo_hip.h), written here from the header's rules alone: per item the columns of
its window one by one, a site's insertion columns directly in front of the column of its base, every byte from the rule of its
column, and the four fields of the row from the item's query bases counted one by one.  Equality is exact, byte by byte and field
by field."""
import os
import re

import numpy as np
import pytest

from mimeo_amd import _ffi
from mimeo_amd.synth import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
COMP = np.full(256, ord('N'), dtype=np.uint8)
for _c, _d in zip(b'ACGT', b'TGCA'):
    COMP[_c] = _d
    COMP[_c + 32] = _d + 32
RES_FIELDS = ('q_lo', 'q_hi', 'bases', 'hidden')


def revcomp(a):
    return COMP[a][::-1].copy()


def letter(b):
    """the engine keeps neither case nor IUPAC codes: A C G T, and N for everything else"""
    c = chr(int(b)).upper()
    return c if c in 'ACGT' else 'N'


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


# ---- the restatement -------------------------------------------------------------------------------------------------------

def restate(seqs, recs, first, blocks, windows, items, sites):
    """(res (nitems, 4) in the order of mimeo_stack_row, row_first, the rows as one bytes object).  seqs: the scaffolds as uint8
    letters; windows: rows of (tid, start, end); items: rows of (aln, window, w0, w1); sites: rows of (window, x, ncols, voters)."""
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 3).tolist()
    st = np.asarray(sites, dtype=np.int64).reshape(-1, 4).tolist()
    res, row_first, out, rc = [], [0], [], {}
    for a, g, w0, w1 in np.asarray(items, dtype=np.int64).reshape(-1, 4).tolist():
        qid, strand = int(recs[a]['qid']), int(recs[a]['qstrand'])
        if strand and qid not in rc:
            rc[qid] = revcomp(seqs[qid])
        Q = rc[qid] if strand else seqs[qid]
        blk = blocks[int(first[a]):int(first[a + 1])].tolist()
        _, start, end = win[g]
        ncols_at = {x: n for sw, x, n, _ in st if sw == g}
        lo = max(w0, blk[0][0]) if blk else 0
        hi = min(w1, blk[-1][0] + blk[-1][2]) if blk else 0
        runs = {}   # p_k -> (first inserted base, dq_k), for the runs that belong to the item: w0 <= p_k < w1
        for k in range(1, len(blk)):
            p, qs = blk[k - 1][0] + blk[k - 1][2], blk[k - 1][1] + blk[k - 1][2]
            if blk[k][1] - qs > 0 and w0 <= p < w1:
                runs[p] = (qs, blk[k][1] - qs)
        row, qbases, hidden = [], [], 0
        for x in range(start, end):
            if x in ncols_at:   # the site's columns, directly in front of the column of x
                qs, dq = runs.get(x, (0, 0))
                row += [letter(Q[qs + j]).lower() if j < dq else '.' for j in range(ncols_at[x])]
            if not lo <= x < hi:
                row.append('.')
                continue
            under = [b for b in blk if b[0] <= x < b[0] + b[2]]
            if under:
                row.append(letter(Q[under[0][1] + x - under[0][0]]))
                qbases.append(under[0][1] + x - under[0][0])
            else:
                row.append('-')
        for p, (qs, dq) in runs.items():
            qbases += range(qs, qs + dq)
            hidden += dq - min(dq, ncols_at.get(p, 0))
        text = ''.join(row)
        bases = sum(1 for ch in text if ch not in '.-')
        if qbases:
            assert sorted(qbases) == list(range(min(qbases), max(qbases) + 1))   # one contiguous stretch
            assert bases + hidden == len(qbases)
            res.append((min(qbases), max(qbases) + 1, bases, hidden))
        else:
            assert bases == 0
            res.append((0, 0, 0, 0))
        out.append(text)
        row_first.append(row_first[-1] + len(text))
    return np.array(res, dtype=np.int64).reshape(-1, 4), np.array(row_first, dtype=np.uint64), ''.join(out).encode()


def paper():
    T = np.frombuffer(b'AAAAACCCCCGGGGGTTTTTAAAAANNNNN', dtype=np.uint8)
    Q = np.frombuffer(b'AAGAACCTTACGTGNGGGTTCCAAAAA', dtype=np.uint8)
    recs = np.zeros(1, dtype=_ffi.ALIGNMENT)
    recs['qid'] = 1
    blk = np.array([(0, 0, 5), (5, 7, 4), (11, 12, 4)], dtype=_ffi.PATH_BLOCK)
    return [T, Q], recs, np.array([0, 3], dtype=np.uint64), blk


def test_restatement_on_paper():
    """The restatement itself, on the 30-base path of tests/test_gpu_pileup.py, small enough to write down by hand:
    block 0: t 0..5 over q 0..5; the 2 query bases CC inserted in front of target base 5; block 1: t 5..9 over q 7..11; then
    target bases 9 and 10 deleted and query base 11, a G, inserted: both jump, p = 9; block 2: t 11..15 over q 12..16"""
    seqs, recs, first, blk = paper()
    win = [(0, 0, 20)]
    res, rf, rows = restate(seqs, recs, first, blk, win, [(0, 0, 0, 20)], [(0, 5, 3, 0), (0, 9, 1, 0)])
    assert rows == b'AAGAA' + b'cc.' + b'TTAC' + b'g' + b'--' + b'TGNG' + b'.....' and rf.tolist() == [0, 24] and res.tolist() == [[0, 16, 16, 0]]
    # an item that starts at the site holds its run; one column for two bases: one is hidden
    res, rf, rows = restate(seqs, recs, first, blk, win, [(0, 0, 5, 9)], [(0, 5, 1, 0)])
    assert rows == b'.....' + b'c' + b'TTAC' + b'.' * 11 and res.tolist() == [[5, 11, 5, 1]]
    # an item that ends at the site does not; the deletion from its first base on holds the run that starts there, without a site
    # all of it hidden; behind its first base the deletion holds nothing
    res, rf, rows = restate(seqs, recs, first, blk, win, [(0, 0, 0, 5), (0, 0, 9, 11), (0, 0, 10, 11)], [(0, 5, 2, 0)])
    assert rows == b'AAGAA..' + b'.' * 15 + b'.' * 7 + b'....--' + b'.' * 9 + b'.' * 7 + b'.....-' + b'.' * 9
    assert rf.tolist() == [0, 22, 44, 66] and res.tolist() == [[0, 5, 5, 0], [11, 12, 0, 1], [0, 0, 0, 0]]
    # no site: the window's own columns; a site at the first block's start, inside a block, inside the deletion, off the alignment
    res, rf, rows = restate(seqs, recs, first, blk, win, [(0, 0, 0, 20)], np.zeros((0, 4)))
    assert rows == b'AAGAATTAC--TGNG.....' and res.tolist() == [[0, 16, 13, 3]]
    res, rf, rows = restate(seqs, recs, first, blk, win, [(0, 0, 0, 20)], [(0, 0, 1, 0), (0, 7, 1, 0), (0, 10, 2, 0), (0, 17, 1, 0)])
    assert rows == b'.AAGAATT.AC-..-TGNG...' + b'...' and res.tolist() == [[0, 16, 13, 3]]


def test_kernel_on_paper(eng):
    seqs, recs, first, blk = paper()
    G = eng.Genome(['t', 'q'], seqs)
    try:
        res, rf, rows = eng.stack(G, None, recs, first, blk, [(0, 0, 20)], [(0, 0, 0, 20), (0, 0, 5, 9), (0, 0, 9, 11)], [(0, 5, 3, 0), (0, 9, 1, 0)])
        assert rows.tobytes() == b'AAGAAcc.TTACg--TGNG.....' + b'.....cc.TTAC.' + b'.' * 11 + b'.' * 12 + b'g--' + b'.' * 9
        assert rf.tolist() == [0, 24, 48, 72] and res.tolist() == [(0, 16, 16, 0), (5, 11, 6, 0), (11, 12, 1, 0)]
    finally:
        G.close()


# ---- made-up paths ---------------------------------------------------------------------------------------------------------

L = (400, 1600, 300)
# an insertion of 5 at 80; a deletion [100, 110); both jump at 135 (10 bases, then [135, 140)); blocks that touch at 170; runs of 2
# and 3 bases at 171 and 172, one target base apart: [50, 212)
PATH = [(50, 100, 30), (80, 135, 20), (110, 155, 25), (140, 190, 30), (170, 220, 1), (171, 223, 1), (172, 227, 40)]
LONG = [(10, 300, 20), (30, 1370, 20)]   # a run of 1050 bases in front of 30


def _genome():
    rng = np.random.default_rng(150)
    s = [ACGT[rng.integers(0, 4, n)].copy() for n in L]
    s[1][110] = ord('N')             # under PATH's first block on the plus strand ...
    s[1][132] = ord('R')             # ... inside the run [130, 135): an IUPAC code is an N to the engine ...
    s[1][1600 - 1 - 112] = ord('n')  # ... and the same on the minus strand (reverse-complement bases 112 and 131)
    s[1][1600 - 1 - 131] = ord('N')
    s[1][240:250] += 32              # soft-masked under the last block
    s[1][500:520] = ord('N')         # inside the long run
    return ['p0', 'p1', 'p2'], s


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
        """an item, in the order of the calls; `what` names the case of the issue's list"""
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
        return self


def made_case():
    c = Case()
    plus, minus = c.add(0, 1, 0, PATH), c.add(0, 1, 1, PATH)
    empty = c.add(0, 1, 0, [])
    lng = c.add(2, 1, 0, LONG)
    # ncols 1, 15, 16, 17 and 1024 occur; a site at the window's first base (40) and at its last (229); sites at x and x + 1
    # (171, 172); at a junction without an insertion (100), inside a deletion (105), inside a block (60)
    A = c.window(0, 40, 230, [(40, 2), (60, 1), (80, 5), (100, 3), (105, 1), (135, 15), (171, 2), (172, 3), (229, 17)])
    # the same window again with sites of its own: more columns than bases (16 for 5), fewer (4 for 10), and no site at 171
    B = c.window(0, 40, 230, [(80, 16), (135, 4), (172, 17)])
    widths = {w: c.window(0, 60, 60 + w) for w in (1, 15, 16, 17, 33)}
    one = c.window(0, 70, 71)
    nothing = c.window(0, 100, 100)
    C = c.window(2, 0, 100, [(30, 1024)])
    D = c.window(2, 20, 40, [(30, 16)])
    E = c.window(0, 130, 180, [(135, 10)])   # overlaps A and B
    F = c.window(0, 80, 173, [(80, 5), (172, 3)])   # a run at the window's first base and one at its last
    for k in range(17):   # rows of one byte: a row starts at every alignment mod 16, and 16 of them share one group
        c.item('a row shorter than one group', (plus, minus)[k & 1], one, 70, 71)
    for w, g in widths.items():
        c.item('window widths 1, 15, 16, 17 and 33', plus, g, 60, 60 + w)
        c.item('window widths 1, 15, 16, 17 and 33', minus, g, 60, 60 + w)
    c.item('a minus-strand record', minus, A, 40, 230)
    c.item('an item clipped inside a block', plus, A, 60, 70)
    c.item('w0 == p_k', plus, A, 80, 120)
    c.item('w0 == p_k', plus, A, 81, 120)    # one base on: the run is not the item's
    c.item('w0 == p_k', minus, A, 135, 150)  # where both jump
    c.item('w1 inside a deletion', plus, A, 90, 105)
    c.item('a window wholly inside a deletion', plus, A, 102, 108)
    c.item('a window wholly inside a deletion', plus, A, 100, 108)   # from the deletion's first base: no run there either
    c.item('a window wholly inside a deletion', plus, A, 136, 139)   # behind the first base of a deletion that a run precedes
    c.item('a record without blocks', empty, A, 40, 230)
    c.item('an empty window', plus, nothing, 100, 100)
    c.item('an empty window', plus, A, 120, 120)   # an empty item of a window with columns
    c.item('the same item twice', plus, A, 40, 230)
    c.item('a run longer than ncols', plus, B, 40, 230)
    c.item('the same item twice', plus, A, 40, 230)
    c.item('a run at a base without a site', minus, B, 150, 212)
    c.item('ncols 1024', lng, C, 0, 100)
    c.item('a run longer than ncols', lng, D, 20, 40)
    c.item('w0 == p_k', lng, D, 30, 31)
    c.item('overlapping and repeated windows', plus, E, 130, 180)
    c.item('overlapping and repeated windows', minus, B, 40, 140)
    c.item('items out of order', plus, widths[16], 62, 70)
    c.item('both sequences jumping at one p_k', plus, E, 135, 136)
    c.item('both sequences jumping at one p_k', minus, E, 134, 141)
    c.item('a site at the first base and at the last', plus, F, 80, 173)
    c.item('a site at the first base and at the last', minus, F, 80, 173)
    return c.finish()


LIST = ('a row shorter than one group', 'window widths 1, 15, 16, 17 and 33', 'a minus-strand record', 'an item clipped inside a block', 'w0 == p_k',
        'w1 inside a deletion', 'a window wholly inside a deletion', 'a record without blocks', 'an empty window', 'the same item twice',
        'a run longer than ncols', 'a run at a base without a site', 'ncols 1024', 'overlapping and repeated windows', 'items out of order',
        'both sequences jumping at one p_k', 'a site at the first base and at the last')


@pytest.fixture(scope='module')
def made(eng):
    c = made_case()
    c.exp_res, c.exp_first, c.exp_rows = restate(c.seqs, c.recs, c.first, c.blocks, c.windows, c.items, c.sites)   # once, shared, and left as it is
    c.exp_res.setflags(write=False)
    c.G = eng.Genome(c.names, c.seqs)
    c.res, c.row_first, c.rows = eng.stack(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites)
    yield c
    c.G.close()


def same(got, exp, tag):
    res, row_first, rows = got
    exp_res, exp_first, exp_rows = exp
    assert row_first.dtype == np.dtype('<u8') and row_first.tolist() == exp_first.tolist(), tag
    assert rows.dtype == np.uint8 and rows.size == len(exp_rows), tag
    if rows.tobytes() != exp_rows:
        bad = np.flatnonzero(rows != np.frombuffer(exp_rows, dtype=np.uint8))
        k = int(np.searchsorted(exp_first, bad[0], side='right')) - 1
        lo, hi = int(exp_first[k]), int(exp_first[k + 1])
        raise AssertionError((tag, 'row', k, 'column', int(bad[0]) - lo, rows[lo:hi].tobytes(), exp_rows[lo:hi], bad.size))
    assert res.dtype == _ffi.STACK_ROW and res.shape == (exp_res.shape[0],), tag
    for k, f in enumerate(RES_FIELDS):
        bad = np.flatnonzero(res[f].astype(np.int64) != exp_res[:, k])
        assert bad.size == 0, (tag, f, bad[:5], res[f][bad[:5]], exp_res[bad[:5], k])


def test_made_up_paths_against_the_restatement(made):
    c = made
    assert set(LIST) == set(c.what)
    same((c.res, c.row_first, c.rows), (c.exp_res, c.exp_first, c.exp_rows), 'made-up paths')
    row = lambda what, k=0: c.exp_rows[int(c.exp_first[c.what[what][k]]):int(c.exp_first[c.what[what][k] + 1])]
    res = lambda what, k=0: c.exp_res[c.what[what][k]].tolist()
    # not vacuous: every byte of the alphabet occurs, and the list, item by item, on the restatement's side: each case is what
    # its name says
    assert set(c.exp_rows) == set(b'ACGTNacgtn-.')
    starts = {int(c.exp_first[k]) % 16 for k in c.what['a row shorter than one group']}
    assert starts == set(range(16)) and all(len(row('a row shorter than one group', k)) == 1 for k in range(17))
    assert sorted({len(row('window widths 1, 15, 16, 17 and 33', k)) for k in range(10)}) == [1, 15, 16, 17, 33]
    assert {int(c.exp_first[k]) % 16 for k in range(c.items.shape[0])} == set(range(16))
    full = row('the same item twice')
    assert full == row('the same item twice', 1) and len(full) == 190 + 49 and res('the same item twice') == [100, 267, 167 - 0, 0]
    assert full[:12] == b'............' and full[12:23].isupper()   # 40's two columns and the ten bases in front of the alignment
    minus = row('a minus-strand record')
    assert minus != full and [ch in b'.-' for ch in minus] == [ch in b'.-' for ch in full] and res('a minus-strand record') == res('the same item twice')
    assert b'N' in full and b'n' in full and b'N' in minus and b'n' in minus
    clip = row('an item clipped inside a block')
    assert clip.strip(b'.') == full[23:33] and res('an item clipped inside a block') == [110, 120, 10, 0]
    assert res('w0 == p_k') == [130, 155 + 10, 5 + 30, 0] and res('w0 == p_k', 1) == [136, 165, 29, 0] and res('w0 == p_k', 2) == [180, 200, 20, 0]
    assert res('w1 inside a deletion') == [145, 155, 10, 0] and row('w1 inside a deletion').strip(b'.').endswith(b'-----')
    assert [res('a window wholly inside a deletion', k) for k in range(3)] == [[0] * 4] * 3
    assert [row('a window wholly inside a deletion', k).strip(b'.').replace(b'.', b'') for k in range(3)] == [b'-' * 6, b'-' * 8, b'-' * 3]
    assert set(row('a record without blocks')) == {ord('.')} and res('a record without blocks') == [0] * 4
    assert row('an empty window') == b'' and set(row('an empty window', 1)) == {ord('.')} and res('an empty window', 1) == [0] * 4
    assert res('a run longer than ncols') == [100, 267, 167 - 6 - 2, 8] and res('a run longer than ncols', 1) == [310, 1380, 10 + 16 + 10, 1034]
    assert res('a run at a base without a site') == [200, 267, 67 - 2, 2]
    wide = row('ncols 1024')
    assert len(wide) == 1124 and res('ncols 1024') == [300, 1390, 1064, 26] and wide[30:1054].islower() and wide[210:230] == b'n' * 20
    assert res('w0 == p_k', 3) == [320, 1371, 17, 1034] and row('w0 == p_k', 3).strip(b'.').islower() is False
    assert res('both sequences jumping at one p_k') == [180, 190, 10, 0] and row('both sequences jumping at one p_k').count(b'-') == 1
    assert res('both sequences jumping at one p_k', 1) == [179, 191, 12, 0] and row('both sequences jumping at one p_k', 1).count(b'-') == 5
    for k in range(2):
        edge = row('a site at the first base and at the last', k)
        assert len(edge) == 93 + 8 and edge[:5].islower() and edge[5:6].isupper() and edge[-4:-1].islower() and edge[-1:].isupper()
        assert res('a site at the first base and at the last', k) == [130, 228, 98 - 10 - 2, 12]   # the runs at 135 and 171 have no site here
    # bases + hidden == q_hi - q_lo, always
    assert (c.exp_res[:, 2] + c.exp_res[:, 3] == c.exp_res[:, 1] - c.exp_res[:, 0]).all() and int((c.exp_res[:, 3] > 0).sum()) >= 4


def _columns(c):
    """per item its window's column kinds: (target base x, -1) for a target column, (site number, j) for an insertion column"""
    kinds = {}
    for g, (_, start, end) in enumerate(c.windows.tolist()):
        mine = {int(s[1]): (k, int(s[2])) for k, s in enumerate(c.sites.tolist()) if s[0] == g}
        kinds[g] = [kind for x in range(start, end) for kind in ([(mine[x][0], j) for j in range(mine[x][1])] if x in mine else []) + [(x, -1)]]
    return kinds


def test_cross_checks_against_k13_k14_and_k11(eng, made):
    """what a caller may rely on, against three existing kernels on the same inputs"""
    c = made
    cols, _ = eng.pileup(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, call=False)
    ires, icols, _ = eng.insertions(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites, call=False)
    row_first, trow, qrow = eng.path_text(c.G, None, c.recs, c.first, c.blocks)
    kinds = _columns(c)
    col_first = np.concatenate([[0], np.cumsum(c.windows[:, 2] - c.windows[:, 1])])
    icol_first = np.concatenate([[0], np.cumsum(c.sites[:, 2])])
    tcount = np.zeros((int(col_first[-1]), 6), dtype=np.int64)    # A C G T N - per target column
    icount = np.zeros((int(icol_first[-1]), 5), dtype=np.int64)   # a c g t n per insertion column
    runs = np.zeros(c.sites.shape[0], dtype=np.int64)
    checked = 0
    for k, (a, g, w0, w1) in enumerate(c.items.tolist()):
        text = c.rows[int(c.row_first[k]):int(c.row_first[k + 1])].tobytes()
        assert len(text) == len(kinds[g])
        for ch, (u, j) in zip(text, kinds[g]):
            if j < 0:
                assert ch in b'ACGTN-.'   # a target column never holds a lower-case letter
                if ch != ord('.'):
                    tcount[int(col_first[g]) + u - int(c.windows[g, 1]), b'ACGTN-'.index(ch)] += 1
            else:
                assert ch in b'acgtn.'    # an insertion column never holds '-' or an upper-case letter
                if ch != ord('.'):
                    icount[int(icol_first[u]) + j, b'acgtn'.index(ch)] += 1
                    runs[u] += j == 0
        r = c.res[k]
        if r['bases'] and not r['hidden']:
            q0 = int(c.blocks[int(c.first[a])]['q'])
            whole = qrow[int(row_first[a]):int(row_first[a + 1])].tobytes().replace(b'-', b'')
            assert text.replace(b'.', b'').replace(b'-', b'').upper() == whole[int(r['q_lo']) - q0:int(r['q_hi']) - q0]
            checked += 1
    for k, f in enumerate(('a', 'c', 'g', 't', 'n', 'del')):
        assert (cols[f].astype(np.int64) == tcount[:, k]).all(), f
    for k, f in enumerate(('a', 'c', 'g', 't', 'n')):
        assert (icols[f].astype(np.int64) == icount[:, k]).all(), f
    assert (ires['runs'].astype(np.int64) == runs).all()
    assert checked >= 30 and tcount.sum() > 1000 and icount.sum() > 1000 and runs.sum() >= 10 and (tcount.sum(axis=0) > 0).all() and (icount.sum(axis=0) > 0).all()


SETTINGS = ({'MIMEO_PATH_STACK_SLICE_BLOCKS': '1'}, {'MIMEO_PATH_STACK_BATCH_BYTES': '1'}, {'MIMEO_PATH_STACK_JOB_COLUMNS': '1'}, {'MIMEO_PATH_LAUNCH_JOBS': '5'},
            {'MIMEO_PATH_STACK_SLICE_BLOCKS': '1', 'MIMEO_PATH_STACK_BATCH_BYTES': '1', 'MIMEO_PATH_STACK_JOB_COLUMNS': '1'})


def test_every_setting_gives_the_same_bytes(eng, made, monkeypatch, capfd):
    """the whole case with every alignment a slice of its own, every row a batch of its own, every column a job of its own, five
    jobs per launch, and the first three at once: the bytes of the call under the defaults.  The switches are read per call.  Four
    records have items, the one without blocks among them: its rows of '.' are made on the device like every other."""
    c = made
    said = []
    for e in ({},) + SETTINGS:
        with monkeypatch.context() as m:
            m.setenv('MIMEO_PATH_STACK_STATS', '1')
            for name, v in e.items():
                m.setenv(name, v)
            capfd.readouterr()
            res, row_first, rows = eng.stack(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items, c.sites)
            err = capfd.readouterr().err
        assert rows.tobytes() == c.rows.tobytes() and res.tobytes() == c.res.tobytes() and row_first.tobytes() == c.row_first.tobytes(), e
        m = re.search(r'\[k15\] stack: (\d+) items, (\d+) sites, (\d+) bytes, (\d+) jobs, slices (\d+), batches (\d+), launches (\d+), kernels', err)
        assert m, err
        said.append(dict(zip(('items', 'sites', 'bytes', 'jobs', 'slices', 'batches', 'launches'), (int(x) for x in m.groups()))))
    plain, slice1, batch1, job1, launch5, smallest = said
    nrows = int((np.diff(c.row_first.astype(np.int64)) > 0).sum())
    assert plain['items'] == c.items.shape[0] and plain['sites'] == c.sites.shape[0] and plain['bytes'] == c.rows.size
    assert plain['slices'] == 1 and plain['batches'] == 1 and plain['jobs'] == nrows and plain['launches'] == 1
    assert slice1['slices'] == 4 and slice1['batches'] == 4 and batch1['batches'] == nrows and job1['jobs'] == c.rows.size
    assert launch5['launches'] == (nrows + 4) // 5 and smallest['batches'] == nrows and smallest['jobs'] == c.rows.size and smallest['slices'] == 4


def test_errors_and_degenerate_calls(eng, made):
    c = made
    recs, first, blocks = c.recs, c.first, c.blocks
    windows = [(0, 40, 230), (0, 100, 100), (2, 0, 100)]
    items = [(0, 0, 50, 212), (1, 0, 80, 120), (3, 2, 0, 100)]
    sites = [(0, 80, 5, 0), (0, 135, 7, 0), (2, 30, 64, 0)]
    ok = eng.stack(c.G, None, recs, first, blocks, windows, items, sites)
    same(ok, restate(c.seqs, recs, first, blocks, windows, items, sites), 'the valid call')

    def bad(match, windows=windows, items=items, sites=sites, recs=recs, first=first, blocks=blocks):
        with pytest.raises(RuntimeError, match=r'libmimeo_hip: mimeo_path_stack: ' + match) as e:
            eng.stack(c.G, None, recs, first, blocks, windows, items, sites)
        assert '(code -1)' in str(e.value)   # MIMEO_ERR_ARG

    def edit(rows, i, k, v):
        rows = [list(r) for r in rows]
        rows[i][k] = v
        return rows

    # everything mimeo_path_insertions checks, under this name and in its order: the paths, the windows, the items, the sites
    blk = blocks.copy()
    blk['len'][1] = 0
    bad(r'record 0, block 1 .*len is 0', blocks=blk)
    r2 = recs.copy()
    r2['qid'][1] = 3
    bad(r'record 1: qid is not a scaffold', recs=r2)
    bad(r'window 2 \(tid 3, \[0, 100\)\): tid is not a scaffold', windows=edit(windows, 2, 0, 3))
    bad(r'window 1 \(tid 0, \[101, 100\)\): start is beyond end', windows=edit(windows, 1, 1, 101))
    bad(r'window 2 \(tid 2, \[0, 301\)\): end is beyond its scaffold', windows=edit(windows, 2, 2, 301))
    bad(r'item 1 \(aln 4, window 0, \[80, 120\)\): aln is not a record', items=edit(items, 1, 0, 4))
    bad(r'item 2 \(aln 3, window 3, .*window is not below nwin', items=edit(items, 2, 1, 3))
    bad(r"item 2 \(aln 3, window 0, .*does not lie on the record's target scaffold", items=edit(items, 2, 1, 0))
    bad(r'item 0 \(aln 0, window 0, \[213, 212\)\): w0 is beyond w1', items=edit(items, 0, 2, 213))
    bad(r'item 0 .*\[39, 212\)\): \[w0, w1\) does not lie inside the window', items=edit(items, 0, 2, 39))
    bad(r'site 2 \(window 3, x 30, ncols 64\): window is not below nwin', sites=edit(sites, 2, 0, 3))
    bad(r'site 0 \(window 0, x 39, ncols 5\): x does not lie inside the window', sites=edit(sites, 0, 1, 39))
    bad(r'site 1 \(window 1, x 100, ncols 7\): x does not lie inside the window', sites=edit(edit(sites, 1, 0, 1), 1, 1, 100))   # an empty window holds no site
    bad(r'site 2 \(window 2, x 30, ncols 0\): ncols is not in 1 \.\. 1024', sites=edit(sites, 2, 2, 0))
    bad(r'site 2 \(window 2, x 30, ncols 1025\): ncols is not in 1 \.\. 1024', sites=edit(sites, 2, 2, 1025))
    bad(r'site 1 \(window 0, x 80, ncols 7\): the sites are not strictly increasing', sites=edit(sites, 1, 1, 80))
    bad(r'item 1 .*aln is not a record', items=edit(items, 1, 0, 4), sites=edit(sites, 0, 2, 0))   # a bad item is named before a bad site
    # the checks run for a call without items too
    bad(r'site 2 .*ncols is not in 1 \.\. 1024', items=np.zeros((0, 4)), sites=edit(sites, 2, 2, 0))
    # voters is not read
    again = eng.stack(c.G, None, recs, first, blocks, windows, items, edit(edit(sites, 0, 3, 0xFFFFFFFF), 1, 3, 9))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, ok))
    # nitems == 0: one zero, no rows — also without a single record
    for r, f, b in ((recs, first, blocks), (recs[:0], first[:1], blocks[:0])):
        res, row_first, rows = eng.stack(c.G, None, r, f, b, windows, np.zeros((0, 4)), sites)
        assert res.size == 0 and res.dtype == _ffi.STACK_ROW and row_first.tolist() == [0] and rows.size == 0 and rows.dtype == np.uint8
    # items whose windows have no column: rows of no byte
    res, row_first, rows = eng.stack(c.G, None, recs, first, blocks, windows, [(0, 1, 100, 100)] * 2, sites)
    assert row_first.tolist() == [0, 0, 0] and rows.size == 0 and not res.tobytes().strip(b'\0')
    # nsites == 0: a stack without insertion columns
    got = eng.stack(c.G, None, recs, first, blocks, windows, items, np.zeros((0, 4)))
    exp = restate(c.seqs, recs, first, blocks, windows, items, np.zeros((0, 4)))
    same(got, exp, 'no site')
    assert got[1].tolist() == [0, 190, 380, 480] and got[0]['hidden'].tolist() == [20, 5, 1050] and not any(ch in exp[2] for ch in b'acgtn')
    # Q given as a genome of its own, with the query scaffolds in another order
    B = eng.Genome(['p2', 'p0', 'p1'], [c.seqs[2], c.seqs[0], c.seqs[1]])
    r2 = recs.copy()
    r2['qid'] = (recs['qid'] + 1) % 3
    other = eng.stack(c.G, B, r2, first, blocks, windows, items, sites)
    B.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(other, ok))


# ---- end to end ------------------------------------------------------------------------------------------------------------

FAM_LEN = (600, 400, 500)
DEL_LEN, FLANK, NSCAF = 12, 15, 5


def family_genome(seed=15, div=0.08):
    """Five scaffolds of 12 kbp of random sequence, each with one copy of three families (600, 400 and 500 bp) in the same order,
    3000 bp apart, every copy with independent substitutions at 8 per cent; the last scaffold is reverse-complemented as a
    whole.  The engine chains like lastz --chain, so of every other scaffold one row lies over a copy: four rows and the
    scaffold's own diagonal.  Every copy of family 0 carries one private deletion of DEL_LEN bases at a family offset of its own,
    built as in tests/test_gpu_insertions.py: the FLANK bases on either side are free of substitutions in every copy, and the
    segment's first base differs from the base that follows the segment and its last base from the base in front of it, so the
    placement of the gap in an alignment is unique.  Whichever copy represents family 0, its four rows insert the twelve bases."""
    rng = np.random.Generator(np.random.PCG64(seed))
    codes = [rng.integers(0, 4, size=12_000, dtype=np.uint8) for _ in range(NSCAF)]
    fams = [rng.integers(0, 4, size=n, dtype=np.uint8) for n in FAM_LEN]
    offs, clean = [], np.zeros(FAM_LEN[0], dtype=bool)
    for k in range(NSCAF):
        o = 60 + 90 * k
        while fams[0][o] == fams[0][o + DEL_LEN] or fams[0][o + DEL_LEN - 1] == fams[0][o - 1]:
            o += 1
        assert o < 60 + 90 * k + 15
        offs.append(o)
        clean[o - FLANK:o + DEL_LEN + FLANK] = True
    for s in range(NSCAF):
        for f in range(3):
            cp = fams[f].copy()
            sub = rng.random(cp.size) < div
            if f == 0:
                sub &= ~clean
            cp[sub] = (cp[sub] + rng.integers(1, 4, size=int(sub.sum()), dtype=np.uint8)) % 4
            if f == 0:
                cp = np.concatenate([cp[:offs[s]], cp[offs[s] + DEL_LEN:]])
            p = 1500 + 3000 * f + int(rng.integers(0, 300))
            codes[s][p:p + cp.size] = cp
    codes[-1] = (3 - codes[-1])[::-1]
    return ['fs%d' % s for s in range(NSCAF)], [ACGT[c] for c in codes]


def _stockholm(path):
    """the blocks of a Stockholm file: [(ID, the DE fields, [(name, text)], RF, cons)]"""
    blocks, cur = [], None
    for line in open(path).read().splitlines():
        if line == '# STOCKHOLM 1.0':
            assert cur is None
            cur = {'rows': []}
        elif line == '//':
            blocks.append(cur)
            cur = None
        elif line.startswith('#=GF ID '):
            cur['id'] = line[8:]
        elif line.startswith('#=GF DE '):
            cur['de'] = line[8:]
        elif line.startswith('#=GC RF '):
            cur['rf'] = line[8:]
        elif line.startswith('#=GC cons '):
            cur['cons'] = line[10:]
        else:
            assert not line.startswith('#'), line
            name, text = line.split(' ')
            cur['rows'].append((name, text))
    assert cur is None
    return blocks


def test_cli_family_alignments_end_to_end(eng, tmp_path):
    """Observed on the MI355X with this genome: three blocks F1, F2, F3 of five members and five sequence rows each (the
    representative's own and one from every other scaffold, those of fs4 on the minus strand), 610, 455 and 509 columns for
    representatives of 593, 438 and 502 bases: F1's insertion columns hold the twelve bases of its private deletion."""
    from mimeo_amd import run_self, workflow
    from tests.test_gpu_insertions import _fasta
    names, seqs = family_genome()
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    plain, sto = tmp_path / 'plain', tmp_path / 'sto'
    run_self.main(['--afasta', fa, '-d', str(plain), '--loglevel', 'WARNING', '--consensus', str(plain / 'lib.fa'), '--consensusInsertions'])
    run_self.main(['--afasta', fa, '-d', str(sto), '--loglevel', 'WARNING', '--consensus', str(sto / 'lib.fa'), '--consensusInsertions', '--familyAlignments',
                   str(sto / 'fam.sto')])
    # TAB, GFF3 and library are what a run without the flag writes
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3', 'lib.fa'):
        assert (sto / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(os.listdir(sto)) == sorted(os.listdir(plain) + ['fam.sto'])
    # the flag alone, with a budget of one row per engine.stack call and small runs of windows: the same file
    A = eng.Genome.from_fasta([fa], None)
    args = run_self.mainArgs(['--afasta', fa])
    try:
        workflow.self_repeats(A, workflow.all_pairs(len(A.names)), str(tmp_path / 'b.tab'), str(tmp_path / 'b.gff3'), prefix=args.prefix, label=args.label,
                              family_alignments=str(tmp_path / 'b.sto'), consensus_budget=700, stack_budget=1)
    finally:
        A.close()
    assert (tmp_path / 'b.sto').read_bytes() == (sto / 'fam.sto').read_bytes()
    assert (tmp_path / 'b.tab').read_bytes() == (plain / 'mimeo_alignment.tab').read_bytes()
    records, blocks = _fasta(sto / 'lib.fa'), _stockholm(sto / 'fam.sto')
    assert len(blocks) == len(records) >= 3
    opened = minus = 0
    for (head, seq), b in zip(records, blocks):
        print(b['id'], b['de'], [n for n, _ in b['rows']])
        assert head.split()[0] == '>' + b['id'] and head.split()[1:3] == b['de'].split()[:2]   # the same ID, representative and position
        de = dict(x.split('=') for x in b['de'].split() if '=' in x)
        width = int(de['columns'])
        assert int(de['rows']) == len(b['rows']) and de['members'] == dict(x.split('=') for x in head.split()[1:] if '=' in x)['members']
        assert all(len(text) == width for _, text in b['rows']) and len(b['rf']) == width == len(b['cons'])
        assert b['cons'].replace('.', '').replace('-', '') == seq
        assert len({n for n, _ in b['rows']}) == len(b['rows'])
        # the representative's own row: its letters at the x columns, '.' elsewhere
        seqid, span = b['de'].split()[1].split(':')
        start, end = (int(x) for x in span.split('-'))
        own_name, own = b['rows'][0]
        assert own_name == '%s/%d-%d' % (seqid, start + 1, end) and b['rf'].count('x') == end - start and set(b['rf']) <= set('x.')
        assert ''.join(ch for ch, r in zip(own, b['rf']) if r == 'x') == seqs[names.index(seqid)][start:end].tobytes().decode()
        assert all(ch == '.' for ch, r in zip(own, b['rf']) if r == '.')
        for name, text in b['rows'][1:]:
            qname, span = name.rsplit('/', 1)
            s, e = (int(x) for x in span.split('.')[0].split('-'))
            q = seqs[names.index(qname)]
            want = q[s - 1:e].tobytes().decode() if s <= e else revcomp(q[e - 1:s]).tobytes().decode()
            minus += s > e
            # no insertion column of the file is empty, so no base is hidden: the row's letters are the named stretch
            assert text.replace('.', '').replace('-', '').upper() == want, name
            assert all((ch in 'acgtn.') if r == '.' else (ch in 'ACGTN-.') for ch, r in zip(text, b['rf']))
        for j, r in enumerate(b['rf']):   # no insertion column is empty
            if r == '.':
                assert any(text[j] != '.' for _, text in b['rows'][1:]), (b['id'], j)
        opened += b['rf'].count('.') >= DEL_LEN
    assert opened >= 1 and minus >= 3
