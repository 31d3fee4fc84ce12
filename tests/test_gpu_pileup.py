"""Column pileup and consensus (mimeo_path_pileup, kernels K13; engine.pileup; `mimeo self --consensus`) against a plain numpy
restatement of "pileup v1" (include/mimeo_hip.h), written here from the header's rules alone: per item and block the query
letters of the block's columns inside the window, the deleted bases of the gap in front of it and the insertion at its start;
the call from the votes of a column.  Equality is exact, counter by counter and byte by byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi
from mimeo_amd.synth import write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('a', 'c', 'g', 't', 'n', 'del', 'ins_runs', 'ins_bases')
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

def restate_counts(seqs, recs, first, blocks, windows, items):
    """(ncols, 8) counts in the order of mimeo_pileup_column.  seqs: the scaffolds as uint8 letters; windows: rows of (tid,
    start, end); items: rows of (aln, window, w0, w1)."""
    win = np.asarray(windows, dtype=np.int64).reshape(-1, 3)
    col_first = np.concatenate([[0], np.cumsum(win[:, 2] - win[:, 1])])
    cols = np.zeros((int(col_first[-1]), 8), dtype=np.int64)
    rc = {}
    for a, g, w0, w1 in np.asarray(items, dtype=np.int64).reshape(-1, 4).tolist():
        qid, strand = int(recs[a]['qid']), int(recs[a]['qstrand'])
        if strand and qid not in rc:
            rc[qid] = revcomp(seqs[qid])
        Q = rc[qid] if strand else seqs[qid]
        base = int(col_first[g]) - int(win[g, 1])   # entry of target base x: base + x
        prev = None
        for t, q, ln in blocks[int(first[a]):int(first[a + 1])].tolist():
            if prev is not None:
                p, dq = prev[0], q - prev[1]
                lo, hi = max(p, w0), min(t, w1)
                if hi > lo:
                    cols[base + lo:base + hi, 5] += 1
                if dq > 0 and w0 <= p < w1:
                    cols[base + p, 6] += 1
                    cols[base + p, 7] += dq
            lo, hi = max(t, w0), min(t + ln, w1)
            if hi > lo:
                y = CODE[Q[q + (lo - t):q + (hi - t)]]
                np.add.at(cols, (base + np.arange(lo, hi), y), 1)
            prev = (t + ln, q + ln)
    return cols


def restate_call(seqs, windows, cols):
    """the call byte of every column, from the votes"""
    out = []
    at = 0
    for tid, start, end in np.asarray(windows, dtype=np.int64).reshape(-1, 3).tolist():
        for x in range(start, end):
            c = cols[at]
            at += 1
            x0 = int(CODE[seqs[tid][x]])
            v = [int(c[b]) + (1 if x0 == b else 0) for b in range(4)]
            vd = int(c[5])
            top = max(v)
            if vd > top:
                out.append(ord('-'))
            elif top == 0:
                out.append(ord('N'))
            else:
                out.append(b'ACGT'[x0 if x0 < 4 and v[x0] == top else v.index(top)])
    return np.array(out, dtype=np.uint8)


def test_restatement_on_paper():
    """The restatement itself, on a path small enough to count by hand"""
    T = np.frombuffer(b'AAAAACCCCCGGGGGTTTTTAAAAANNNNN', dtype=np.uint8)
    Q = np.frombuffer(b'AAGAACCTTACGTGNGGGTTCCAAAAA', dtype=np.uint8)
    #  block 0: t 0..5 over q 0..5 AAGAA; 2 inserted query bases in front of target base 5
    #  block 1: t 5..9 over q 7..11 TTAC; then target bases 9 and 10 deleted and query base 11 inserted: both jump, p = 9
    #  block 2: t 11..15 over q 12..16 TGNG
    recs = np.zeros(1, dtype=_ffi.ALIGNMENT)
    recs['qid'] = 1
    blk = np.array([(0, 0, 5), (5, 7, 4), (11, 12, 4)], dtype=_ffi.PATH_BLOCK)
    first = np.array([0, 3], dtype=np.uint64)
    c = restate_counts([T, Q], recs, first, blk, [(0, 0, 20)], [(0, 0, 0, 20)])
    letters = lambda c: ''.join('acgtnd'[int(np.argmax(r[:6]))] if r[:6].sum() else '.' for r in c)
    assert letters(c) == 'aagaattacddtgng.....' and c[:, :6].sum() == 15
    assert c[:, 6].tolist() == [0] * 5 + [1, 0, 0, 0, 1] + [0] * 10 and c[:, 7].tolist() == [0] * 5 + [2, 0, 0, 0, 1] + [0] * 10
    # a window [5, 9): the insertion at p = 5 == w0 is counted, the one at p = 9 == w1 is not; [9, 10): one deleted base of two
    c = restate_counts([T, Q], recs, first, blk, [(0, 3, 12)], [(0, 0, 5, 9)])
    assert letters(c) == '..ttac...' and c[:, 6].tolist() == [0, 0, 1, 0, 0, 0, 0, 0, 0]
    c = restate_counts([T, Q], recs, first, blk, [(0, 9, 10)], [(0, 0, 9, 10)])
    assert c.tolist() == [[0, 0, 0, 0, 0, 1, 1, 1]]
    # the call: own base A under g: a tie, the own base wins; own C under t, t: T; deleted G: vd = 1 ties with the own base: G
    c = restate_counts([T, Q], recs, first, blk, [(0, 0, 20)], [(0, 0, 0, 20), (0, 0, 5, 7)])
    assert restate_call([T, Q], [(0, 0, 20)], c).tobytes() == b'AAAAATTCCCGGGGGTTTTT'
    c = restate_counts([T, Q], recs, first, blk, [(0, 0, 20)], [(0, 0, 0, 20)] * 2)
    assert restate_call([T, Q], [(0, 0, 20)], c).tobytes() == b'AAGAATTAC--TGGGTTTTT'   # ... twice: the pile outvotes the own base; n never votes


# ---- made-up paths ---------------------------------------------------------------------------------------------------------

L = (6000, 5000, 4000)
MODS = tuple(range(33)) + (63,)
PATH4 = [(500, 300, 100), (600, 405, 100), (720, 505, 80), (830, 600, 60)]   # an insertion of 5 at 600, a deletion [700, 720), both at 800: 15 / 30
BIG = [(1000, 100, 500), (1600, 700, 600), (2300, 1310, 748), (3048, 2070, 400), (3500, 2470, 300)]
BIG2 = [(1900, 50, 100), (2050, 150, 200), (2250, 360, 1500)]
TILE_EDGES = (2024, 3048)   # of the window [1000, 4000) in tiles of 1024 columns


def _genome():
    rng = np.random.default_rng(130)
    s = [ACGT[rng.integers(0, 4, n)].copy() for n in L]
    s[0][2000:2010] = ord('N')     # N in the target, inside the 3 000-column window and under BIG2's deletion's neighbourhood
    s[0][570:573] = ord('n')
    s[0][3050] = ord('R')          # an IUPAC code is an N to the engine
    s[1][350:360] = ord('N')       # N in the query: under PATH4 on the plus strand ...
    s[1][4500:4510] = ord('N')     # ... and on the minus strand (reverse-complement bases 490 .. 499)
    s[2][800:830] = ord('N')       # under BIG's block that crosses a tile edge
    s[2][1500:1520] += 32          # soft-masked
    # the designed piles of test_call_rule: the query letters A C G T N at scaffold 1 [4900, 4905)
    s[1][4900:4905] = np.frombuffer(b'ACGTN', dtype=np.uint8)
    s[2][3500:3540] = np.frombuffer(b'TTTTCTTTNTTTNTTTGTTTATTTGTTTNTTTTTTTNTTT', dtype=np.uint8)
    return ['p0', 'p1', 'p2'], s


class Case:
    def __init__(self):
        self.names, self.seqs = _genome()
        self.recs, self.first, self.blocks = [], [0], []
        self.windows, self.items, self.what = [], [], {}

    def add(self, tid, qid, strand, blk):
        t_end = q_end = 0
        for t, q, ln in blk:   # the contract of mimeo_path_block, so that a slip in a table is not taken for a kernel's
            assert ln >= 1 and t >= t_end and q >= q_end and t + ln <= L[tid] and q + ln <= L[qid], (t, q, ln)
            t_end, q_end = t + ln, q + ln
        self.recs.append((tid, qid, strand))
        self.blocks.extend(blk)
        self.first.append(len(self.blocks))
        return len(self.recs) - 1

    def window(self, what, tid, start, end, items):
        """a window and its items (aln, w0, w1); `what` names the case of the issue's list that it covers"""
        g = len(self.windows)
        self.windows.append((tid, start, end))
        self.what.setdefault(what, []).append(g)
        for a, w0, w1 in items:
            assert self.recs[a][0] == tid and start <= w0 <= w1 <= end
            self.items.append((a, g, w0, w1))
        return g

    def finish(self):
        r = np.zeros(len(self.recs), dtype=_ffi.ALIGNMENT)
        r['tid'], r['qid'], r['qstrand'] = [x[0] for x in self.recs], [x[1] for x in self.recs], [x[2] for x in self.recs]
        self.recs, self.first, self.blocks = r, np.array(self.first, dtype=np.uint64), np.array(self.blocks, dtype=_ffi.PATH_BLOCK)
        self.windows = np.array(self.windows, dtype=np.int64)
        self.items = np.array(self.items, dtype=np.int64)
        self.col_first = np.concatenate([[0], np.cumsum(self.windows[:, 2] - self.windows[:, 1])])
        return self

    def cols_of(self, cols, g):
        return cols[int(self.col_first[g]):int(self.col_first[g + 1])]


def made_case():
    c = Case()
    rng = np.random.default_rng(131)
    plus, minus = c.add(0, 1, 0, PATH4), c.add(0, 1, 1, PATH4)
    for what, s, e in (('a window starting mid-block', 550, 650), ('a window starting inside a deletion', 710, 760),
                       ('a window wholly inside a deletion', 703, 715), ('a window off the alignment', 100, 200), ('an empty window', 640, 640),
                       ('an insertion with p_k == w0, counted', 600, 650), ('an insertion with p_k == w1, not counted', 560, 600),
                       ('a both-jump gap', 790, 840), ('a minus-strand query', 450, 950), ('N in the query', 520, 720)):
        c.window(what, 0, s, e, [(plus, s, e), (minus, s, e)])
    c.what['N in the target'] = c.what['a window starting mid-block'][:1]   # target bases 570 .. 572 are n: they play no part in the counts
    # overlapping windows, and one record in two windows: [550, 650) above and these, the second with items clipped inside it
    c.window('overlapping windows, one record in two windows', 0, 600, 700, [(plus, 600, 700)])
    c.window('overlapping windows, one record in two windows', 0, 400, 1000, [(plus, 450, 650), (plus, 650, 900), (minus, 400, 1000)])
    # 3 000 columns: tiles [1000, 2024), [2024, 3048), [3048, 4000).  BIG: a block [1600, 2200) over the first edge, a block that
    # ends on the second edge and an insertion of 12 in front of base 3048, the first column of the third tile.  BIG2: a deletion
    # [2000, 2050) over the first edge, and a block [2250, 3750) over the second
    big, big2 = c.add(0, 2, 0, BIG), c.add(0, 2, 1, BIG2)
    assert BIG[1][0] < TILE_EDGES[0] < BIG[1][0] + BIG[1][2] and BIG[2][0] + BIG[2][2] == TILE_EDGES[1] == BIG[3][0] and BIG[3][1] - (BIG[2][1] + BIG[2][2]) == 12
    assert BIG2[0][0] + BIG2[0][2] < TILE_EDGES[0] < BIG2[1][0] and BIG2[2][0] < TILE_EDGES[1] < BIG2[2][0] + BIG2[2][2]
    c.window('a window of 3 000 columns', 0, 1000, 4000, [(big, 1000, 4000), (big2, 1000, 4000), (big, 2500, 3048), (big, 3048, 3500)])
    # one block of 150 columns from every target start and every query start of MODS mod 64, on both strands, each in a window
    # that cuts it one base short on either side
    for m in MODS:
        for strand in (0, 1):
            for t, q in ((64 * 5 + m, 64 * 7 + (5 * m + 1) % 64), (64 * 9 + 5, 64 * 3 + m)):
                a = c.add(2, 1, strand, [(t, q, 150)])
                c.window('starts at every residue', 2, t - 2 * (m & 1), t + 149, [(a, t + 1, t + 149)])
    # a record without blocks
    e = c.add(1, 2, 0, [])
    c.window('a record without blocks', 1, 100, 300, [(e, 100, 300)])
    # 300 items on one tile, of both strands
    c.window('300 items on one tile', 0, 480, 900, [((plus, minus)[k & 1],) + tuple(sorted(rng.integers(480, 901, 2).tolist())) for k in range(300)])
    # a window that nobody names
    c.window('no item', 1, 4890, 4910, [])
    return c.finish()


LIST = ('a window starting mid-block', 'a window starting inside a deletion', 'a window wholly inside a deletion', 'a window off the alignment',
        'an empty window', 'a window of 3 000 columns', 'an insertion with p_k == w0, counted', 'an insertion with p_k == w1, not counted',
        'a both-jump gap', 'starts at every residue', 'a minus-strand query', 'N in the query', 'N in the target', 'a record without blocks',
        'overlapping windows, one record in two windows', '300 items on one tile')


@pytest.fixture(scope='module')
def made(eng):
    c = made_case()
    c.exp = restate_counts(c.seqs, c.recs, c.first, c.blocks, c.windows, c.items)   # once, shared, and left as it is
    c.exp.setflags(write=False)
    c.exp_call = restate_call(c.seqs, c.windows, c.exp)
    c.G = eng.Genome(c.names, c.seqs)
    c.cols, c.call = eng.pileup(c.G, None, c.recs, c.first, c.blocks, c.windows, c.items)
    yield c
    c.G.close()


def same(cols, exp, tag):
    assert cols.dtype == _ffi.PILEUP_COLUMN and cols.shape == (exp.shape[0],), tag
    for k, f in enumerate(FIELDS):
        bad = np.flatnonzero(cols[f].astype(np.int64) != exp[:, k])
        assert bad.size == 0, (tag, f, bad[:5], cols[f][bad[:5]], exp[bad[:5], k])


def test_made_up_paths_against_the_restatement(made):
    c = made
    assert set(LIST) <= set(c.what)
    same(c.cols, c.exp, 'made-up paths')
    assert c.call.dtype == np.uint8 and c.call.tobytes() == c.exp_call.tobytes()
    # not vacuous: every counter occurs, every letter is called
    assert (c.exp.sum(axis=0) > 0).all() and set(c.exp_call.tobytes()) == set(b'ACGTN-')
    of = lambda what, k=0: c.cols_of(c.exp, c.what[what][k])
    depth = lambda e: e[:, :6].sum(axis=1)
    # the list, item by item, on the restatement's side: each case is what its name says
    assert depth(of('a window starting mid-block')).tolist() == [2] * 100 and of('a window starting mid-block')[50, 6:].tolist() == [2, 10]
    assert of('a window starting inside a deletion')[:, 5].tolist() == [2] * 10 + [0] * 40
    assert of('a window wholly inside a deletion')[:, 5].tolist() == [2] * 12 and of('a window wholly inside a deletion')[:, :5].sum() == 0
    assert of('a window off the alignment').sum() == 0 and of('a window off the alignment').shape[0] == 100
    assert of('an empty window').shape[0] == 0
    assert of('an insertion with p_k == w0, counted')[0, 6:].tolist() == [2, 10] and of('an insertion with p_k == w1, not counted')[:, 6:].sum() == 0
    both = of('a both-jump gap')
    assert both[10, 5:].tolist() == [2, 2, 30] and both[10:40, 5].tolist() == [2] * 30 and both[:, 6].sum() == 2
    assert of('N in the query')[:, 4].sum() == 20 and of('a record without blocks').sum() == 0 and of('no item').sum() == 0
    big = of('a window of 3 000 columns')
    assert big.shape[0] == 3000
    e0, e1 = (e - 1000 for e in TILE_EDGES)
    assert depth(big)[e0 - 1:e0 + 1].tolist() == [2, 2] and big[e0 - 1:e0 + 1, 5].tolist() == [1, 1]       # a block and a deletion over the first edge
    assert big[e1, 6:].tolist() == [2, 24] and big[e1 - 1, 6:].tolist() == [0, 0] and big[:, 6].sum() == 3 + 1 + 0 + 1   # the insertion at the edge: in its tile, once per item
    assert depth(big)[e1 - 1:e1 + 1].tolist() == [3, 3] and big[:, 4].sum() >= 30                              # the second edge; N in the query
    mods = [c.windows[g] for g in c.what['starts at every residue']]
    assert {int(w[1]) % 32 for w in mods} == set(range(32)) and len(mods) == 4 * len(MODS)
    assert {int(c.blocks[int(c.first[a])]['q']) % 64 for a in range(4 + 0, 4 + 4 * len(MODS))} >= {0, 1, 31, 32, 63}
    many = of('300 items on one tile')
    assert depth(many).max() > 100 and sum(1 for it in c.items if it[1] == c.what['300 items on one tile'][0]) == 300
    # what a caller may rely on: the counts are additive over a partition of an item's window — the two halves of [450, 900)
    # and the whole of it ...
    g = c.what['overlapping windows, one record in two windows'][1]
    whole = restate_counts(c.seqs, c.recs, c.first, c.blocks, c.windows, [(0, g, 450, 900), (1, g, 400, 1000)])
    assert (c.cols_of(whole, g) == c.cols_of(c.exp, g)).all()


CHILD = '''
import sys
import numpy as np
from mimeo_amd import engine
engine.init(0)
z = np.load(sys.argv[1])
G = engine.Genome(['p0', 'p1', 'p2'], [z['s0'], z['s1'], z['s2']])
cols, call = engine.pileup(G, None, z['recs'], z['first'], z['blocks'], z['windows'], z['items'])
only_cols, none = engine.pileup(G, None, z['recs'], z['first'], z['blocks'], z['windows'], z['items'], call=False)
assert none is None and only_cols.tobytes() == cols.tobytes()
none, only_call = engine.pileup(G, None, z['recs'], z['first'], z['blocks'], z['windows'], z['items'], counts=False)
assert none is None and only_call.tobytes() == call.tobytes()
np.savez(sys.argv[2], cols=cols, call=call)
'''
SETTINGS = ({}, {'MIMEO_PILEUP_JOB_ITEMS': '7'}, {'MIMEO_PILEUP_SLICE_BLOCKS': '1'}, {'MIMEO_PILEUP_COLUMNS': '1500'}, {'MIMEO_PATH_LAUNCH_JOBS': '3'})


def test_every_setting_gives_the_same_bytes(made, tmp_path):
    """the whole case under the defaults, 7 items per job, every alignment a slice of its own, batches of 1500 columns and three
    jobs per launch, each in a fresh child process: the bytes of this process's call"""
    c = made
    np.savez(tmp_path / 'in.npz', s0=c.seqs[0], s1=c.seqs[1], s2=c.seqs[2], recs=c.recs, first=c.first, blocks=c.blocks, windows=c.windows, items=c.items)
    (tmp_path / 'child.py').write_text(CHILD)
    base = dict(os.environ, MIMEO_PILEUP_STATS='1', PYTHONPATH=os.pathsep.join(p for p in (ROOT, os.environ.get('PYTHONPATH')) if p))
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
        assert got['cols'].tobytes() == c.cols.tobytes() and got['call'].tobytes() == c.call.tobytes(), SETTINGS[k]
        lines = [l for l in err.splitlines() if l.startswith('[k13]')]
        assert len(lines) == 3 and '%d items' % c.items.shape[0] in lines[0] and 'kernels' in lines[0], err
        m = re.search(r'(\d+) items, (\d+) windows, (\d+) columns, (\d+) tiles, (\d+) jobs, slices (\d+) of (\d+), batches (\d+), launches (\d+), kernels', lines[0])
        assert m, lines[0]
        said.append(dict(zip(('items', 'windows', 'columns', 'tiles', 'jobs', 'slices', 'of', 'batches', 'launches'), (int(x) for x in m.groups()))))
    # the statistics line says what each setting did
    plain, jobs7, slice1, cols1500, launch3 = said
    assert int(plain['batches']) == 1 and int(plain['slices']) == 1 and int(cols1500['batches']) > 10 and int(slice1['slices']) > 100
    assert int(jobs7['jobs']) >= int(plain['jobs']) + 300 // 7 - 300 // 64 - 1 and int(launch3['launches']) >= int(plain['jobs']) // 3
    assert plain['tiles'] == cols1500['tiles'] == slice1['tiles']


def test_second_witness_k10(eng, made):
    """summed over a window's columns the counts are what K10, an existing kernel, counts for the same items with one group per
    window"""
    c = made
    ws = eng.window_stats(c.G, None, c.recs, c.first, c.blocks, c.items.astype(np.uint32), len(c.windows))
    sums = np.zeros((len(c.windows), 8), dtype=np.int64)
    for g in range(len(c.windows)):
        got = c.cols_of(c.cols, g)
        sums[g] = [int(got[f].astype(np.int64).sum()) for f in FIELDS]
    k10 = {f: ws[f].astype(np.int64) for f in ws.dtype.names}
    assert (sums[:, :5].sum(axis=1) == k10['matches'] + k10['transitions'] + k10['transversions'] + k10['ambiguous']).all()
    assert (sums[:, 5] == k10['del_bases']).all() and (sums[:, 6] == k10['ins_runs']).all() and (sums[:, 7] == k10['ins_bases']).all()
    assert sums[:, 5].sum() > 100 and sums[:, 6].sum() > 10 and sums[:, :5].sum() > 50_000


def test_call_rule(eng, made):
    """designed piles, one column each, on scaffold 2 [3500, 3540): the own base every fourth column from 3504 on, the query
    letters A C G T N at scaffold 1 [4900, 4905)"""
    c = made
    q = {b: 4900 + k for k, b in enumerate('ACGTN')}
    recs, first, blocks, items = [], [0], [], []

    def pile(x, letters, dels=0):
        for b in letters:   # one column of one record each
            blocks.append((x, q[b], 1))
            first.append(len(blocks))
            items.append((len(recs), 0, x, x + 1))
            recs.append((2, 1, 0))
        for _ in range(dels):   # a record with target base x deleted, asked about x alone
            blocks.extend([(x - 1, q['A'], 1), (x + 1, q['A'] + 1, 1)])
            first.append(len(blocks))
            items.append((len(recs), 0, x, x + 1))
            recs.append((2, 1, 0))

    own = bytes(c.seqs[2][3500:3540])
    assert own == b'TTTTCTTTNTTTNTTTGTTTATTTGTTTNTTTTTTTNTTT'
    pile(3504, 'A')            # own C, one A: a tie, and the own base wins (the order alone would say A)
    pile(3508, 'CA')           # own N, A and C tie: A
    pile(3512, 'TG')           # own N, G and T tie: G
    pile(3516, '', dels=1)     # own G, a deletion ties with it: the base wins
    pile(3520, 'A', dels=2)    # own A and an A against two deletions: a tie, the base wins
    pile(3524, '', dels=2)     # own G, two deletions: strictly largest, '-'
    # 3528: an uncovered target N gives N
    pile(3532, 'NNN')          # own T covered by query N only: T
    pile(3536, 'N', dels=0)    # own N under a query N: no vote at all, N
    pile(3502, 'CC')           # own T, two C: the pile outvotes the own base
    pile(3506, 'N', dels=1)    # own T, an N and a deletion: 1 against 1, the base wins
    pile(3538, 'ACGT' * 2 + 'T', dels=3)   # own T: T 4, deletion 3, the others 2
    r = np.zeros(len(recs), dtype=_ffi.ALIGNMENT)
    r['tid'], r['qid'], r['qstrand'] = [x[0] for x in recs], [x[1] for x in recs], [x[2] for x in recs]
    first, blocks = np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK)
    cols, call = eng.pileup(c.G, None, r, first, blocks, [(2, 3500, 3540)], items)
    want = bytearray(own)
    for x, b in ((3504, 'C'), (3508, 'A'), (3512, 'G'), (3516, 'G'), (3520, 'A'), (3524, '-'), (3528, 'N'), (3532, 'T'), (3536, 'N'), (3502, 'C'), (3506, 'T'),
                 (3538, 'T')):
        want[x - 3500] = ord(b)
    assert call.tobytes() == bytes(want)
    exp = restate_counts(c.seqs, r, first, blocks, [(2, 3500, 3540)], items)
    same(cols, exp, 'call rule')
    assert restate_call(c.seqs, [(2, 3500, 3540)], exp).tobytes() == bytes(want)
    assert cols[24].tolist() == (0, 0, 0, 0, 0, 2, 0, 0) and cols[32].tolist() == (0, 0, 0, 0, 3, 0, 0, 0) and cols[38].tolist() == (2, 2, 2, 3, 0, 3, 0, 0)


def test_errors_and_edge_inputs(eng, made):
    c = made
    recs, first, blocks = c.recs[:5], c.first[:6], c.blocks[:int(c.first[5])]
    windows = [(0, 500, 900), (0, 1000, 1000), (2, 0, 4000)]
    items = [(0, 0, 550, 650), (1, 0, 500, 900), (2, 1, 1000, 1000), (4, 2, 300, 500)]
    assert [int(x) for x in recs['tid']] == [0, 0, 0, 0, 2]
    ok_cols, ok_call = eng.pileup(c.G, None, recs, first, blocks, windows, items)
    same(ok_cols, restate_counts(c.seqs, recs, first, blocks, windows, items), 'the valid call')

    def bad(match, windows=windows, items=items, recs=recs, first=first, blocks=blocks):
        with pytest.raises(RuntimeError, match=r'libmimeo_hip: mimeo_path_pileup: ' + match) as e:
            eng.pileup(c.G, None, recs, first, blocks, windows, items)
        assert '(code -1)' in str(e.value)   # MIMEO_ERR_ARG

    def edit(rows, i, k, v):
        rows = [list(r) for r in rows]
        rows[i][k] = v
        return rows

    # everything mimeo_path_stats checks, under this name
    blk = blocks.copy()
    blk['len'][1] = 0
    bad(r'record 0, block 1 .*len is 0', blocks=blk)
    r2 = recs.copy()
    r2['qid'][1] = 3
    bad(r'record 1: qid is not a scaffold', recs=r2)
    f2 = first.copy()
    f2[-1] += 1
    bad(r'record 4: path_first\[n\] is not nblocks', first=f2)
    # windows
    bad(r'window 2 \(tid 3, \[0, 4000\)\): tid is not a scaffold', windows=edit(windows, 2, 0, 3))
    bad(r'window 1 \(tid 0, \[1001, 1000\)\): start is beyond end', windows=edit(windows, 1, 1, 1001))
    bad(r'window 2 \(tid 2, \[0, 4001\)\): end is beyond its scaffold', windows=edit(windows, 2, 2, 4001))
    # items
    bad(r'item 1 \(aln 5, window 0, \[500, 900\)\): aln is not a record', items=edit(items, 1, 0, 5))
    bad(r'item 3 \(aln 4, window 3, .*window is not below nwin', items=edit(items, 3, 1, 3))
    bad(r"item 3 \(aln 4, window 0, .*does not lie on the record's target scaffold", items=edit(items, 3, 1, 0))
    bad(r'item 0 \(aln 0, window 0, \[651, 650\)\): w0 is beyond w1', items=edit(items, 0, 2, 651))
    bad(r'item 0 .*\[499, 650\)\): \[w0, w1\) does not lie inside the window', items=edit(items, 0, 2, 499))
    bad(r'item 1 .*\[500, 901\)\): \[w0, w1\) does not lie inside the window', items=edit(items, 1, 3, 901))
    with pytest.raises(ValueError):
        eng.pileup(c.G, None, recs, first[:-1], blocks, windows, items)
    # nothing was launched and nothing is broken: the valid call answers as before
    again = eng.pileup(c.G, None, recs, first, blocks, windows, items)
    assert again[0].tobytes() == ok_cols.tobytes() and again[1].tobytes() == ok_call.tobytes()
    # nwin == 0: MIMEO_OK at once, nothing is looked at, not even a bad item
    cols, call = eng.pileup(c.G, None, recs, first, blocks, np.zeros((0, 3)), [(99, 0, 0, 0)])
    assert cols.size == 0 and cols.dtype == _ffi.PILEUP_COLUMN and call.size == 0 and call.dtype == np.uint8
    # nitems == 0: zero counts, and the call is the target's own letters — also without a single record
    for r, f, b in ((recs, first, blocks), (recs[:0], first[:1], blocks[:0])):
        cols, call = eng.pileup(c.G, None, r, f, b, [(0, 560, 580), (0, 3040, 3060), (0, 1990, 2020)], np.zeros((0, 4)))
        assert cols.size == 70 and not cols.tobytes().strip(b'\0')
        own = np.concatenate([c.seqs[0][560:580], c.seqs[0][3040:3060], c.seqs[0][1990:2020]])
        assert call.tobytes() == bytes(b'ACGTN'[int(CODE[x])] for x in own) and call.tobytes().count(b'N') == 3 + 1 + 10
    # only empty windows: no column, with or without items
    cols, call = eng.pileup(c.G, None, recs, first, blocks, [(0, 600, 600), (2, 4000, 4000)], [(0, 0, 600, 600)])
    assert cols.size == 0 and call.size == 0
    # Q given as a genome of its own, with the query scaffolds in another order
    B = eng.Genome(['p2', 'p0', 'p1'], [c.seqs[2], c.seqs[0], c.seqs[1]])
    r2 = recs.copy()
    r2['qid'] = (recs['qid'] + 1) % 3
    other = eng.pileup(c.G, B, r2, first, blocks, windows, items)
    B.close()
    assert other[0].tobytes() == ok_cols.tobytes() and other[1].tobytes() == ok_call.tobytes()


# ---- end to end ------------------------------------------------------------------------------------------------------------

E2E_SEED = 5
# (family, reverse-complemented) of the six slots of either scaffold, 3000 bp apart.  The engine chains like lastz --chain: of a
# scaffold pair and strand only the best collinear set of HSPs becomes alignments, so a copy has at most four rows over it — its
# scaffold's own diagonal, one from the minus strand of its own scaffold, and one per strand from the other scaffold — and which
# of them it has depends on the order and the strands of the copies along both scaffolds.  Scaffold 0 is its own mirror image
# (every copy faces a reversed copy of its family across the middle); with five forward and three reversed copies of family 0 no
# layout on two scaffolds gives every copy three rows (the three forward copies that share a scaffold have five partners between
# them and need six).  In this one the CPU oracle (oracle/oracle.py, default parameters, rows of 100 bp and 60 per cent that
# cover 80 per cent of the copy) finds 3 or 4 rows over ten of the twelve copies and 2 over the last two of scaffold 1.
E2E_LAYOUT = (((0, False), (0, False), (1, False), (1, True), (0, True), (0, True)),
              ((0, False), (0, False), (1, True), (0, True), (0, False), (1, False)))


def consensus_genome(seed=E2E_SEED, layout=E2E_LAYOUT, div=0.08):
    """Two scaffolds of 20 kbp of random sequence; a family of 600 bp planted 8 times, three of them reverse-complemented, and
    one of 400 bp planted 4 times; every copy with independent substitutions at 8 per cent and no indel, so that the positions
    of a copy and of its family correspond.  Returns (names, seqs, families as codes 0..3, [(scaffold, start, end, family,
    reversed)])."""
    rng = np.random.Generator(np.random.PCG64(seed))
    codes = [rng.integers(0, 4, size=20_000, dtype=np.uint8) for _ in range(2)]
    fams = [rng.integers(0, 4, size=600, dtype=np.uint8), rng.integers(0, 4, size=400, dtype=np.uint8)]
    planted = []
    for s, slots in enumerate(layout):
        for k, (f, rev) in enumerate(slots):
            cp = fams[f].copy()
            sub = rng.random(cp.size) < div
            cp[sub] = (cp[sub] + rng.integers(1, 4, size=int(sub.sum()), dtype=np.uint8)) % 4
            if rev:
                cp = (3 - cp)[::-1]
            p = 1500 + 3000 * k + int(rng.integers(0, 300))
            codes[s][p:p + cp.size] = cp
            planted.append((s, p, p + cp.size, f, rev))
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


def test_cli_consensus_end_to_end(eng, tmp_path):
    from mimeo_amd import run_self
    names, seqs, fams, planted = consensus_genome()
    assert sum(1 for p in planted if p[3] == 0) == 8 and sum(1 for p in planted if p[3] == 0 and p[4]) == 3 and sum(1 for p in planted if p[3] == 1) == 4
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    plain, cons = tmp_path / 'plain', tmp_path / 'cons'
    run_self.main(['--afasta', fa, '-d', str(plain), '--loglevel', 'WARNING'])
    run_self.main(['--afasta', fa, '-d', str(cons), '--loglevel', 'WARNING', '--consensus', str(cons / 'lib.fa'), '--families', str(cons / 'fam.tsv')])
    # nothing else changes
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3'):
        assert (cons / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(os.listdir(cons)) == sorted(os.listdir(plain) + ['lib.fa', 'fam.tsv'])
    # one record per family of the --families file of the same run, in the same order
    fam_rows = [l.split('\t') for l in (cons / 'fam.tsv').read_text().splitlines()[1:]]
    fam_names = list(dict.fromkeys(r[4] for r in fam_rows))
    recs = _fasta(cons / 'lib.fa')
    assert len(recs) == len(fam_names) >= 2 and [h.split()[0][1:] for h, _ in recs] == fam_names
    by_id = {r[0]: r for r in fam_rows}
    better = 0
    for head, seq in recs:
        f = dict(x.split('=') for x in head.split()[1:] if '=' in x)
        seqid, span = head.split()[2].split(':')
        start, end = (int(x) for x in span.split('-'))
        row = by_id[f['rep']]
        assert row[1:5] == [seqid, str(start), str(end), head.split()[0][1:]] and int(f['members']) == int(row[5])   # the representative is a member
        assert int(f['length']) == len(seq) and set(seq) <= set('ACGTN')
        s = names.index(seqid)
        over = [p for p in planted if p[0] == s and p[1] < end and start < p[2]]
        assert len(over) == 1, (head, over)   # a region is one planted copy
        _, p0, p1, fam, rev = over[0]
        assert len(seq) == end - start, head   # no column was called '-': column i of the consensus is target base start + i
        truth = ((3 - fams[fam])[::-1] if rev else fams[fam])
        a, b = max(start, p0), min(end, p1)    # the planted span of the representative copy inside its region
        assert b - a >= 0.9 * (p1 - p0)
        want = ACGT[truth[a - p0:b - p0]]
        own = int((seqs[s][a:b] != want).sum())
        got = int((np.frombuffer(seq[a - start:b - start].encode(), dtype=np.uint8) != want).sum())
        print(head, 'mismatches to the family: the copy', own, 'the consensus', got)
        assert float(f['mean_depth']) >= 2.0
        if int(f['members']) > 1:
            assert got < own, (head, got, own)   # strictly fewer mismatches than the representative copy itself has
            better += 1
    assert better >= 2   # both planted families
    # the budget cuts the windows into runs and changes no byte
    from mimeo_amd import workflow
    old = workflow.CONSENSUS_BUDGET
    args = run_self.mainArgs(['--afasta', fa])
    A = eng.Genome.from_fasta([fa], None)
    try:
        workflow.self_repeats(A, workflow.all_pairs(len(A.names)), str(tmp_path / 'b.tab'), str(tmp_path / 'b.gff3'), prefix=args.prefix, label=args.label,
                              consensus=str(tmp_path / 'b.fa'), consensus_budget=700)
    finally:
        A.close()
    assert workflow.CONSENSUS_BUDGET == old and (tmp_path / 'b.fa').read_bytes() == (cons / 'lib.fa').read_bytes()
    assert (tmp_path / 'b.gff3').read_bytes() == (plain / 'mimeo-self_repeats.gff3').read_bytes()
