"""Alignment text from the device (mimeo_path_text, kernel K11; engine.path_text; `--maf`, `--paf --cs`) against a plain numpy
restatement that works from the sequences and the blocks alone: letters ACGTacgt -> ACGT, anything else -> N, the reverse
complement taken on the host; between two blocks the insertion columns ('-' over the query bases) and then the deletion
columns (the target bases over '-'), then the block.  Equality is byte for byte."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi
from mimeo_amd.synth import flanked_tandem_genome, synth_genome, tandem_genome, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_runs', 'ins_bases', 'del_runs', 'del_bases')
GAP, N = ord('-'), ord('N')
LETTER = np.full(256, N, dtype=np.uint8)
COMP = np.full(256, N, dtype=np.uint8)
for _c, _d in zip(b'ACGT', b'TGCA'):
    LETTER[_c] = LETTER[_c + 32] = _c
    COMP[_c], COMP[_c + 32] = _d, _d + 32


def revcomp(a):
    return COMP[a][::-1].copy()


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def restate(seq_t, seq_q, recs, first, blocks):
    """(row_first, trow, qrow) from the sequences and the blocks alone.  seq_t / seq_q: scaffold number -> uint8 bases."""
    lt, lq, rc = {}, {}, {}
    tparts, qparts, row_first = [], [], [0]
    for i in range(recs.size):
        r = recs[i]
        tid, qid = int(r['tid']), int(r['qid'])
        if tid not in lt:
            lt[tid] = LETTER[seq_t[tid]]
        T = lt[tid]
        if int(r['qstrand']):
            if qid not in rc:
                rc[qid] = LETTER[revcomp(seq_q[qid])]
            Q = rc[qid]
        else:
            if qid not in lq:
                lq[qid] = LETTER[seq_q[qid]]
            Q = lq[qid]
        cols, pt, pq = 0, None, None
        for k in range(int(first[i]), int(first[i + 1])):
            t, q, ln = int(blocks['t'][k]), int(blocks['q'][k]), int(blocks['len'][k])
            if pt is not None:
                dq, dt = q - pq, t - pt
                assert dq >= 0 and dt >= 0
                tparts += [np.full(dq, GAP, np.uint8), T[pt:pt + dt]]       # insertions first, then deletions
                qparts += [Q[pq:pq + dq], np.full(dt, GAP, np.uint8)]
                cols += dq + dt
            assert t + ln <= T.size and q + ln <= Q.size
            tparts.append(T[t:t + ln])
            qparts.append(Q[q:q + ln])
            cols += ln
            pt, pq = t + ln, q + ln
        row_first.append(row_first[-1] + cols)
    cat = lambda p: np.concatenate(p) if p else np.zeros(0, np.uint8)
    return np.array(row_first, dtype=np.uint64), cat(tparts), cat(qparts)


def same(got, exp, tag):
    (gf, gt, gq), (ef, et, eq) = got, exp
    assert gf.dtype == np.dtype('<u8') and gt.dtype == np.uint8 and gq.dtype == np.uint8, tag
    assert gf.tolist() == ef.tolist(), tag
    for name, g, e in (('trow', gt, et), ('qrow', gq, eq)):
        assert g.size == e.size, (tag, name)
        bad = np.flatnonzero(g != e)
        if bad.size:
            i = int(np.searchsorted(ef, bad[0], side='right')) - 1
            a, z = int(ef[i]), min(int(ef[i + 1]), int(ef[i]) + 200)
            raise AssertionError((tag, name, 'record %d, column %d of %d, %d bytes differ' % (i, bad[0] - a, int(ef[i + 1]) - a, bad.size),
                                  bytes(g[a:z]), bytes(e[a:z])))


def select_rows(exp, rows):
    ef, et, eq = exp
    out = np.zeros(len(rows) + 1, dtype=np.uint64)
    out[1:] = np.cumsum([int(ef[i + 1] - ef[i]) for i in rows])
    take = np.concatenate([np.arange(int(ef[i]), int(ef[i + 1])) for i in rows]) if len(rows) else np.zeros(0, np.int64)
    return out, et[take], eq[take]


# ---- made-up paths ---------------------------------------------------------------------------------------------------------

MODS = (0, 1, 31, 32, 33, 63)
LENS = (1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
GAPS = (0, 1, 15, 16, 17, 63, 64, 65)
N_RUNS = ((5000, 5400), (12_000, 12_001), (19_990, 19_999))   # of scaffold 1; the last one ends the scaffold


def _genome():
    rng = np.random.default_rng(110)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    s = [acgt[rng.integers(0, 4, n)].copy() for n in (20_000, 19_999, 12_345)]
    for a, b in N_RUNS:
        s[1][a:b] = N
    s[1][7000:7300] += 32    # soft-masked stretches, one running into an n
    s[1][11_990:12_010] = np.where(s[1][11_990:12_010] == N, ord('n'), s[1][11_990:12_010] + 32)
    s[1][100] = ord('R')     # an IUPAC code is an N to the engine
    s[0][3000:3040] += 32
    return ['m0', 'm1', 'm2'], s


def _paths():
    """(records, first, blocks, {what: record numbers}) of the hand-built set; tid / qid index the three scaffolds"""
    _, s = _genome()
    L = [int(x.size) for x in s]
    rng = np.random.default_rng(111)
    recs, first, blocks, names = [], [0], [], {}

    def add(what, tid, qid, strand, blk):
        t_end = q_end = 0
        for t, q, ln in blk:   # the contract of mimeo_path_block, so that a slip in this table is not taken for a kernel's
            assert ln >= 1 and t >= t_end and q >= q_end and t + ln <= L[tid] and q + ln <= L[qid], (what, t, q, ln)
            t_end, q_end = t + ln, q + ln
        names.setdefault(what, []).append(len(recs))
        recs.append((tid, qid, strand))
        blocks.extend(blk)
        first.append(len(blocks))

    def chain(nb, t, q, max_len):
        blk = []
        for _ in range(nb):
            ln = int(rng.integers(1, max_len + 1))
            blk.append((t, q, ln))
            kind = int(rng.integers(0, 3))   # an insertion, a deletion, or both
            t, q = t + ln + (int(rng.integers(1, 4)) if kind != 0 else 0), q + ln + (int(rng.integers(1, 4)) if kind != 1 else 0)
        return blk

    # block starts with t mod 64 and q mod 64 each of MODS, independently; every length of LENS at every such start
    for i, tm in enumerate(MODS):
        for j, qm in enumerate(MODS):
            tid, qid = (i + j) % 3, (i + 2 * j + 1) % 3
            t, q, blk = 192 + tm, 320 + qm, []
            for ln in LENS:
                blk.append((t, q, ln))
                step = 64 * ((ln + 1 + 63) // 64)
                t, q = t + step, q + step
            add('mods', tid, qid, (i * 6 + j) & 1, blk)
    # every combination of the gaps where at least one is non-zero, between blocks that end and start anywhere in a word;
    # around the soft-masked stretch and the IUPAC letter of scaffold 1 as well
    for i, dq in enumerate(GAPS):
        for j, dt in enumerate(GAPS):
            if dq or dt:
                t0, q0 = 6900 + 7 * i + j, 40 + 5 * j + i
                add('gaps', 1, (i + j) % 3, (i + j) & 1, [(t0, q0, 40), (t0 + 40 + dt, q0 + 40 + dq, 33), (t0 + 73 + 2 * dt, q0 + 73 + 2 * dq, 1)])
    # chains of one-column blocks with one-base gaps between them: 16 columns cross ten segments and more
    for strand in (0, 1):
        for kinds in ((1,), (2,), (0,), (0, 1, 2)):   # deletions, insertions, both at once, mixed
            t, q, blk = 80 + strand, 95, []
            for k in range(150):
                blk.append((t, q, 1))
                kind = kinds[k % len(kinds)]
                t, q = t + 1 + (kind != 2), q + 1 + (kind != 1)
            add('ones', 1, 0, strand, blk)
    # a block starting at base 0 and one ending on the last base of both scaffolds, forward and reverse-complement strand
    for strand in (0, 1):
        add('ends', 0, 2, strand, [(0, 0, 100), (L[0] - 77, L[2] - 77, 77)])
        add('ends', 1, 0, strand, [(0, 0, 1), (L[1] - 1, L[0] - 1, 1)])
        add('ends', 1, 2, strand, [(L[1] - 48, L[2] - 48, 48)])   # 16-column groups that end on the scaffolds' last bases
    # 1, 64, 65 and 200 blocks
    for nb in (1, 64, 65, 200):
        for strand in (0, 1):
            add('blocks %d' % nb, 0, 1, strand, chain(nb, 3, 17, 90))
    # one block of 10 000 columns, and two blocks of 19 070 columns in all
    for strand in (0, 1):
        add('long', 0, 1, strand, [(33, 1, 10_000)])
        add('long', 1, 0, strand, [(64, 127, 9000), (9070, 9191, 10_000)])
    # blocks lying wholly in N, on either side and on both strands
    a, b = N_RUNS[0]
    add('in N', 1, 0, 0, [(a + 10, 700, 300)])
    add('in N', 0, 1, 0, [(700, a + 10, 300)])
    add('in N', 0, 1, 1, [(700, L[1] - b + 10, 300)])
    add('in N', 1, 1, 1, [(a, L[1] - b, b - a)])
    # T and Q the same scaffold: the main diagonal and off it, both strands
    for strand in (0, 1):
        add('same', 0, 0, strand, [(100, 100, 500), (1000, 3000, 500)])
        add('same', 1, 1, strand, [(4900, 4900, 700)])
    # no blocks at all
    add('empty', 2, 1, 0, [])
    # 3 000 short alignments in one call: several workgroups, rows that share their 16-byte groups with their neighbours
    for _ in range(3000):
        tid, qid = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        nb = int(rng.integers(1, 5))
        add('many', tid, qid, int(rng.integers(0, 2)), chain(nb, int(rng.integers(0, 5000)), int(rng.integers(0, 5000)), 200))
    r = np.zeros(len(recs), dtype=_ffi.ALIGNMENT)
    r['tid'], r['qid'], r['qstrand'] = [x[0] for x in recs], [x[1] for x in recs], [x[2] for x in recs]
    return r, np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK), names


@pytest.fixture(scope='module')
def made_up():
    names, s = _genome()
    recs, first, blocks, what = _paths()
    seq = dict(enumerate(s))
    return names, s, recs, first, blocks, what, restate(seq, seq, recs, first, blocks)


def test_made_up_paths_cover_what_they_claim(made_up):
    """On the restatement's side: the table holds every case it was built for."""
    _, s, recs, first, blocks, what, (ef, et, eq) = made_up
    blk = lambda w: blocks[np.concatenate([np.arange(int(first[i]), int(first[i + 1])) for i in what[w]])]
    b = blk('mods')
    assert {(int(t) % 64, int(q) % 64) for t, q in zip(b['t'], b['q'])} == {(a, c) for a in MODS for c in MODS}
    assert set(b['len'].tolist()) == set(LENS)
    gaps = set()
    for i in what['gaps']:
        g = blocks[int(first[i]):int(first[i + 1])]
        gaps.add((int(g['q'][1]) - int(g['q'][0]) - int(g['len'][0]), int(g['t'][1]) - int(g['t'][0]) - int(g['len'][0])))
    assert gaps == {(a, c) for a in GAPS for c in GAPS if a or c}
    assert sorted(int(first[i + 1] - first[i]) for k in (1, 64, 65, 200) for i in what['blocks %d' % k]) == [1, 1, 64, 64, 65, 65, 200, 200]
    cols = (ef[1:] - ef[:-1]).astype(np.int64)
    assert sorted(cols[what['long']].tolist()) == [10_000, 10_000, 19_070, 19_070] and cols[what['empty'][0]] == 0
    # a lane's 16 columns cross ten segments and more: in the chains of ones every 16 columns hold at least 5 gap runs on a side
    for i in what['ones']:
        row_t, row_q = et[int(ef[i]):int(ef[i + 1])], eq[int(ef[i]):int(ef[i + 1])]
        gap = (row_t == GAP) | (row_q == GAP)
        seg = 1 + np.count_nonzero(np.diff(gap[:16].astype(np.int8)) != 0)
        assert seg >= 10, (i, seg)
    for i in what['in N'][:3]:
        row_t, row_q = et[int(ef[i]):int(ef[i + 1])], eq[int(ef[i]):int(ef[i + 1])]
        assert ((row_t == N) | (row_q == N)).all() and not ((row_t == N) & (row_q == N)).any()
    i = what['in N'][3]
    assert (et[int(ef[i]):int(ef[i + 1])] == N).all() and (eq[int(ef[i]):int(ef[i + 1])] == N).all()
    i = what['same'][0]
    assert (et[int(ef[i]):int(ef[i]) + 500] == eq[int(ef[i]):int(ef[i]) + 500]).all()
    assert set(recs['qstrand'].tolist()) == {0, 1} and recs.size > 3000
    assert set(np.unique(et).tolist()) == set(b'ACGTN-') == set(np.unique(eq).tolist())   # nothing in lower case, no R
    # every alignment of the output against a 16-byte group: all row starts and all row lengths mod 16, and more than 1 000 row
    # boundaries inside a group
    assert set((ef[:-1] % 16).tolist()) == set(range(16)) and set((cols % 16).tolist()) == set(range(16))
    inner = ef[1:-1]
    assert np.count_nonzero((inner % 16 != 0) & (cols[:-1] > 0) & (cols[1:] > 0)) > 1000


def test_made_up_paths_equal_the_restatement(eng, made_up, monkeypatch):
    names, s, recs, first, blocks, what, exp = made_up
    A = eng.Genome(names, s)
    got = eng.path_text(A, None, recs, first, blocks)
    same(got, exp, 'made-up')
    same(eng.path_text(A, A, recs, first, blocks), exp, 'B given as A itself')
    # the same list in reversed alignment order: every row at another place of the output
    from mimeo_amd import formats
    rev = np.arange(recs.size)[::-1]
    f2, b2 = formats.select_paths(first, blocks, rev)
    same(eng.path_text(A, None, recs[rev], f2, b2), select_rows(exp, rev.tolist()), 'reversed')
    # every alignment a slice of its own, small slices; rows cut into jobs of 16 and of 48 columns, never cut; both at once; one
    # job per launch (a workgroup with three idle wavefronts) and three (a partial last workgroup); the jobs of a cut row in
    # different launches; a launch cap that is no number or zero is the default
    for env in ({'MIMEO_PATH_TEXT_SLICE_COLUMNS': '1'}, {'MIMEO_PATH_TEXT_SLICE_COLUMNS': '100'}, {'MIMEO_PATH_TEXT_SLICE_COLUMNS': '4096'},
                {'MIMEO_PATH_TEXT_SPLIT_COLUMNS': '16'}, {'MIMEO_PATH_TEXT_SPLIT_COLUMNS': '48'}, {'MIMEO_PATH_TEXT_SPLIT_COLUMNS': '0'},
                {'MIMEO_PATH_TEXT_SLICE_COLUMNS': '700', 'MIMEO_PATH_TEXT_SPLIT_COLUMNS': '32'},
                {'MIMEO_PATH_LAUNCH_JOBS': '1'}, {'MIMEO_PATH_LAUNCH_JOBS': '3'}, {'MIMEO_PATH_TEXT_SPLIT_COLUMNS': '16', 'MIMEO_PATH_LAUNCH_JOBS': '3'},
                {'MIMEO_PATH_LAUNCH_JOBS': '0'}, {'MIMEO_PATH_LAUNCH_JOBS': 'abc'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        same(eng.path_text(A, None, recs, first, blocks), exp, env)
        for k in env:
            monkeypatch.delenv(k)
    # n == 0
    rf, tr, qr = eng.path_text(A, None, recs[:0], first[:1], blocks[:0])
    assert rf.dtype == np.dtype('<u8') and rf.tolist() == [0] and tr.size == 0 and qr.size == 0 and tr.dtype == np.uint8
    # alignments without blocks alone: rows of no columns
    e = what['empty'][0]
    rf, tr, qr = eng.path_text(A, None, recs[[e, e]], np.zeros(3, np.uint64), blocks[:0])
    assert rf.tolist() == [0, 0, 0] and tr.size == 0 and qr.size == 0
    # Q another genome than T: the query scaffolds in another order
    B = eng.Genome(['m2', 'm0', 'm1'], [s[2], s[0], s[1]])
    r2 = recs.copy()
    r2['qid'] = (recs['qid'] + 1) % 3
    same(eng.path_text(A, B, r2, first, blocks), exp, 'two genomes')
    A.close()
    B.close()


def test_validation_reaches_the_caller(eng, made_up):
    """the five bad inputs of tests/test_gpu_divergence.py::test_validation_reaches_the_caller, under this entry point's name"""
    names, s, recs, first, blocks, what, exp = made_up
    A = eng.Genome(names, s)
    n = 40
    f, b = first[:n + 1].copy(), blocks[:int(first[n])].copy()
    bad = b.copy()
    bad['len'][int(f[7]) + 2] = 0
    with pytest.raises(RuntimeError, match=r'mimeo_path_text: record 7, block %d .*len is 0' % (int(f[7]) + 2)):
        eng.path_text(A, None, recs[:n], f, bad)
    bad = b.copy()
    k = int(f[12])
    bad['t'][k], bad['len'][k] = 0xFFFFFFF0, 0x20
    with pytest.raises(RuntimeError, match=r'mimeo_path_text: record 12, block %d .*beyond the target scaffold' % k):
        eng.path_text(A, None, recs[:n], f, bad)
    r = recs[:n].copy()
    r['qstrand'][5] = 2
    with pytest.raises(RuntimeError, match=r'mimeo_path_text: record 5: qstrand'):
        eng.path_text(A, None, r, f, b)
    r = recs[:n].copy()
    r['tid'][9] = 3
    with pytest.raises(RuntimeError, match=r'mimeo_path_text: record 9: tid'):
        eng.path_text(A, None, r, f, b)
    f2 = f.copy()
    f2[3] = f2[2] - 1
    with pytest.raises(RuntimeError, match=r'mimeo_path_text: record 2: path_first decreases'):
        eng.path_text(A, None, recs[:n], f2, b)
    with pytest.raises(ValueError):
        eng.path_text(A, None, recs[:n], f[:-1], b)
    # nothing was launched and nothing is broken: a valid call still answers
    same(eng.path_text(A, None, recs[:n], f, b), select_rows(exp, list(range(n))), 'after the refusals')
    A.close()


# ---- the engine's own paths ------------------------------------------------------------------------------------------------

def _inputs():
    """the four inputs of tests/test_gpu_paths.py::_inputs"""
    _, s = tandem_genome(3, 2, 60_000)
    _, f = flanked_tandem_genome(1, 2)
    _, y = synth_genome(50, 200_000, 2, repeat_frac=0.2, families=5)
    return [('tandem (0, 1)', s[0], s[1]), ('tandem (0, 0)', s[0], s[0]), ('flanked, query reverse-complemented', f[0], revcomp(f[1])),
            ('synth (0, 1)', y[0], y[1])]


def stats_of_rows(row_first, trow, qrow):
    """the eight fields of mimeo_column_stats counted from the rows"""
    out = np.zeros(row_first.size - 1, dtype=_ffi.COLUMN_STATS)
    purine = np.zeros(256, bool)
    purine[list(b'AG')] = True
    for i in range(out.size):
        t, q = trow[int(row_first[i]):int(row_first[i + 1])], qrow[int(row_first[i]):int(row_first[i + 1])]
        ins, dele = t == GAP, q == GAP
        col = ~ins & ~dele
        amb = col & ((t == N) | (q == N))
        ok = col & ~amb
        runs = lambda m: int(np.count_nonzero(m & ~np.concatenate([[False], m[:-1]])))
        out[i] = (np.count_nonzero(ok & (t == q)), np.count_nonzero(ok & (t != q) & (purine[t] == purine[q])),
                  np.count_nonzero(ok & (purine[t] != purine[q])), np.count_nonzero(amb), runs(ins), np.count_nonzero(ins), runs(dele), np.count_nonzero(dele))
    return out


@pytest.mark.parametrize('rule', [0, 1], ids=['box', 'path'])
def test_engine_paths(eng, rule):
    minus = gapped = 0
    for tag, T, Q in _inputs():
        g = eng.Genome(['t', 'q'], [T, Q])
        recs, first, blocks = eng.align_pairs(g, None, [(0, 1)], eng.default_params(anchor_rule=rule), paths=True)
        assert not eng.failed_pairs()
        got = eng.path_text(g, None, recs, first, blocks)
        k9 = eng.path_stats(g, None, recs, first, blocks)
        g.close()
        exp = restate({0: T}, {1: Q}, recs, first, blocks)
        # the case is not vacuous: asserted on the restatement's side
        ef, et, eq = exp
        assert recs.size >= 1 and int(ef[-1]) > 10_000, tag
        minus += int(np.count_nonzero(recs['qstrand']))
        gapped += int(np.count_nonzero([(et[int(ef[i]):int(ef[i + 1])] == GAP).any() or (eq[int(ef[i]):int(ef[i + 1])] == GAP).any() for i in range(recs.size)]))
        same(got, exp, (tag, rule))
        rf, tr, qr = got
        i64 = lambda f: recs[f].astype(np.int64)
        nongap_t = np.array([np.count_nonzero(tr[int(rf[i]):int(rf[i + 1])] != GAP) for i in range(recs.size)])
        nongap_q = np.array([np.count_nonzero(qr[int(rf[i]):int(rf[i + 1])] != GAP) for i in range(recs.size)])
        assert (nongap_t == i64('tend') - i64('tstart')).all() and (nongap_q == i64('qend') - i64('qstart')).all(), tag
        mine = stats_of_rows(rf, tr, qr)
        for f in FIELDS:
            assert (mine[f] == k9[f]).all(), (tag, rule, f, mine[f][:5], k9[f][:5])
        assert (mine['matches'] == recs['id_n']).all(), tag
    assert minus >= 2 and gapped >= 5, (minus, gapped)


# ---- CLI end to end --------------------------------------------------------------------------------------------------------

def _cigar_blocks(t, q, cigar):
    out = []
    for n, op in re.findall(r'(\d+)([MID])', cigar):
        n = int(n)
        if op == 'M':
            out.append((t, q, n))
            t, q = t + n, q + n
        elif op == 'I':
            q += n
        else:
            t += n
    return out


def _run(tmp_path, tag, cmd, extra):
    d = tmp_path / tag
    r = subprocess.run([sys.executable, '-m', 'mimeo_amd'] + cmd + ['-d', str(d)] + [str(d / x) if x.startswith('a.') else x for x in extra],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return d


def _three_runs(tmp_path, tag, cmd, same_files):
    """plain (with --paf), --maf, --paf --cs: the TAB, the GFF3 and the listing are the same apart from the new files"""
    d_plain = _run(tmp_path, tag + '_plain', cmd, ['--paf', 'a.paf'])
    d_maf = _run(tmp_path, tag + '_maf', cmd, ['--maf', 'a.maf'])
    d_cs = _run(tmp_path, tag + '_cs', cmd, ['--paf', 'a.paf', '--cs'])
    for d in (d_maf, d_cs):
        for f in same_files:
            assert (d / f).read_bytes() == (d_plain / f).read_bytes(), (tag, f)
    new = {'a.paf', 'a.maf'}
    assert sorted(set(os.listdir(d_plain)) - new) == sorted(set(os.listdir(d_maf)) - new) == sorted(set(os.listdir(d_cs)) - new)
    assert 'a.maf' in os.listdir(d_maf) and 'a.paf' not in os.listdir(d_maf) and 'a.maf' not in os.listdir(d_cs)
    return d_plain, d_maf, d_cs


def _parse_maf(path):
    text = path.read_text()
    assert text.startswith('##maf version=1 scoring=mimeo-amd\n')
    out = []
    for block in text.split('\n', 1)[1].split('\n\n'):
        if not block.strip():
            continue
        lines = block.split('\n')
        assert len(lines) == 3 and lines[0].startswith('a score=') and all(l.startswith('s ') for l in lines[1:]), block[:200]
        out.append((int(lines[0][8:]), lines[1].split(' '), lines[2].split(' ')))
    assert text.endswith('\n\n')
    return out


def _check_maf(maf, tab, tnames, tseqs, qnames, qseqs):
    """one block per TAB row in TAB order, with the TAB's scores; every s line as specified; the ungapped rows are the slices"""
    rows = [l.split('\t') for l in tab.read_text().splitlines() if not l.startswith('#')]
    blocks = _parse_maf(maf)
    assert len(blocks) == len(rows) > 3
    tidx, qidx = {n: i for i, n in enumerate(tnames)}, {n: i for i, n in enumerate(qnames)}
    strands = set()
    for (score, st, sq), r in zip(blocks, rows):
        # TAB: name1 strand1 start1 (origin one) end1 name2 strand2 start2+ end2+ score identity
        assert score == int(r[8]) and len(st) == 7 and len(sq) == 7
        T, Q = tseqs[tidx[r[0]]], qseqs[qidx[r[4]]]
        ts, te, qs, qe = int(r[2]) - 1, int(r[3]), int(r[6]) - 1, int(r[7])
        assert st[1:6] == [r[0], str(ts), str(te - ts), '+', str(T.size)]
        minus = r[5] == '-'
        assert sq[1:6] == [r[4], str(Q.size - qe if minus else qs), str(qe - qs), '-' if minus else '+', str(Q.size)]
        strands.add(r[5])
        assert len(st[6]) == len(sq[6])
        assert st[6].replace('-', '') == bytes(LETTER[T[ts:te]]).decode()
        assert sq[6].replace('-', '') == bytes(LETTER[(revcomp(Q) if minus else Q)[(Q.size - qe if minus else qs):(Q.size - qs if minus else qe)]]).decode()
    return strands


def _check_cs(paf_cs, paf_plain, tnames, tseqs, qnames, qseqs):
    rows, plain = paf_cs.read_text().splitlines(), paf_plain.read_text().splitlines()
    assert len(rows) == len(plain) > 3
    assert [re.sub(r'\tcs:Z:[^\t]*', '', l) for l in rows] == plain
    tidx, qidx = {n: i for i, n in enumerate(tnames)}, {n: i for i, n in enumerate(qnames)}
    subs = gaps = 0
    for l, pl in zip(rows, plain):
        assert l.startswith(pl + '\tcs:Z:')
        p = l.split('\t')
        assert p[-2].startswith('cg:Z:') and p[-1].startswith('cs:Z:')
        minus = p[4] == '-'
        T, Q = LETTER[tseqs[tidx[p[5]]]], qseqs[qidx[p[0]]]
        Q = LETTER[revcomp(Q)] if minus else LETTER[Q]
        t, q = int(p[7]), (int(p[1]) - int(p[3]) if minus else int(p[2]))
        ops, matches = [], 0
        for op, arg in re.findall(r'([:*+-])([0-9a-z]+)', p[-1][5:]):
            if op == ':':
                n = int(arg)
                assert (T[t:t + n] == Q[q:q + n]).all() and (T[t:t + n] != N).all()
                matches += n
                ops.append(['M', n])
                t, q = t + n, q + n
            elif op == '*':
                assert len(arg) == 2 and arg == (chr(T[t]) + chr(Q[q])).lower() and (arg[0] != arg[1] or arg == 'nn')
                subs += 1
                ops.append(['M', 1])
                t, q = t + 1, q + 1
            elif op == '+':
                assert arg == bytes(Q[q:q + len(arg)]).decode().lower()
                gaps += 1
                ops.append(['I', len(arg)])
                q += len(arg)
            else:
                assert arg == bytes(T[t:t + len(arg)]).decode().lower()
                gaps += 1
                ops.append(['D', len(arg)])
                t += len(arg)
        assert ''.join(op + arg for op, arg in re.findall(r'([:*+-])([0-9a-z]+)', p[-1][5:])) == p[-1][5:]   # nothing else in the tag
        merged = []
        for op, n in ops:
            if merged and merged[-1][0] == op:
                merged[-1][1] += n
            else:
                merged.append([op, n])
        assert ''.join('%d%s' % (n, op) for op, n in merged) == p[-2][5:], l[:300]
        assert matches == int(p[9]) and t == int(p[8])
    assert subs > 10 and gaps >= 1


def test_cli_self_maf_and_cs(tmp_path, eng):
    names, seqs = tandem_genome(3, 2, 60_000)
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    d_plain, d_maf, d_cs = _three_runs(tmp_path, 'self', ['self', '--afasta', fa], ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3'))
    _check_maf(d_maf / 'a.maf', d_maf / 'mimeo_alignment.tab', names, seqs, names, seqs)
    _check_cs(d_cs / 'a.paf', d_plain / 'a.paf', names, seqs, names, seqs)
    # the writer with a column budget of 1 000 (every row of 60 kb goes alone, the short ones in runs) writes the same bytes
    from mimeo_amd import workflow
    A = eng.Genome.from_fasta([fa])
    pairs = workflow.all_pairs(len(A.names))
    for tag, kw in (('small', {'text_budget': 1000}), ('default', {})):
        d = tmp_path / ('writer_' + tag)
        os.makedirs(d)
        workflow.self_repeats(A, pairs, str(d / 't.tab'), str(d / 't.gff3'), maf=str(d / 'a.maf'), prefix='Self_Repeat', **kw)
        assert (d / 'a.maf').read_bytes() == (d_maf / 'a.maf').read_bytes(), tag
        assert (d / 't.tab').read_bytes() == (d_maf / 'mimeo_alignment.tab').read_bytes()
    A.close()


def test_cli_map_maf_and_cs(tmp_path):
    names, seqs = tandem_genome(3, 2, 60_000)
    fa, fb = str(tmp_path / 'a.fa'), str(tmp_path / 'b.fa')
    write_fasta(fa, names, seqs)
    bnames, bseqs = ['b0', 'b1'], [revcomp(seqs[1]), seqs[0][5000:45_000].copy()]
    write_fasta(fb, bnames, bseqs)
    d_plain, d_maf, d_cs = _three_runs(tmp_path, 'map', ['map', '--afasta', fa, '--bfasta', fb, '--minIdt', '60'], ('mimeo_alignment.tab',))
    assert _check_maf(d_maf / 'a.maf', d_maf / 'mimeo_alignment.tab', names, seqs, bnames, bseqs) == {'+', '-'}
    _check_cs(d_cs / 'a.paf', d_plain / 'a.paf', names, seqs, bnames, bseqs)
