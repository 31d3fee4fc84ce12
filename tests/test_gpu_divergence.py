"""Column statistics of alignment paths (mimeo_path_stats, kernel K9; engine.path_stats; `--paf --divergence`) against a plain
numpy restatement: per column of every block, x = target base, y = query base (reverse-complemented query for a minus row),
ambiguous where either is not ACGT, else match / transition (x ^ y == 2) / transversion; gaps from the jumps between blocks.
Equality is exact, field by field."""
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


def restate(seq_t, seq_q, recs, first, blocks):
    """The statistics of every record, from the sequences and the blocks alone.  seq_t / seq_q: scaffold number -> uint8 bases."""
    out = np.zeros(recs.size, dtype=_ffi.COLUMN_STATS)
    rc = {}
    for i in range(recs.size):
        r = recs[i]
        b = blocks[int(first[i]):int(first[i + 1])]
        T, qid = seq_t[int(r['tid'])], int(r['qid'])
        if int(r['qstrand']):
            if qid not in rc:
                rc[qid] = revcomp(seq_q[qid])
            Q = rc[qid]
        else:
            Q = seq_q[qid]
        t, q, ln = b['t'].astype(np.int64), b['q'].astype(np.int64), b['len'].astype(np.int64)
        c = np.zeros(4, dtype=np.int64)
        for k in range(b.size):
            x, y = CODE[T[int(t[k]):int(t[k] + ln[k])]], CODE[Q[int(q[k]):int(q[k] + ln[k])]]
            assert x.size == y.size == int(ln[k])
            amb = (x == 4) | (y == 4)
            c += [np.count_nonzero(~amb & (x == y)), np.count_nonzero(~amb & ((x ^ y) == 2)),
                  np.count_nonzero(~amb & (x != y) & ((x ^ y) != 2)), np.count_nonzero(amb)]
        dt, dq = t[1:] - (t[:-1] + ln[:-1]), q[1:] - (q[:-1] + ln[:-1])
        out[i] = (c[0], c[1], c[2], c[3], np.count_nonzero(dq > 0), dq[dq > 0].sum(), np.count_nonzero(dt > 0), dt[dt > 0].sum())
    return out


def same(got, exp, tag):
    assert got.dtype == _ffi.COLUMN_STATS and got.shape == exp.shape, tag
    for f in FIELDS:
        bad = np.flatnonzero(got[f] != exp[f])
        assert bad.size == 0, (tag, f, bad[:5], got[bad[:5]], exp[bad[:5]])


# ---- made-up paths ---------------------------------------------------------------------------------------------------------

MODS = (0, 1, 31, 32, 33, 63)
LENS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129)
N_RUNS = ((5000, 5400), (12_000, 12_001), (19_990, 19_999))   # of scaffold 1; the last one ends the scaffold


def _genome():
    rng = np.random.default_rng(20)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    s = [acgt[rng.integers(0, 4, n)].copy() for n in (20_000, 19_999, 12_345)]
    for a, b in N_RUNS:
        s[1][a:b] = ord('N')
    s[1][7000:7300] += 32    # soft-masked stretches, one running into an N
    s[1][11_990:12_010] = np.where(s[1][11_990:12_010] == ord('N'), ord('n'), s[1][11_990:12_010] + 32)
    s[1][100] = ord('R')     # an IUPAC code is an N to the engine
    return ['m0', 'm1', 'm2'], s


def _paths():
    """(records, first, blocks, {what: record numbers}) of the hand-built set; tid / qid index the three scaffolds"""
    _, s = _genome()
    L = [int(x.size) for x in s]
    rng = np.random.default_rng(21)
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

    def chain(nb, t, q, max_len, tid, qid):
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
    # a block starting at base 0 and one ending on the last base of both scaffolds, forward and reverse-complement strand
    for strand in (0, 1):
        add('ends', 0, 2, strand, [(0, 0, 100), (L[0] - 77, L[2] - 77, 77)])
        add('ends', 1, 0, strand, [(0, 0, 1), (L[1] - 1, L[0] - 1, 1)])
    # 1, 64, 65 and 200 blocks: a full pass of the lanes, more blocks than lanes, a partial last pass
    for nb in (1, 64, 65, 200):
        for strand in (0, 1):
            add('blocks %d' % nb, 0, 1, strand, chain(nb, 3, 17, 90, 0, 1))
    # one block of 10 000 columns: many chunks per lane (and, with the split forced, many jobs per alignment)
    for strand in (0, 1):
        add('long', 0, 1, strand, [(33, 1, 10_000)])
        add('long', 1, 0, strand, [(64, 127, 9000), (9070, 9127, 10_000)])
    # blocks lying wholly in N, on either side and on both strands
    a, b = N_RUNS[0]
    add('in N', 1, 0, 0, [(a + 10, 700, 300)])
    add('in N', 0, 1, 0, [(700, a + 10, 300)])
    add('in N', 0, 1, 1, [(700, L[1] - b + 10, 300)])
    add('in N', 1, 1, 1, [(a, L[1] - b, b - a)])
    # T and Q the same scaffold: the main diagonal (every column a match) and off it, both strands
    for strand in (0, 1):
        add('same', 0, 0, strand, [(100, 100, 500), (1000, 3000, 500)])
        add('same', 1, 1, strand, [(4900, 4900, 700)])
    # no blocks at all
    add('empty', 2, 1, 0, [])
    # 3 000 alignments in one call: several workgroups
    for _ in range(3000):
        tid, qid = int(rng.integers(0, 3)), int(rng.integers(0, 3))
        nb = int(rng.integers(1, 5))
        add('many', tid, qid, int(rng.integers(0, 2)), chain(nb, int(rng.integers(0, 5000)), int(rng.integers(0, 5000)), 200, tid, qid))
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
    _, s, recs, first, blocks, what, exp = made_up
    b = blocks[np.concatenate([np.arange(int(first[i]), int(first[i + 1])) for i in what['mods']])]
    assert {(int(t) % 64, int(q) % 64) for t, q in zip(b['t'], b['q'])} == {(a, c) for a in MODS for c in MODS}
    assert set(b['len'].tolist()) == set(LENS)
    assert sorted(int(first[i + 1] - first[i]) for k in (1, 64, 65, 200) for i in what['blocks %d' % k]) == [1, 1, 64, 64, 65, 65, 200, 200]
    assert all(exp['ambiguous'][i] == 300 and exp['matches'][i] == 0 for i in what['in N'][:3]) and exp['ambiguous'][what['in N'][3]] == 400
    assert exp['matches'][what['same'][0]] > 500 and exp['transversions'][what['same'][0]] > 100
    assert exp['matches'][what['same'][1]] + exp['ambiguous'][what['same'][1]] == 700 and exp['ambiguous'][what['same'][1]] == 400
    assert set(recs['qstrand'].tolist()) == {0, 1} and recs.size > 3000
    assert exp['ambiguous'].sum() > 1000 and exp['transitions'].sum() > 10_000 and exp['transversions'].sum() > 20_000
    assert exp['ins_runs'].sum() > 1000 and exp['del_runs'].sum() > 1000 and (exp['ins_runs'] != exp['del_runs']).any()


def test_made_up_paths_equal_the_restatement(eng, made_up, monkeypatch):
    names, s, recs, first, blocks, what, exp = made_up
    A = eng.Genome(names, s)
    got = eng.path_stats(A, None, recs, first, blocks)
    same(got, exp, 'made-up')
    assert eng.path_stats(A, A, recs, first, blocks).tobytes() == got.tobytes()   # B given as A itself
    # the same list in reversed alignment order
    from mimeo_amd import formats
    rev = np.arange(recs.size)[::-1]
    f2, b2 = formats.select_paths(first, blocks, rev)
    same(eng.path_stats(A, None, recs[rev], f2, b2), exp[rev], 'reversed')
    # every alignment a slice of its own; alignments cut into jobs of one and of three chunks; never cut; one job per launch (a
    # workgroup with three idle wavefronts) and three (a partial last workgroup); the jobs of a cut alignment in different
    # launches; a launch cap that is no number or zero is the default
    for env in ({'MIMEO_PATH_STATS_SLICE_BLOCKS': '1'}, {'MIMEO_PATH_STATS_SPLIT_CHUNKS': '1'}, {'MIMEO_PATH_STATS_SPLIT_CHUNKS': '3'},
                {'MIMEO_PATH_STATS_SPLIT_CHUNKS': '0'}, {'MIMEO_PATH_STATS_SLICE_BLOCKS': '70', 'MIMEO_PATH_STATS_SPLIT_CHUNKS': '2'},
                {'MIMEO_PATH_LAUNCH_JOBS': '1'}, {'MIMEO_PATH_LAUNCH_JOBS': '3'}, {'MIMEO_PATH_STATS_SPLIT_CHUNKS': '1', 'MIMEO_PATH_LAUNCH_JOBS': '3'},
                {'MIMEO_PATH_LAUNCH_JOBS': '0'}, {'MIMEO_PATH_LAUNCH_JOBS': 'abc'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        same(eng.path_stats(A, None, recs, first, blocks), exp, env)   # the whole list, also with one launch per alignment
        for k in env:
            monkeypatch.delenv(k)
    # n == 0
    none = eng.path_stats(A, None, recs[:0], first[:1], blocks[:0])
    assert none.dtype == _ffi.COLUMN_STATS and none.size == 0
    # Q another genome than T: the query scaffolds in another order
    B = eng.Genome(['m2', 'm0', 'm1'], [s[2], s[0], s[1]])
    r2 = recs.copy()
    r2['qid'] = (recs['qid'] + 1) % 3
    same(eng.path_stats(A, B, r2, first, blocks), exp, 'two genomes')
    A.close()
    B.close()


def test_validation_reaches_the_caller(eng, made_up):
    names, s, recs, first, blocks, what, exp = made_up
    A = eng.Genome(names, s)
    n = 40
    f, b = first[:n + 1].copy(), blocks[:int(first[n])].copy()
    bad = b.copy()
    bad['len'][int(f[7]) + 2] = 0
    with pytest.raises(RuntimeError, match=r'record 7, block %d .*len is 0' % (int(f[7]) + 2)):
        eng.path_stats(A, None, recs[:n], f, bad)
    bad = b.copy()
    k = int(f[12])
    bad['t'][k], bad['len'][k] = 0xFFFFFFF0, 0x20
    with pytest.raises(RuntimeError, match=r'record 12, block %d .*beyond the target scaffold' % k):
        eng.path_stats(A, None, recs[:n], f, bad)
    r = recs[:n].copy()
    r['qstrand'][5] = 2
    with pytest.raises(RuntimeError, match=r'record 5: qstrand'):
        eng.path_stats(A, None, r, f, b)
    r = recs[:n].copy()
    r['tid'][9] = 3
    with pytest.raises(RuntimeError, match=r'record 9: tid'):
        eng.path_stats(A, None, r, f, b)
    f2 = f.copy()
    f2[3] = f2[2] - 1
    with pytest.raises(RuntimeError, match=r'record 2: path_first decreases'):
        eng.path_stats(A, None, recs[:n], f2, b)
    # nothing was launched and nothing is broken: a valid call still answers
    same(eng.path_stats(A, None, recs[:n], f, b), exp[:n], 'after the refusals')
    A.close()


# ---- the engine's own paths ------------------------------------------------------------------------------------------------

def _inputs():
    """the four inputs of tests/test_gpu_paths.py::_inputs"""
    _, s = tandem_genome(3, 2, 60_000)
    _, f = flanked_tandem_genome(1, 2)
    _, y = synth_genome(50, 200_000, 2, repeat_frac=0.2, families=5)
    return [('tandem (0, 1)', s[0], s[1]), ('tandem (0, 0)', s[0], s[0]), ('flanked, query reverse-complemented', f[0], revcomp(f[1])),
            ('synth (0, 1)', y[0], y[1])]


# (input, rule) -> kept alignments, matches, transitions, transversions, gap runs, minus-strand rows: counted on the CPU from
# the path oracle (tests/paths_oracle.c) before the kernel existed
TOTALS = {(0, 0): (5, 23765, 917, 1704, 38, 0), (0, 1): (10, 43848, 1583, 2854, 107, 0),
          (1, 0): (1, 60000, 0, 0, 0, 0), (1, 1): (1, 60000, 0, 0, 0, 0),
          (2, 0): (2, 49961, 973, 1831, 38, 2), (2, 1): (6, 91550, 2211, 3991, 92, 6),
          (3, 0): (7, 16571, 839, 1593, 167, 4), (3, 1): (7, 16571, 839, 1593, 167, 4)}


@pytest.mark.parametrize('rule', [0, 1], ids=['box', 'path'])
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_engine_paths(eng, k, rule):
    tag, T, Q = _inputs()[k]
    g = eng.Genome(['t', 'q'], [T, Q])
    recs, first, blocks = eng.align_pairs(g, None, [(0, 1)], eng.default_params(anchor_rule=rule), paths=True)
    assert not eng.failed_pairs()
    got = eng.path_stats(g, None, recs, first, blocks)
    g.close()
    exp = restate({0: T}, {1: Q}, recs, first, blocks)
    # the case is not vacuous: asserted on the restatement's side
    tot = (recs.size, int(exp['matches'].sum()), int(exp['transitions'].sum()), int(exp['transversions'].sum()),
           int(exp['ins_runs'].sum() + exp['del_runs'].sum()), int(np.count_nonzero(recs['qstrand'])))
    print(tag, rule, tot)
    assert tot == TOTALS[(k, rule)], (tag, rule, tot)
    assert int(exp['ambiguous'].sum()) == 0
    same(got, exp, (tag, rule))
    i64 = lambda f: recs[f].astype(np.int64)
    assert (got['matches'] == recs['id_n']).all(), tag
    assert (got['matches'].astype(np.int64) + got['transitions'] + got['transversions'] + got['ambiguous'] == i64('id_d')).all(), tag
    assert (got['del_bases'] == i64('tend') - i64('tstart') - i64('id_d')).all(), tag
    assert (got['ins_bases'] == i64('qend') - i64('qstart') - i64('id_d')).all(), tag


# ---- CLI end to end --------------------------------------------------------------------------------------------------------

TAGS = re.compile(r'\t(?:NM:i|de:f|ts:i|tv:i|kd:f):[^\t]*')


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


def _run(tmp_path, tag, cmd):
    d = tmp_path / tag
    r = subprocess.run([sys.executable, '-m', 'mimeo_amd'] + cmd + ['-d', str(d), '--paf', str(d / 'a.paf')] + (['--divergence'] if tag.endswith('div') else []),
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return d


def _check_paf(paf_div, paf_plain, tnames, tseqs, qnames, qseqs):
    """rows with the five tags removed are the plain rows; NM / ts / tv of every row equal the restatement of its cg:Z:"""
    rows, plain = paf_div.read_text().splitlines(), paf_plain.read_text().splitlines()
    assert len(rows) == len(plain) > 3
    assert [TAGS.sub('', l) for l in rows] == plain
    tidx, qidx = {n: i for i, n in enumerate(tnames)}, {n: i for i, n in enumerate(qnames)}
    recs = np.zeros(len(rows), dtype=_ffi.ALIGNMENT)
    blocks, first = [], [0]
    for i, l in enumerate(rows):
        p = l.split('\t')
        assert len(p) == 19 and [x[:5] for x in p[12:]] == ['AS:i:', 'NM:i:', 'de:f:', 'ts:i:', 'tv:i:', 'kd:f:', 'cg:Z:'], l
        minus = p[4] == '-'
        recs[i]['tid'], recs[i]['qid'], recs[i]['qstrand'] = tidx[p[5]], qidx[p[0]], int(minus)
        blocks += _cigar_blocks(int(p[7]), int(p[1]) - int(p[3]) if minus else int(p[2]), p[18][5:])
        first.append(len(blocks))
    exp = restate(dict(enumerate(tseqs)), dict(enumerate(qseqs)), recs, np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK))
    from mimeo_amd import formats
    gapped = 0
    for i, l in enumerate(rows):
        p = l.split('\t')
        e = exp[i]
        assert int(p[9]) == int(e['matches']), l   # PAF's residue matches is id_n
        assert p[13:18] == formats.divergence_tags(e).split('\t'), (l, e)
        assert int(p[13][5:]) == int(e['transitions']) + int(e['transversions']) + int(e['ambiguous']) + int(e['ins_bases']) + int(e['del_bases'])
        assert (int(p[15][5:]), int(p[16][5:])) == (int(e['transitions']), int(e['transversions']))
        gapped += int(e['ins_runs']) + int(e['del_runs']) > 0
    assert gapped >= 1 and int(exp['transitions'].sum()) > 0 and int(exp['transversions'].sum()) > 0


def test_cli_self_and_map_divergence(tmp_path):
    names, seqs = tandem_genome(3, 2, 60_000)
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    cmd = ['self', '--afasta', fa]
    d_div, d_plain = _run(tmp_path, 'self_div', cmd), _run(tmp_path, 'self_plain', cmd)
    for f in ('mimeo_alignment.tab', 'mimeo-self_repeats.gff3'):
        assert (d_div / f).read_bytes() == (d_plain / f).read_bytes(), f
    assert sorted(os.listdir(d_div)) == sorted(os.listdir(d_plain))
    _check_paf(d_div / 'a.paf', d_plain / 'a.paf', names, seqs, names, seqs)
    # mimeo map on two genomes: Q != T
    bnames, bseqs = ['b0', 'b1'], [revcomp(seqs[1]), seqs[0][5000:45_000].copy()]
    fb = str(tmp_path / 'b.fa')
    write_fasta(fb, bnames, bseqs)
    cmd = ['map', '--afasta', fa, '--bfasta', fb, '--minIdt', '60']
    m_div, m_plain = _run(tmp_path, 'map_div', cmd), _run(tmp_path, 'map_plain', cmd)
    assert (m_div / 'mimeo_alignment.tab').read_bytes() == (m_plain / 'mimeo_alignment.tab').read_bytes()
    _check_paf(m_div / 'a.paf', m_plain / 'a.paf', names, seqs, bnames, bseqs)
    rows = (m_div / 'a.paf').read_text().splitlines()
    assert {l.split('\t')[4] for l in rows} == {'+', '-'}
