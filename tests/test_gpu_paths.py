"""Alignment paths out of the engine (mimeo_align_units_paths, engine.align_units(..., paths=True), `--paf`) against the
path oracle tests/paths_oracle.c: an engine path is turned into the oracle's key set, t << 32 | q per diagonal step, matched
to the oracle's extended alignment with the same (minus, score, first key), and the key arrays must be equal.  Every returned
alignment is also rescored from the two sequences and its blocks alone (HOXD70, 400 + 30 g per gap) and held to the
invariants include/mimeo_hip.h promises."""
import multiprocessing as mp
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import formats
from mimeo_amd.synth import flanked_tandem_genome, synth_genome, tandem_genome, write_fasta

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ['tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand']
SUB = np.array([[91, -114, -31, -123, -100], [-114, 100, -125, -31, -100], [-31, -125, 100, -114, -100],
                [-123, -31, -114, 91, -100], [-100, -100, -100, -100, -100]], dtype=np.int64)   # HOXD70, N = -100
CODE = np.full(256, 4, dtype=np.int64)
for _k, _c in enumerate(b'ACGT'):
    CODE[_c] = _k
    CODE[_c + 32] = _k
GAP_OPEN, GAP_EXTEND = 400, 30


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def revcomp(a):
    from tests import bounded_oracle as B
    return B.revcomp(a)


def _inputs():
    """(tag, T, Q, alignments the path rule keeps, is it the shortcut case) — the table of the issue"""
    _, s = tandem_genome(3, 2, 60_000)
    _, f = flanked_tandem_genome(1, 2)
    _, y = synth_genome(50, 200_000, 2, repeat_frac=0.2, families=5)
    return [('tandem (0, 1)', s[0], s[1], 10, False), ('tandem (0, 0)', s[0], s[0], 1, True),
            ('flanked, query reverse-complemented', f[0], revcomp(f[1]), 6, False), ('synth (0, 1)', y[0], y[1], 7, False)]


def _wide():
    from tests import bounded_oracle as B
    tag, T, Q, kw = [c for c in B.flanked_cases() if c[0][0] == 'ydrop 90000'][0]
    return T, Q, kw


def _oracle_job(args):
    from tests import paths_oracle as PO
    T, Q, rule, kw = args
    return PO.align_paths(T, Q, rule, **kw)


@pytest.fixture(scope='module')
def oracle():
    """{(input number, rule): (records, extended alignments)} and the wide-band case under 'wide': computed once, on a pool"""
    from tests import paths_oracle as PO
    PO.lib()   # build once, before the workers look for it
    ins = _inputs()
    jobs = [(T.tobytes(), Q.tobytes(), rule, {}) for _, T, Q, _, _ in ins for rule in (0, 1)]
    T, Q, kw = _wide()
    jobs.append((T.tobytes(), Q.tobytes(), 0, kw))
    with mp.get_context('spawn').Pool(min(9, os.cpu_count() or 1)) as pool:
        res = pool.map(_oracle_job, jobs, chunksize=1)
    out = {(k // 2, k % 2): res[k] for k in range(2 * len(ins))}
    out['wide'] = res[-1]
    return out


def nblocks_of_keys(keys):
    k = np.sort(keys)
    t, q = (k >> np.uint64(32)).astype(np.int64), (k & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return (1 + int(np.count_nonzero((np.diff(t) != 1) | (np.diff(q) != 1)))) if k.size else 0


def check_against_oracle(recs, first, blocks, orecs, ext, tag):
    from tests import paths_oracle as PO
    a, b = recs[COLS], orecs[COLS]
    assert a.size == b.size and (a == b).all(), (tag, a[:5], b[:5])
    assert first.size == recs.size + 1 and int(first[0]) == 0 and int(first[-1]) == blocks.size, tag
    index = {}
    for minus, at, aq, score, keys in ext:
        ks = np.sort(keys)
        index.setdefault((minus, score, int(ks[0]) if ks.size else -1), []).append(ks)
    for i in range(recs.size):
        k = PO.blocks_to_keys(blocks[int(first[i]):int(first[i + 1])])
        cand = index.get((int(recs['qstrand'][i]), int(recs['score'][i]), int(k[0]) if k.size else -1))
        assert cand is not None, (tag, i, recs[i])
        assert any(np.array_equal(c, k) for c in cand), (tag, i, recs[i])


def rescore(recs, first, blocks, seq_t, seq_q, tag):
    """Test 3.  seq_t / seq_q: tid / qid -> uint8 bases.  Score, matches and mismatches recomputed from the blocks equal the
    record's; the invariants of include/mimeo_hip.h hold."""
    rc = {}
    for i in range(recs.size):
        r = recs[i]
        b = blocks[int(first[i]):int(first[i + 1])]
        assert b.size >= 1, (tag, i)
        T = seq_t[int(r['tid'])]
        qid, Lq = int(r['qid']), int(seq_q[int(r['qid'])].size)
        if int(r['qstrand']):
            if qid not in rc:
                rc[qid] = revcomp(seq_q[qid])
            Q = rc[qid]
        else:
            Q = seq_q[qid]
        t, q, ln = b['t'].astype(np.int64), b['q'].astype(np.int64), b['len'].astype(np.int64)
        assert (ln >= 1).all(), (tag, i)
        dt, dq = t[1:] - (t[:-1] + ln[:-1]), q[1:] - (q[:-1] + ln[:-1])
        assert (dt >= 0).all() and (dq >= 0).all() and ((dt > 0) | (dq > 0)).all(), (tag, i, b)   # increasing, never touching on a diagonal
        assert int(t[0]) == int(r['tstart']) and int(t[-1] + ln[-1]) == int(r['tend']), (tag, i)
        q_first, q_end = int(q[0]), int(q[-1] + ln[-1])
        if int(r['qstrand']):
            assert (int(r['qstart']), int(r['qend'])) == (Lq - q_end, Lq - q_first), (tag, i)
        else:
            assert (int(r['qstart']), int(r['qend'])) == (q_first, q_end), (tag, i)
        assert int(ln.sum()) == int(r['id_d']), (tag, i)
        score = nm = 0
        for k in range(b.size):
            x, y = CODE[T[int(t[k]):int(t[k] + ln[k])]], CODE[Q[int(q[k]):int(q[k] + ln[k])]]
            score += int(SUB[x, y].sum())
            nm += int(np.count_nonzero((x == y) & (x < 4)))
        for g in np.concatenate([dt[dt > 0], dq[dq > 0]]).tolist():
            score -= GAP_OPEN + GAP_EXTEND * int(g)
        assert score == int(r['score']), (tag, i, score, int(r['score']))
        assert nm == int(r['id_n']) and int(ln.sum()) - nm == int(r['id_d']) - int(r['id_n']), (tag, i)


@pytest.mark.parametrize('rule', [0, 1], ids=['box', 'path'])
@pytest.mark.parametrize('k', [0, 1, 2, 3])
def test_paths_equal_the_oracle_and_rescore(eng, oracle, k, rule):
    """Tests 1, 2 and 3 of the issue on each of the four inputs under both rules."""
    tag, T, Q, kept_path_rule, shortcut = _inputs()[k]
    orecs, ext = oracle[(k, rule)]
    # the case shows something: asserted on the oracle's side
    kept = [e for e in ext if e[3] >= 3000]
    assert len(kept) == orecs.size
    if rule == 1:
        assert orecs.size == kept_path_rule, (tag, orecs.size)
    most = max(nblocks_of_keys(e[4]) for e in kept)
    assert most == 1 if shortcut else most > 1, (tag, most)
    if k in (2, 3):
        assert sum(e[0] for e in kept) >= (len(kept) if k == 2 else 1), 'no minus-strand alignment with gaps in this case'
    g = eng.Genome(['t', 'q'], [T, Q])
    prm = eng.default_params(anchor_rule=rule)
    recs, first, blocks = eng.align_units(g, None, [(0, 1, 3)], prm, paths=True)
    assert not eng.failed_pairs()
    plain = eng.align_units(g, None, [(0, 1, 3)], prm)
    assert recs.tobytes() == plain.tobytes(), tag   # test 2: the records are untouched
    check_against_oracle(recs, first, blocks, orecs, ext, (tag, rule))
    rescore(recs, first, blocks, {0: T}, {1: Q}, (tag, rule))
    if shortcut:
        assert blocks.size == 1 and blocks[0].tolist() == (0, 0, T.size)   # the identical-suffix shortcut's diagonal, both halves merged
    g.close()


def _rows(recs, first, blocks):
    return sorted(recs[i].tobytes() + blocks[int(first[i]):int(first[i + 1])].tobytes() for i in range(recs.size))


def test_layout_independence(eng, monkeypatch, capfd):
    """Test 4: all 64 pairs of an 8-scaffold tandem genome, box rule with paths: the same (record, path) set whatever the
    layout (super-scaffolds, mirror units, index blocks), the round structure, the slices of the trace pass or the entry point."""
    names, seqs = tandem_genome(7, 8, 150_000)
    n = len(names)
    A = eng.Genome(names, seqs)
    pairs = [(t, q) for t in range(n) for q in range(n)]
    monkeypatch.setenv('MIMEO_K6_STATS', '1')
    capfd.readouterr()
    recs, first, blocks = eng.align_pairs(A, None, pairs, paths=True)
    lines = [l for l in capfd.readouterr().err.splitlines() if 'paths out: traceback' in l]
    monkeypatch.delenv('MIMEO_K6_STATS')
    assert eng.stats()['super_units'] > 0 and not eng.failed_pairs() and lines
    assert recs.tobytes() == eng.align_pairs(A, None, pairs).tobytes()
    assert int(np.diff(first.astype(np.int64)).max()) > 1
    seq = dict(enumerate(seqs))
    rescore(recs, first, blocks, seq, seq, 'all pairs')
    ref = _rows(recs, first, blocks)
    pool_mb = str(int(max(float(l.split('largest half ')[1].split()[0]) for l in lines)) + 1)
    for env in ({'MIMEO_PACK': '0'}, {'MIMEO_MIRROR': '0'}, {'MIMEO_PACK': '0', 'MIMEO_INDEX_BUDGET_MB': '300'}, {'MIMEO_K6_BMAX': '1'},
                {'MIMEO_K6_TRACE_POOL_MB': pool_mb, 'MIMEO_K6_STATS': '1'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        alt = eng.align_pairs(A, None, pairs, paths=True)
        err = capfd.readouterr().err
        assert not eng.failed_pairs(), env
        assert _rows(*alt) == ref, env
        if 'MIMEO_INDEX_BUDGET_MB' in env:
            assert eng.stats()['index_blocks'] > 1
        if 'MIMEO_K6_TRACE_POOL_MB' in env:
            sl = [int(l.split('slices ')[1].split(',')[0]) for l in err.splitlines() if 'paths out: traceback' in l]
            assert sl and max(sl) > 1, err[-2000:]
        for k in env:
            monkeypatch.delenv(k)
    units = eng.align_units(A, None, [(t, q, 3) for t, q in pairs], paths=True)
    assert units[0].tobytes() == recs.tobytes() and _rows(*units) == ref
    twice = eng.align_pairs(A, None, pairs + [pairs[10]], paths=True)
    t, q = pairs[10]
    dup = np.flatnonzero((recs['tid'] == t) & (recs['qid'] == q))
    assert dup.size >= 1
    assert twice[0].tobytes() == recs.tobytes() + recs[dup].tobytes()
    assert _rows(*twice) == sorted(ref + _rows(recs[dup], *formats.select_paths(first, blocks, dup)))
    A.close()


def test_wide_band(eng, oracle):
    """Test 5: y-drop 90000 on a flanked array: bands beyond the register kernels (k6_dp_any), the trace's score ring in the pool."""
    T, Q, kw = _wide()
    orecs, ext = oracle['wide']
    assert max(nblocks_of_keys(e[4]) for e in ext if e[3] >= 3000) > 1
    g = eng.Genome(['t', 'q'], [T, Q])
    recs, first, blocks = eng.align_units(g, None, [(0, 1, 3)], eng.default_params(**kw), paths=True)
    assert not eng.failed_pairs()
    check_against_oracle(recs, first, blocks, orecs, ext, 'wide')
    g.close()


def test_trace_pool_too_small_for_one_half(eng, monkeypatch):
    """Test 6: with paths the pair is left out with MIMEO_ERR_LIMIT and the call returns 0; without, nothing changes."""
    _, s = tandem_genome(3, 2, 60_000)
    g = eng.Genome(['t', 'q'], [s[0], s[1]])
    full = eng.align_units(g, None, [(0, 1, 3)])
    assert full.size >= 2
    monkeypatch.setenv('MIMEO_K6_TRACE_POOL_MB', '1')
    recs, first, blocks = eng.align_units(g, None, [(0, 1, 3)], paths=True)
    assert eng.failed_pairs() == [(0, -5)]   # MIMEO_ERR_LIMIT
    assert recs.size == 0 and first.size == recs.size + 1 and blocks.size == 0
    plain = eng.align_units(g, None, [(0, 1, 3)])
    assert not eng.failed_pairs() and plain.tobytes() == full.tobytes()
    g.close()


def test_ungapped_one_block_per_alignment(eng):
    """Test 7: gapped = 0: the block of an alignment is its box."""
    _, s = synth_genome(50, 200_000, 2, repeat_frac=0.2, families=5)
    g = eng.Genome(['t', 'q'], [s[0], s[1]])
    prm = eng.default_params(gapped=0)
    recs, first, blocks = eng.align_units(g, None, [(0, 1, 3)], prm, paths=True)
    assert recs.tobytes() == eng.align_units(g, None, [(0, 1, 3)], prm).tobytes()
    assert recs.size >= 2 and set(recs['qstrand'].tolist()) == {0, 1}
    assert first.tolist() == list(range(recs.size + 1)) and blocks.size == recs.size
    minus = recs['qstrand'] != 0
    assert (blocks['t'] == recs['tstart']).all() and (blocks['len'] == recs['tend'] - recs['tstart']).all()
    assert (blocks['len'] == recs['qend'] - recs['qstart']).all()
    assert (blocks['q'] == np.where(minus, s[1].size - recs['qend'].astype(np.int64), recs['qstart'].astype(np.int64))).all()
    g.close()


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


def test_cli_self_paf(eng, tmp_path):
    """Test 8: `mimeo self --paf`: TAB and GFF3 byte-identical to a run without the flag; one PAF row per TAB row in the
    TAB's order with the TAB's coordinates; the CIGARs rescore to the TAB's scores."""
    from mimeo_amd import _ffi
    names, seqs = synth_genome(50, 300_000, 3, repeat_frac=0.2, families=5)
    fa = str(tmp_path / 'g.fa')
    write_fasta(fa, names, seqs)
    out = {}
    for tag, extra in (('plain', []), ('paf', ['--paf', str(tmp_path / 'x.paf')])):
        d = tmp_path / tag
        r = subprocess.run([sys.executable, '-m', 'mimeo_amd', 'self', '--afasta', fa, '-d', str(d)] + extra, cwd=ROOT, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[tag] = ((d / 'mimeo_alignment.tab').read_bytes(), (d / 'mimeo-self_repeats.gff3').read_bytes(), sorted(os.listdir(d)))
    assert out['plain'] == out['paf']
    tab = [l.split('\t') for l in out['paf'][0].decode().splitlines()[1:]]
    paf = [l.split('\t') for l in (tmp_path / 'x.paf').read_text().splitlines()]
    assert len(tab) == len(paf) > 3
    idx, length = {n: i for i, n in enumerate(names)}, {n: int(s.size) for n, s in zip(names, seqs)}
    recs = np.zeros(len(tab), dtype=_ffi.ALIGNMENT)
    blocks, first = [], [0]
    gapped = 0
    for i, (t, p) in enumerate(zip(tab, paf)):
        assert len(p) == 14 and p[11] == '255'
        assert (p[5], p[0], p[4]) == (t[0], t[4], t[5])
        assert (int(p[7]), int(p[8]), int(p[2]), int(p[3])) == (int(t[2]) - 1, int(t[3]), int(t[6]) - 1, int(t[7]))
        assert (int(p[6]), int(p[1])) == (length[p[5]], length[p[0]])
        assert p[12] == 'AS:i:' + t[8] and p[13].startswith('cg:Z:')
        minus = p[4] == '-'
        b = _cigar_blocks(int(p[7]), length[p[0]] - int(p[3]) if minus else int(p[2]), p[13][5:])
        gapped += len(b) > 1
        r = recs[i]
        r['tid'], r['qid'], r['qstrand'] = idx[p[5]], idx[p[0]], int(minus)
        r['tstart'], r['tend'], r['qstart'], r['qend'], r['score'], r['id_n'] = int(p[7]), int(p[8]), int(p[2]), int(p[3]), int(t[8]), int(p[9])
        r['id_d'] = sum(x[2] for x in b)
        assert int(p[10]) == int(r['id_d']) + (int(p[8]) - int(p[7]) - int(r['id_d'])) + (int(p[3]) - int(p[2]) - int(r['id_d']))
        assert '%.1f' % (100.0 * int(p[9]) / int(r['id_d'])) == t[9]
        blocks += b
        first.append(len(blocks))
    assert gapped >= 1
    seq = dict(enumerate(seqs))
    rescore(recs, np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK), seq, seq, 'cli')
