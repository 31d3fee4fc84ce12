"""Bounded gapped extensions (mimeo_params.bound_extensions = 1 with the path anchor rule; CLI --anchorRule path
--boundExtensions) against their specification, tests/bounded_oracle.c: every engine record equals the specification's byte
for byte.  The flanked-array cases (mimeo_amd.synth.flanked_tandem_genome) are those on which bounded and unbounded path rule
part — tests/test_host_bounds.py asserts that for each of them with the specification alone."""
import os
import time
from contextlib import contextmanager

import numpy as np
import pytest

from mimeo_amd.synth import flanked_tandem_genome, tandem_genome
from tests import bounded_oracle as B

pytestmark = pytest.mark.gpu

COLS = ['tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand']
CALL_BUDGET_S = 120.0   # per engine call: the largest case here (64 pairs of 50 kbp, one anchor per round) takes seconds


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


@contextmanager
def budget(tag, seconds=CALL_BUDGET_S):
    t0 = time.perf_counter()
    yield
    dt = time.perf_counter() - t0
    assert dt < seconds, '%s took %.1f s (budget %.0f s)' % (tag, dt, seconds)


def _cmp(got, exp, tag):
    a, b = got[COLS], exp[COLS]
    assert a.size == b.size, (tag, a.size, b.size, a[:5], b[:5])
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (tag, a[bad[:5]], b[bad[:5]])


def _by_pair(recs, pairs):
    return {pr: recs[(recs['tid'] == pr[0]) & (recs['qid'] == pr[1])] for pr in pairs}


def _prm(eng, **kw):
    return eng.default_params(anchor_rule=1, bound_extensions=1, **kw)


def test_flanked_pairs_equal_the_specification(eng):
    """six flanked pairs and one whose query is given reverse-complemented (both strands each); a flanked scaffold against
    itself with every HSP an anchor: once the main diagonal is accepted, the identical-suffix shortcut of the other anchors'
    halves is off (an earlier alignment reaches into their rows); y-drop 90000: every band outgrows the register kernel and
    the bounded k6_dp_any runs it"""
    cases = B.flanked_cases()
    exp = B.many([(T.tobytes(), Q.tobytes(), b, kw) for _, T, Q, kw in cases for b in (1, 0)])
    for k, (tag, T, Q, kw) in enumerate(cases):
        g = eng.Genome(['t', 'q'], [T, Q])
        with budget(tag):
            got = eng.align_pair(g, 0, g, 1, _prm(eng, **kw))
        _cmp(got, exp[2 * k], tag)
        with budget(tag):
            unb = eng.align_pair(g, 0, g, 1, eng.default_params(anchor_rule=1, **kw))
        _cmp(unb, exp[2 * k + 1], (tag, 'unbounded'))
        assert got[COLS].tobytes() != unb[COLS].tobytes(), tag
        g.close()


@pytest.mark.parametrize('seed,nscaf,scaf_bp', [(3, 3, 200_000), (11, 3, 200_000), (21, 2, 300_000), (29, 4, 150_000)])
def test_tandem_genomes_equal_the_specification(eng, seed, nscaf, scaf_bp):
    """the cases of test_gpu_path_rule.test_path_rule_equals_study_oracle: units of 150-900 bp, no homologous flanks"""
    names, seqs = tandem_genome(seed, nscaf, scaf_bp)
    g = eng.Genome(names, seqs)
    pairs = [(t, (t + 1) % nscaf) for t in range(nscaf)]
    exp = B.many([(seqs[t].tobytes(), seqs[q].tobytes(), 1, {}) for t, q in pairs])
    for k, (t, q) in enumerate(pairs):
        with budget((seed, t, q)):
            got = eng.align_pair(g, t, g, q, _prm(eng))
        _cmp(got, exp[k], (seed, t, q))
    g.close()


def _stats_line(err):
    line = [l for l in err.splitlines() if 'path rule: traceback' in l][-1]
    return line, int(line.split('bounded jobs ')[1].split(',')[0]), int(line.split('rescheduled ')[1].split()[0])


def test_flanked_genome_all_layouts(eng, monkeypatch, capfd):
    """Every ordered pair of an 8-scaffold flanked genome (the packed path) against the specification pair by pair; then the
    same records under every switch that changes the layout or the round structure, and through mimeo_align_units.  The rule
    is sequential and the rounds are speculative: with the default batch some anchor's extension is bounded by an alignment
    accepted after it ran and is run again; with one anchor per round none is."""
    names, seqs = flanked_tandem_genome(B.FLANKED_GENOME_SEED, 8)
    n = len(names)
    A = eng.Genome(names, seqs)
    pairs = [(t, q) for t in range(n) for q in range(n)]
    prm = _prm(eng)
    monkeypatch.setenv('MIMEO_K6_STATS', '1')
    capfd.readouterr()
    with budget('align_pairs'):
        whole = eng.align_pairs(A, None, pairs, prm)
    line, bjobs, resched = _stats_line(capfd.readouterr().err)
    monkeypatch.delenv('MIMEO_K6_STATS')
    assert eng.stats()['super_units'] > 0 and not eng.failed_pairs()
    assert bjobs > 0 and resched > 0, line
    exp = B.many([(seqs[t].tobytes(), seqs[q].tobytes(), 1, {}) for t, q in pairs])
    got = _by_pair(whole, pairs)
    unb = _by_pair(eng.align_pairs(A, None, pairs, eng.default_params(anchor_rule=1)), pairs)
    parted = 0
    for k, pr in enumerate(pairs):
        _cmp(got[pr], exp[k], pr)
        parted += got[pr][COLS].tobytes() != unb[pr][COLS].tobytes()
    assert parted >= 8, parted
    key = lambda r: np.sort(r, order=['tid', 'qid'] + COLS)
    ref = key(whole)
    pool_mb = str(int(float(line.split('largest half ')[1].split()[0])) + 1)
    for env in ({'MIMEO_PACK': '0'}, {'MIMEO_MIRROR': '0'}, {'MIMEO_PACK': '0', 'MIMEO_INDEX_BUDGET_MB': '300'},
                {'MIMEO_K6_BMAX': '1', 'MIMEO_K6_STATS': '1'}, {'MIMEO_K6_BMAX': '4'},
                {'MIMEO_K6_TRACE_POOL_MB': pool_mb, 'MIMEO_K6_STATS': '1'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        with budget(env):
            alt = eng.align_pairs(A, None, pairs, prm)
        err = capfd.readouterr().err
        assert not eng.failed_pairs(), env
        assert key(alt).tobytes() == ref.tobytes(), env
        if 'MIMEO_INDEX_BUDGET_MB' in env:
            assert eng.stats()['index_blocks'] > 1
        if 'MIMEO_K6_BMAX' in env and 'MIMEO_K6_STATS' in env:
            l1, b1, r1 = _stats_line(err)
            assert r1 == 0 and b1 > 0, l1   # the lowest unfinalised anchor of a group is always valid when it runs
        if 'MIMEO_K6_TRACE_POOL_MB' in env:
            lines = [l for l in err.splitlines() if 'path rule: traceback' in l]
            assert lines and any(int(l.split('slices ')[1].split()[0].rstrip(',')) > int(l.split('rounds ')[1].split()[0]) for l in lines), lines
        for k in env:
            monkeypatch.delenv(k)
    with budget('align_units'):
        units = eng.align_units(A, None, [(t, q, 3) for t, q in pairs], prm)
    assert key(units).tobytes() == ref.tobytes()
    A.close()


def test_long_half_under_a_low_score_cap(eng, monkeypatch):
    """The 300 kb extension under a low score cap: too many rows for the register kernel, so the bounded k6_dp_any runs it
    and rebases its cells, and the bounded trace re-run, which takes the same cap and rebases as it goes, ends on the same
    cell.  (Bands beyond the register kernel: the y-drop 90000 case of bounded_oracle.flanked_cases.)"""
    rng = np.random.default_rng(123)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    core = rng.integers(0, 4, 300_000)
    mut = core.copy()
    sub = rng.random(core.size) < 0.03
    mut[sub] = (mut[sub] + rng.integers(1, 4, int(sub.sum()))) & 3
    for p in sorted(rng.integers(1000, core.size - 1000, 40).tolist(), reverse=True):  # indels of 1-3 bases
        mut = np.delete(mut, slice(p, p + int(rng.integers(1, 4)))) if rng.random() < 0.5 else np.insert(mut, p, rng.integers(0, 4, int(rng.integers(1, 4))))
    LT = acgt[np.concatenate([rng.integers(0, 4, 5000), core, rng.integers(0, 4, 5000)])]
    LQ = acgt[np.concatenate([rng.integers(0, 4, 3000), mut, rng.integers(0, 4, 3000)])]
    exp = B.align_bounded(LT.tobytes(), LQ.tobytes(), 1, strand=1)
    monkeypatch.setenv('MIMEO_K6_SCORE_CAP', '100000')
    g = eng.Genome(['t', 'q'], [LT, LQ])
    with budget('long'):
        got = eng.align_pair(g, 0, g, 1, _prm(eng, strand=1))
    assert int((exp['tend'] - exp['tstart']).max()) > 280_000
    _cmp(got, exp, 'long')
    g.close()
    monkeypatch.delenv('MIMEO_K6_SCORE_CAP')


def test_the_two_argument_errors(eng):
    import ctypes as C
    from mimeo_amd import _ffi
    _, seqs = flanked_tandem_genome(1, 1, flank=2000)
    g = eng.Genome(['a'], seqs)
    ptr, n = C.c_void_p(), C.c_uint64()

    def rc_of(p):
        return _ffi.load().mimeo_align_pair(g._h, 0, g._h, 0, C.byref(p), C.byref(ptr), C.byref(n))

    assert rc_of(eng.default_params(anchor_rule=1, bound_extensions=2)) == -1 and 'bound_extensions' in eng.last_error()   # MIMEO_ERR_ARG
    assert rc_of(eng.default_params(anchor_rule=0, bound_extensions=1)) == -1 and 'bound_extensions' in eng.last_error()
    assert rc_of(eng.default_params(anchor_rule=1, bound_extensions=1)) == 0
    if ptr.value:
        _ffi.load().mimeo_free(ptr)
    g.close()


def test_cli_self_bound_extensions_end_to_end(eng, tmp_path):
    """`mimeo self --anchorRule path --boundExtensions` on a flanked FASTA: TAB and GFF3 equal to the oracle pipeline fed with
    the specification's alignments, and different from the run without the flag."""
    import subprocess
    import sys
    from oracle import pipeline as P
    from mimeo_amd.synth import write_fasta
    names, seqs = flanked_tandem_genome(B.FLANKED_GENOME_SEED, 4)
    fa = str(tmp_path / 'g.fa')
    write_fasta(fa, names, seqs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for tag, extra in (('bounded', ['--boundExtensions']), ('path', [])):
        d = tmp_path / tag
        r = subprocess.run([sys.executable, '-m', 'mimeo_amd', 'self', '--afasta', fa, '-d', str(d), '--minIdt', '80', '--minLen', '100',
                            '--minCov', '3', '--anchorRule', 'path'] + extra, cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[tag] = ((d / 'mimeo_alignment.tab').read_text(), (d / 'mimeo-self_repeats.gff3').read_text())
    pairs = [(a, b) for a in range(4) for b in range(4)]
    alns = B.many([(seqs[t].tobytes(), seqs[q].tobytes(), 1, {}) for t, q in pairs])
    tab = ['#name1\tstrand1\tstart1\tend1\tname2\tstrand2\tstart2+\tend2+\tscore\tidentity']
    for (t, q), al in zip(pairs, alns):
        al['tid'], al['qid'] = t, q
        tab += P.filter_project_sort('\n'.join(P.general_rows(names, names, [len(s) for s in seqs], al)) + '\n', 100, 80)
    assert out['bounded'][0] == '\n'.join(tab) + '\n'
    bed = P.bed_project_sort(tab)
    iv = [(l.split('\t')[0], int(l.split('\t')[1]), int(l.split('\t')[2])) for l in bed]
    regs = P.coverage_collapse(iv, {n: len(s) for n, s in zip(names, seqs)}, 3, 100)
    gff = P.gff_self_lines(regs, 'Self_Repeat', 'Self_Repeat', source='mimeo-self')
    assert len(gff) > 2
    assert out['bounded'][1] == '\n'.join(gff) + '\n'   # gff_self_lines starts with the two header lines
    assert out['bounded'][0] != out['path'][0]
