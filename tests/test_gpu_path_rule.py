"""The path anchor rule of the gapped stage (mimeo_params.anchor_rule = MIMEO_ANCHOR_PATH, CLI --anchorRule path) against its
specification, the study oracle (oracle/box_vs_path.c, orc_align_pair_rule(..., path_rule=1)): an anchor is skipped iff it
is a match/mismatch column of the path of an earlier alignment of its (pair, strand).  Tandem-array genomes
(mimeo_amd.synth.tandem_genome) are where the box and path rules part; every case below checks that they do."""
import multiprocessing as mp
import os

import numpy as np
import pytest

from mimeo_amd.synth import synth_genome, tandem_genome

pytestmark = pytest.mark.gpu

COLS = ['tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand']


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def _rule_job(args):
    from tests import study_oracle as S
    T, Q, rule, kw = args
    return S.align_rule(T, Q, rule, **kw)


def oracle_many(jobs):
    """[(T bytes, Q bytes, rule, oracle params)] -> [records], on a pool of fresh processes"""
    from tests import study_oracle as S
    S.lib()   # build once, before the workers look for it
    with mp.get_context('spawn').Pool(min(8, os.cpu_count() or 1)) as pool:
        return pool.map(_rule_job, jobs, chunksize=1)


def _cmp(got, exp, tag):
    a, b = got[COLS], exp[COLS]
    assert a.size == b.size, (tag, a.size, b.size, a[:5], b[:5])
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (tag, a[bad[:5]], b[bad[:5]])


def _by_pair(recs, pairs):
    return {pr: recs[(recs['tid'] == pr[0]) & (recs['qid'] == pr[1])] for pr in pairs}


@pytest.mark.parametrize('seed,nscaf,scaf_bp', [(3, 3, 200_000), (11, 3, 200_000), (21, 2, 300_000), (29, 4, 150_000)])
def test_path_rule_equals_study_oracle(eng, seed, nscaf, scaf_bp):
    names, seqs = tandem_genome(seed, nscaf, scaf_bp)
    g = eng.Genome(names, seqs)
    pairs = [(t, (t + 1) % nscaf) for t in range(nscaf)]
    jobs = [(seqs[t].tobytes(), seqs[q].tobytes(), rule, {}) for t, q in pairs for rule in (1, 0)]
    exp = oracle_many(jobs)
    parted = 0
    for k, (t, q) in enumerate(pairs):
        path, box = exp[2 * k], exp[2 * k + 1]
        parted += box.tobytes() != path.tobytes()
        got = eng.align_pair(g, t, g, q, eng.default_params(anchor_rule=1))
        _cmp(got, path, (seed, t, q))
    assert parted, 'the rules do not part on this genome: the case shows nothing'
    g.close()


def test_box_rule_explicit_equals_default(eng):
    from oracle import oracle as O
    names, seqs = tandem_genome(3, 3, 200_000)
    g = eng.Genome(names, seqs)
    dflt = eng.align_pair(g, 0, g, 1)
    box = eng.align_pair(g, 0, g, 1, eng.default_params(anchor_rule=0))
    assert dflt.tobytes() == box.tobytes()
    _cmp(box, O.align_pair(seqs[0].tobytes(), seqs[1].tobytes()), 'box')
    path = eng.align_pair(g, 0, g, 1, eng.default_params(anchor_rule=1))
    assert path.tobytes() != box.tobytes()
    g.close()


def test_path_rule_all_layouts(eng, monkeypatch, capfd):
    """Every ordered pair of an 8-scaffold tandem genome (the packed path: super-scaffolds, mirrored plus strand) against the
    oracle pair by pair; then the same records under every switch that changes the layout or the round structure, and
    through mimeo_align_units."""
    names, seqs = tandem_genome(7, 8, 150_000)
    n = len(names)
    A = eng.Genome(names, seqs)
    pairs = [(t, q) for t in range(n) for q in range(n)]
    prm = eng.default_params(anchor_rule=1)
    whole = eng.align_pairs(A, None, pairs, prm)
    assert eng.stats()['super_units'] > 0 and not eng.failed_pairs()
    exp = oracle_many([(seqs[t].tobytes(), seqs[q].tobytes(), 1, {}) for t, q in pairs])
    got = _by_pair(whole, pairs)
    box = _by_pair(eng.align_pairs(A, None, pairs), pairs)
    parted = 0
    for k, pr in enumerate(pairs):
        _cmp(got[pr], exp[k], pr)
        parted += got[pr].tobytes() != box[pr].tobytes()
    assert parted >= 2
    key = lambda r: np.sort(r, order=['tid', 'qid'] + COLS)
    ref = key(whole)
    # a pool just above the largest half's traceback: several slices per round (counted in the K6 statistics line)
    monkeypatch.setenv('MIMEO_K6_STATS', '1')
    capfd.readouterr()
    eng.align_pairs(A, None, pairs, prm)
    line = [l for l in capfd.readouterr().err.splitlines() if 'path rule: traceback' in l][-1]
    monkeypatch.delenv('MIMEO_K6_STATS')
    pool_mb = str(int(float(line.split('largest half ')[1].split()[0])) + 1)
    for env in ({'MIMEO_PACK': '0'}, {'MIMEO_MIRROR': '0'}, {'MIMEO_PACK': '0', 'MIMEO_INDEX_BUDGET_MB': '300'},
                {'MIMEO_K6_BMAX': '1'}, {'MIMEO_K6_BMAX': '4'},
                {'MIMEO_K6_TRACE_POOL_MB': pool_mb, 'MIMEO_K6_STATS': '1'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        alt = eng.align_pairs(A, None, pairs, prm)
        err = capfd.readouterr().err
        assert not eng.failed_pairs(), env
        assert key(alt).tobytes() == ref.tobytes(), env
        if 'MIMEO_INDEX_BUDGET_MB' in env:
            assert eng.stats()['index_blocks'] > 1
        if 'MIMEO_K6_TRACE_POOL_MB' in env:
            lines = [l for l in err.splitlines() if 'path rule: traceback' in l]
            assert lines and any(int(l.split('slices ')[1].split()[0].rstrip(',')) > int(l.split('rounds ')[1].split()[0]) for l in lines), lines
        for k in env:
            monkeypatch.delenv(k)
    units = eng.align_units(A, None, [(t, q, 3) for t, q in pairs], prm)
    assert key(units).tobytes() == ref.tobytes()
    A.close()


def test_path_rule_wide_bands_long_halves_and_self(eng, monkeypatch):
    """Bands beyond 2048 columns (k6_dp_any; the trace keeps its rows in the pool), the 300 kb extension under a low score cap
    (k6_dp_any rebases its cells, and so does k6_trace: the cap reaches the trace, whose re-run shares the band DP and its rebase),
    and the (A, A) self pair whose identical-suffix shortcut has the diagonal as its path."""
    names, seqs = synth_genome(97, 120_000, 2, repeat_frac=0.2, families=2, cons_len=(800, 2000), max_div=0.1)
    tn, tseqs = tandem_genome(11, 2, 200_000)
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
    jobs = [(seqs[0].tobytes(), seqs[1].tobytes(), 1, {'ydrop': 90000}), (seqs[0].tobytes(), seqs[1].tobytes(), 0, {'ydrop': 90000}),
            (LT.tobytes(), LQ.tobytes(), 1, {'strand': 1}),
            (tseqs[0].tobytes(), tseqs[0].tobytes(), 1, {}), (tseqs[1].tobytes(), tseqs[1].tobytes(), 1, {})]
    exp = oracle_many(jobs)
    g = eng.Genome(names, seqs)
    got = eng.align_pair(g, 0, g, 1, eng.default_params(ydrop=90000, anchor_rule=1))
    _cmp(got, exp[0], 'wide')
    g.close()
    monkeypatch.setenv('MIMEO_K6_SCORE_CAP', '100000')
    g = eng.Genome(['t', 'q'], [LT, LQ])
    got = eng.align_pair(g, 0, g, 1, eng.default_params(strand=1, anchor_rule=1))
    assert int((exp[2]['tend'] - exp[2]['tstart']).max()) > 280_000
    _cmp(got, exp[2], 'long')
    g.close()
    monkeypatch.delenv('MIMEO_K6_SCORE_CAP')
    g = eng.Genome(tn, tseqs)
    for k in (0, 1):
        _cmp(eng.align_pair(g, k, g, k, eng.default_params(anchor_rule=1)), exp[3 + k], ('self', k))
    g.close()


def test_path_rule_penalties_beyond_the_lean_kernel(eng):
    """Penalties the lean kernel cannot hold (every job of a round goes to the 2048-column kernel): the traceback re-runs
    those halves and the alignments equal the oracle's.  The third set of test_gpu_align's BEYOND_LEAN, a y-drop beyond
    2^28, is left to the box rule there: the traceback sizes a row by y-drop / gap extend, 18 million columns, and would
    reserve gigabytes of trace pool for a 925 bp alignment."""
    names, seqs = synth_genome(97, 6000, 2, repeat_frac=0.3, families=2, cons_len=(800, 1500), max_div=0.1)
    sets = [{'gap_extend': 70000}, {'gap_open': (1 << 24) + 1}]
    exp = oracle_many([(seqs[0].tobytes(), seqs[1].tobytes(), 1, kw) for kw in sets])
    g = eng.Genome(names, seqs)
    for kw, e in zip(sets, exp):
        assert e.size >= 1
        _cmp(eng.align_pair(g, 0, g, 1, eng.default_params(anchor_rule=1, **kw)), e, kw)
    g.close()


def test_trace_pool_too_small_fails_the_pair_only(eng, monkeypatch):
    """A half whose traceback alone exceeds the pool fails its pair (MIMEO_ERR_LIMIT, as a DP band beyond the limit); the
    other pairs are returned and equal the oracle."""
    names, seqs = tandem_genome(5, 3, 200_000)
    A = eng.Genome(names, seqs)
    pairs = [(t, q) for t in range(3) for q in range(3)]
    exp = oracle_many([(seqs[t].tobytes(), seqs[q].tobytes(), 1, {}) for t, q in pairs])
    monkeypatch.setenv('MIMEO_K6_TRACE_POOL_MB', '1')
    got = _by_pair(eng.align_pairs(A, None, pairs, eng.default_params(anchor_rule=1)), pairs)
    failed = eng.failed_pairs()
    assert failed and len(failed) < len(pairs), failed
    assert all(code == -5 for _, code in failed)   # MIMEO_ERR_LIMIT
    bad = {int(i) for i, _ in failed}
    for k, pr in enumerate(pairs):
        if k in bad:
            assert got[pr].size == 0
        else:
            _cmp(got[pr], exp[k], pr)
    A.close()


def test_bad_anchor_rule_is_an_argument_error(eng):
    import ctypes as C
    from mimeo_amd import _ffi
    names, seqs = synth_genome(5, 40_000, 1)
    g = eng.Genome(names, seqs)
    p = eng.default_params(anchor_rule=2)
    ptr, n = C.c_void_p(), C.c_uint64()
    rc = _ffi.load().mimeo_align_pair(g._h, 0, g._h, 0, C.byref(p), C.byref(ptr), C.byref(n))
    assert rc == -1 and 'anchor_rule' in eng.last_error()   # MIMEO_ERR_ARG
    g.close()


def test_cli_self_path_rule_end_to_end(eng, tmp_path):
    """`mimeo self --anchorRule path` on a tandem FASTA: TAB and GFF3 equal to the oracle pipeline fed with path-rule
    alignments, and different from the --anchorRule box run."""
    import subprocess
    import sys
    from oracle import pipeline as P
    from mimeo_amd.synth import write_fasta
    names, seqs = tandem_genome(11, 3, 200_000)
    fa = str(tmp_path / 'g.fa')
    write_fasta(fa, names, seqs)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for rule in ('path', 'box'):
        d = tmp_path / rule
        r = subprocess.run([sys.executable, '-m', 'mimeo_amd', 'self', '--afasta', fa, '-d', str(d), '--minIdt', '80', '--minLen', '100',
                            '--minCov', '2', '--anchorRule', rule], cwd=root, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout + r.stderr
        out[rule] = ((d / 'mimeo_alignment.tab').read_text(), (d / 'mimeo-self_repeats.gff3').read_text())
    pairs = [(a, b) for a in range(3) for b in range(3)]
    alns = oracle_many([(seqs[t].tobytes(), seqs[q].tobytes(), 1, {}) for t, q in pairs])
    tab = ['#name1\tstrand1\tstart1\tend1\tname2\tstrand2\tstart2+\tend2+\tscore\tidentity']
    for (t, q), al in zip(pairs, alns):
        al['tid'], al['qid'] = t, q
        tab += P.filter_project_sort('\n'.join(P.general_rows(names, names, [len(s) for s in seqs], al)) + '\n', 100, 80)
    assert out['path'][0] == '\n'.join(tab) + '\n'
    bed = P.bed_project_sort(tab)
    iv = [(l.split('\t')[0], int(l.split('\t')[1]), int(l.split('\t')[2])) for l in bed]
    regs = P.coverage_collapse(iv, {n: len(s) for n, s in zip(names, seqs)}, 2, 100)
    gff = P.gff_self_lines(regs, 'Self_Repeat', 'Self_Repeat', source='mimeo-self')
    assert len(gff) > 2
    assert out['path'][1] == '\n'.join(gff) + '\n'   # gff_self_lines starts with the two header lines
    assert out['path'][0] != out['box'][0]
