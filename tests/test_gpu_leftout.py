"""The "left out" contract (include/mimeo_hip.h, mimeo_align_units / mimeo_get_failed_pairs) on every path, entry point and
rank count, on the designed genome of tests/leftout_cases.py under MIMEO_K6_TRACE_POOL_MB=1: the scaffold pairs F of the
design — and no other — are left out, every entry of the list that names one is reported once and has no rows, every other
pair equals the uncapped oracle, and a job of N ranks writes the files of one process."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import formats, workflow
from mimeo_amd.dist import BOTH, MINUS, PLUS, Dist, deal_units, shard_pairs_by_target
from mimeo_amd.synth import write_fasta
from tests import leftout_cases as LC

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COLS = ['tid', 'qid', 'tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand']   # test_gpu_pack.py
KNOBS = ('MIMEO_PACK', 'MIMEO_MIRROR', 'MIMEO_BATCH_UNITS', 'MIMEO_K6_BMAX', 'MIMEO_INDEX_BUDGET_MB', 'MIMEO_PACK_MIN')
ERR_LIMIT = -5
F = set(LC.F)


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope='module')
def genomes(eng):
    """{nscaf: (engine genome, sequences)}: the six-scaffold genome is the head of the nine-scaffold one"""
    out = {}
    for n in (6, 9):
        names, seqs = LC.genome(n)
        out[n] = (eng.Genome(names, seqs), seqs)
    yield out
    for g, _ in out.values():
        g.close()


@pytest.fixture(scope='module')
def oracle(genomes):
    """{(t, q): the uncapped oracle's records, tid / qid filled in} of all 81 pairs, computed once"""
    rows = LC.oracle_rows(genomes[9][1], all_pairs(9))
    out = {}
    for (t, q), r in rows.items():
        r = r.copy()
        r['tid'], r['qid'] = t, q
        out[(t, q)] = r
    return out


@pytest.fixture(autouse=True)
def pool_cap(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv('MIMEO_K6_TRACE_POOL_MB', '1')
    yield
    monkeypatch.delenv('MIMEO_K6_TRACE_POOL_MB', raising=False)


def _cost(seqs):   # workflow.align_blocks
    return {t: int(s.size) * sum(int(x.size) for x in seqs) for t, s in enumerate(seqs)}


def all_pairs(n):
    return [(t, q) for t in range(n) for q in range(n)]


def _rows(recs, first, blocks):   # test_gpu_paths.py
    return sorted(recs[i].tobytes() + blocks[int(first[i]):int(first[i + 1])].tobytes() for i in range(recs.size))


def _failed(eng, entries):
    """the scaffold pairs named by failed_pairs(), and the entry indexes (each at most once, all with MIMEO_ERR_LIMIT)"""
    fp = eng.failed_pairs()
    idx = [i for i, _ in fp]
    assert all(code == ERR_LIMIT for _, code in fp) and len(set(idx)) == len(idx), fp
    return {(int(entries[i][0]), int(entries[i][1])) for i in idx}, sorted(idx)


def _table(recs):
    m = np.stack([np.asarray(recs[c], dtype=np.int64) for c in COLS], axis=1) if recs.size else np.zeros((0, len(COLS)), np.int64)
    return m[np.lexsort(m.T[::-1])].tolist()


def _check_paths(recs, first, blocks):
    assert first.size == recs.size + 1 and int(first[0]) == 0 and int(first[-1]) == blocks.size
    s = np.concatenate([np.zeros(1, np.int64), np.cumsum(blocks['len'].astype(np.int64))])
    f = first.astype(np.int64)
    assert (np.diff(f) >= 1).all() and (s[f[1:]] - s[f[:-1]] == recs['id_d']).all()   # every record's blocks sum to its id_d


def _check_survivors(recs, pairs, oracle):
    """pairs of F have no rows; every other pair equals the oracle (all of them, so also every pair that shares a scaffold
    with a pair of F)"""
    shared = 0
    for pr in pairs:
        got = recs[(recs['tid'] == pr[0]) & (recs['qid'] == pr[1])]
        if pr in F:
            assert got.size == 0, (pr, got)
            continue
        assert _table(got) == _table(oracle[pr]), pr
        shared += LC.shares_a_scaffold_with_F(*pr)
    assert shared >= 30


_default = {}


def default_run(eng, genomes, n):
    """the single align_pairs call over all pairs with paths, default layout, under the cap: run once per genome"""
    if n not in _default:
        g, _ = genomes[n]
        recs, first, blocks = eng.align_pairs(g, None, all_pairs(n), paths=True)
        _default[n] = (recs, first, blocks, _failed(eng, all_pairs(n))[0], eng.stats(), eng.last_error())
    return _default[n]


@pytest.mark.parametrize('n', [9, 6], ids=['packed', 'per_pair'])
def test_failed_set_and_survivors(eng, genomes, oracle, n):
    recs, first, blocks, failed, st, err = default_run(eng, genomes, n)
    assert (st['super_units'] > 0) == (n == 9), st
    assert failed == F
    if n == 6:   # the strand that does not fail has rows in the uncapped oracle: an empty pair shows the whole pair went
        assert (oracle[(0, 3)]['qstrand'] == LC.PLUS).any() and (oracle[(1, 4)]['qstrand'] == LC.MINUS).any()
    _check_survivors(recs, all_pairs(n), oracle)
    _check_paths(recs, first, blocks)
    assert re.search(r'strand [+-]:', err) and 'left out' in err, err


def test_layouts(eng, genomes, monkeypatch):
    recs, first, blocks, failed, _, _ = default_run(eng, genomes, 9)
    ref = _rows(recs, first, blocks)
    g, _ = genomes[9]
    for env in ({'MIMEO_PACK': '0'}, {'MIMEO_MIRROR': '0'}, {'MIMEO_BATCH_UNITS': '1'}, {'MIMEO_K6_BMAX': '1'}):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        alt = eng.align_pairs(g, None, all_pairs(9), paths=True)
        assert _failed(eng, all_pairs(9))[0] == F, env
        assert (eng.stats()['super_units'] > 0) == ('MIMEO_PACK' not in env), env
        assert _rows(*alt) == ref, env
        for k in env:
            monkeypatch.delenv(k)


def test_strand_split_entries(eng, genomes):
    """dist.units_of_row hands (t, q, MINUS) and (q, t, PLUS) of a pair to different entries: both go when one fails"""
    recs, first, blocks, _, _, _ = default_run(eng, genomes, 6)
    g, seqs = genomes[6]
    units = deal_units(6, _cost(seqs), 1, 0)
    got = eng.align_units(g, None, units, paths=True)
    assert eng.stats()['super_units'] == 0
    failed, idx = _failed(eng, units)
    assert failed == F
    assert idx == [k for k, u in enumerate(units) if (u[0], u[1]) in F]   # every entry naming a pair of F, once
    named = [units[k] for k in idx]
    # (1, 4) fails on the plus strand, which row 4 owns, and its minus strand is an entry of row 1; (3, 0) the other way round
    assert sorted(named) == sorted([(0, 3, BOTH), (3, 0, PLUS), (3, 0, MINUS), (1, 4, MINUS), (1, 4, PLUS), (4, 1, BOTH), (5, 5, BOTH)])
    assert _rows(*got) == _rows(recs, first, blocks)
    _check_paths(*got)
    assert not np.isin(got[0]['tid'].astype(np.int64) << 32 | got[0]['qid'].astype(np.int64), [t << 32 | q for t, q in F]).any()


@pytest.mark.parametrize('pack', [True, False], ids=['packed', 'per_pair'])
def test_duplicates(eng, genomes, monkeypatch, pack):
    recs, first, blocks, _, _, _ = default_run(eng, genomes, 9)
    g, _ = genomes[9]
    if not pack:
        monkeypatch.setenv('MIMEO_PACK', '0')
    pairs = all_pairs(9) + [(0, 3), (2, 4), (0, 3)]
    twice = eng.align_pairs(g, None, pairs, paths=True)
    assert (eng.stats()['super_units'] > 0) == pack
    failed, idx = _failed(eng, pairs)
    assert failed == F
    assert idx == sorted([k for k, pr in enumerate(all_pairs(9)) if pr in F] + [81, 83])   # all three (0, 3), once each
    dup = np.flatnonzero((recs['tid'] == 2) & (recs['qid'] == 4))
    assert dup.size >= 2
    assert twice[0].tobytes() == recs.tobytes() + recs[dup].tobytes()   # (2, 4) answered twice, nothing for the three (0, 3)
    assert _rows(*twice) == sorted(_rows(recs, first, blocks) + _rows(recs[dup], *formats.select_paths(first, blocks, dup)))
    _check_paths(*twice)


def _merge(eng, g, shares, fn):
    """each rank's share through the engine, then what a job does after its gather (workflow.drop_failed_pairs)"""
    parts, failed = [], set()
    for share in shares:
        assert share
        parts.append(fn(g, None, share, paths=True))
        failed |= _failed(eng, share)[0]
    recs = np.concatenate([p[0] for p in parts])
    cnt = np.concatenate([np.diff(p[1].astype(np.int64)) for p in parts])
    first = np.zeros(recs.size + 1, dtype=np.uint64)
    first[1:] = np.cumsum(cnt)
    a, f, b, union = workflow.drop_failed_pairs(Dist(), recs, first, np.concatenate([p[2] for p in parts]), sorted(failed))
    return a, f, b, set(union)


@pytest.mark.parametrize('world', [2, 3])
def test_ranks_in_process(eng, genomes, world):
    for n in (6, 9):
        recs, first, blocks, _, _, _ = default_run(eng, genomes, n)
        g, seqs = genomes[n]
        cost = _cost(seqs)
        if n == 6:
            shares, fn = [deal_units(n, cost, world, r) for r in range(world)], eng.align_units
        else:
            shares, fn = [shard_pairs_by_target(all_pairs(n), cost, world, r) for r in range(world)], eng.align_pairs
        a, f, b, union = _merge(eng, g, shares, fn)
        assert union == F, (n, world)
        assert _rows(a, f, b) == _rows(recs, first, blocks), (n, world)
        _check_paths(a, f, b)


def test_path_rule_without_paths(eng, genomes):
    """the path anchor rule traces every half it extends: the designed halves are the same ones"""
    g, _ = genomes[6]
    recs = eng.align_pairs(g, None, all_pairs(6), eng.default_params(anchor_rule=1))
    assert _failed(eng, all_pairs(6))[0] == F
    key = set(zip(recs['tid'].tolist(), recs['qid'].tolist()))
    assert not (key & F) and len(key) == 36 - len(F)
    assert re.search(r'strand [+-]:', eng.last_error())


def test_nothing_asked_nothing_lost(eng, genomes, oracle):
    """box rule, no paths, the same cap: no traceback, no failure, and nothing is left of the failures of the call before"""
    g, _ = genomes[6]
    eng.align_pairs(g, None, all_pairs(6), paths=True)
    assert _failed(eng, all_pairs(6))[0] == F
    recs = eng.align_pairs(g, None, all_pairs(6))
    assert eng.failed_pairs() == []
    for pr in all_pairs(6):   # the designed pairs with their long alignments
        assert _table(recs[(recs['tid'] == pr[0]) & (recs['qid'] == pr[1])]) == _table(oracle[pr]), pr
    for pr, strand in LC.F.items():
        r = recs[(recs['tid'] == pr[0]) & (recs['qid'] == pr[1]) & (recs['qstrand'] == strand)]
        assert int((r['tend'] - r['tstart']).max()) >= 0.9 * LC.LONG_BP, pr
    plain = eng.align_units(g, None, [(t, q, BOTH) for t, q in all_pairs(6)])
    assert eng.failed_pairs() == [] and plain.tobytes() == recs.tobytes()


def test_cli_self_one_process_and_two_ranks_leave_out_the_same_pairs(tmp_path):
    """`mimeo self --paf` on the six-scaffold FASTA, the cap in the child's environment: two gloo ranks on GPU 0 are dealt
    units (dist.deal_units: the strands of a pair on different ranks) and write the TAB, GFF3 and PAF of one process; no row
    names a pair of F; each run warns of every pair of F once, by its names."""
    names, seqs = LC.genome(6)
    fa = str(tmp_path / 'six.fa')
    write_fasta(fa, names, seqs)
    env1 = {k: v for k, v in os.environ.items() if k not in KNOBS}
    env1['MIMEO_K6_TRACE_POOL_MB'] = '1'

    def args(tag):
        return ['self', '--afasta', fa, '--minLen', '100', '--minCov', '3', '--paf', str(tmp_path / (tag + '.paf')), '-d', str(tmp_path / tag)]
    one = subprocess.run([sys.executable, '-m', 'mimeo_amd'] + args('one'), cwd=ROOT, capture_output=True, text=True, timeout=600, env=env1)
    assert one.returncode == 0, one.stdout + one.stderr
    s = socket.socket(); s.bind(('127.0.0.1', 0)); port = s.getsockname()[1]; s.close()
    env2 = dict(env1, MIMEO_DIST_BACKEND='gloo', MIMEO_FORCE_DEVICE='0')
    two = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
                          '--master-port', str(port), '-m', 'mimeo_amd'] + args('two'), cwd=ROOT, capture_output=True, text=True, timeout=900, env=env2)
    assert two.returncode == 0, two.stdout[-2000:] + two.stderr[-3000:]
    for run in (one, two):
        for t, q in sorted(F):
            assert run.stderr.count('Alignment of %s onto %s hit an engine limit' % (names[q], names[t])) == 1, ((t, q), run.stderr[-3000:])
        assert run.stderr.count('hit an engine limit') == len(F), run.stderr[-3000:]
    for f in ('one/mimeo_alignment.tab', 'one/mimeo-self_repeats.gff3', 'one.paf'):
        a, b = (tmp_path / f).read_text(), (tmp_path / f.replace('one', 'two')).read_text()
        assert a == b, f
    tab = [l.split('\t') for l in (tmp_path / 'one' / 'mimeo_alignment.tab').read_text().splitlines()[1:]]
    idx = {n: i for i, n in enumerate(names)}
    seen = {(idx[r[0]], idx[r[4]]) for r in tab}
    assert len(tab) > 30 and not (seen & F) and len(seen) == 36 - len(F)
    assert (tmp_path / 'one.paf').read_text().count('\n') == len(tab)
