"""Every tail kernel of the gap-free stage in one small batch, under the three paths a record can take (k4_queue.h: the staged
appends, the shard map, the claim; k4_extend.hip).

One scaffold of 70 000 bases aligned to itself, both strands: six microsatellite arrays (followers, runs, walks that outlive the
frame), four copies of a 3 kbp family at about 2 % substitutions (walks beyond LONG_WINDOWS windows, large segments) and, on the
plus strand, the main diagonal of 70 000 columns — more than ENT_LONG = 65 536, so k4_diag0 and the two k4_entropy_big kernels
have work.  The engine must equal the oracle exactly under the default path, when the queues overflow and the batch is repeated
(MIMEO_QUEUE_SHRINK) and under the other decomposition of the heavy phase (MIMEO_HEAVY=v1), and the three must agree byte for
byte."""
import re

import numpy as np
import pytest
from numpy.lib.recfunctions import repack_fields

from tests.test_gpu_runs import ACGT, HCOLS, _arrays

pytestmark = pytest.mark.gpu

N = 70_000
ENT_LONG = 1 << 16
SEED = 376   # all of the below hold: checked on the CPU (first test) and printed on the GPU
MOTIFS = [[0], [3], [1, 0], [3, 2], [0, 1, 2], [1, 2, 3]]   # with their reverse complements: the minus strand has rectangles too
FAMILY = 3000
COPIES = (4_000, 21_000, 39_000, 57_000)
ENV = ('MIMEO_HEAVY', 'MIMEO_K4_VARIANT', 'MIMEO_QUEUE_SHRINK', 'MIMEO_K4_STATS', 'MIMEO_K34_DEBUG')
PATHS = {'default': {}, 'rerun': {'MIMEO_QUEUE_SHRINK': '4000'}, 'v1': {'MIMEO_HEAVY': 'v1'}}
_cache = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def scaffold():
    """the scaffold, where its arrays lie, and how many bases the family copies differ in"""
    if 'scaffold' not in _cache:
        rng = np.random.default_rng(SEED)
        s, where = _arrays(rng, N, MOTIFS, 6, 0.0)
        fam = rng.integers(0, 4, size=FAMILY, dtype=np.uint8)
        subs = []
        for p in COPIES:
            c = fam.copy()
            k = rng.random(FAMILY) < 0.02
            c[k] = (c[k] + rng.integers(1, 4, size=int(k.sum()), dtype=np.uint8)) & 3
            s[p:p + FAMILY] = c
            subs.append(int(k.sum()))
        _cache['scaffold'] = (ACGT[s], where, subs)
    return _cache['scaffold']


def _bytes(a):
    """the compared columns alone, packed"""
    return repack_fields(a).tobytes()


def expected(strand):
    """the oracle's HSPs of a strand, sorted; computed once"""
    if ('exp', strand) not in _cache:
        from oracle import oracle as O
        seq = scaffold()[0].tobytes()
        _cache['exp', strand] = np.sort(O.ungapped_hsps(seq, seq, strand, O.default_params(chain=0))[HCOLS], order=HCOLS)
    return _cache['exp', strand]


def run(eng, monkeypatch, capfd, path):
    """both strands under one path, once: sorted HSPs per strand, seed hits, reruns, the counts of the last [k4] line"""
    if ('run', path) not in _cache:
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in dict(PATHS[path], MIMEO_K4_STATS='1').items():
            monkeypatch.setenv(k, v)
        g = eng.Genome(['s'], [scaffold()[0]])
        out = {'hsps': [], 'seed_hits': [], 'reruns': 0, 'counts': []}
        for strand in (0, 1):
            capfd.readouterr()
            got = eng.ungapped_hsps(g, 0, g, 0, strand, eng.default_params(chain=0))
            st = eng.stats()
            err = capfd.readouterr().err
            lines = re.findall(r'\[k4\] units \d+ walk queue \d+ walked \d+ generic (\d+) long (\d+) followers (\d+) candidates (\d+)', err)
            assert lines, err
            out['hsps'].append(np.sort(got[HCOLS], order=HCOLS))
            out['seed_hits'].append(st['seed_hits'])
            out['reruns'] += st['queue_reruns']
            out['counts'].append(tuple(int(x) for x in lines[-1]))
        g.close()
        for k in ENV:
            monkeypatch.delenv(k, raising=False)
        _cache['run', path] = out
    return _cache['run', path]


def test_the_input_is_what_the_tails_need():
    """on the CPU: the arrays are 200-500 bp and clear of the family copies, the copies differ by about 2 %, and the oracle's plus
    strand holds the main diagonal in one piece"""
    seq, where, subs = scaffold()
    assert seq.size == N and len(where) == 6
    for p, ln in where:
        assert 200 <= ln <= 500, (p, ln)
        assert all(p + ln <= c or c + FAMILY <= p for c in COPIES), (p, ln)
    assert all(0.01 * FAMILY < k < 0.03 * FAMILY for k in subs), subs
    exp = expected(0)
    diag = exp[(exp['tstart'] == 0) & (exp['qstart'] == 0)]
    assert diag.size == 1 and int(diag['length'][0]) == N and N > ENT_LONG, diag
    # the family: every copy against every other, on the plus strand
    fam = exp[(exp['length'] > FAMILY // 2) & (exp['tstart'] != exp['qstart'])]
    assert fam.size >= 12, fam


@pytest.mark.parametrize('path', list(PATHS))
def test_the_engine_equals_the_oracle(eng, monkeypatch, capfd, path):
    r = run(eng, monkeypatch, capfd, path)
    print(path, 'reruns', r['reruns'], 'seed hits', r['seed_hits'], '(generic, long, followers, candidates) per strand', r['counts'])
    for strand in (0, 1):
        a, b = r['hsps'][strand], expected(strand)
        assert a.size == b.size and (a == b).all(), (path, strand, a.size, b.size)
        # every tail kernel had work: walks beyond the frame, beyond LONG_WINDOWS windows, followers to sort and resolve, candidates
        assert all(n > 0 for n in r['counts'][strand]), (path, strand, r['counts'])
    assert (r['reruns'] >= 1) == (path == 'rerun'), (path, r['reruns'])


def test_the_three_paths_agree(eng, monkeypatch, capfd):
    base = run(eng, monkeypatch, capfd, 'default')
    for path in ('rerun', 'v1'):
        r = run(eng, monkeypatch, capfd, path)
        assert r['seed_hits'] == base['seed_hits'], (path, r['seed_hits'], base['seed_hits'])
        for strand in (0, 1):
            assert _bytes(r['hsps'][strand]) == _bytes(base['hsps'][strand]), (path, strand)
