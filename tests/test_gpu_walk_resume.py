"""The hand-over of a walk from the walk kernel to k4_extend_generic, on the designed diagonals of tests/walk_resume_cases.py
(what they cover is asserted on the CPU: tests/test_host_walk_resume.py).  The engine must equal the oracle, exactly: under the
default path, under MIMEO_HEAVY=v1 with the full-plane variant, and when the queues overflow and the batch is repeated — the
record that carries the walk's state goes through every one of them."""
import re

import numpy as np
import pytest

from tests import gapfree_cases as G
from tests import oracle_pool
from tests import walk_resume_cases as W

pytestmark = pytest.mark.gpu

COLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
ENV = ('MIMEO_HEAVY', 'MIMEO_K4_VARIANT', 'MIMEO_QUEUE_SHRINK', 'MIMEO_PACK', 'MIMEO_K4_STATS')
PATHS = (('k34', {}), ('v1_full_planes', {'MIMEO_HEAVY': 'v1', 'MIMEO_K4_VARIANT': '5'}), ('rerun', {'MIMEO_QUEUE_SHRINK': '4000'}))
_cache = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def pairs():
    if 'pairs' not in _cache:
        _cache['pairs'] = W.pairs()
    return _cache['pairs']


def expected(name, minus):
    """the oracle's HSPs of a pair and strand, computed once"""
    if (name, minus) not in _cache:
        from oracle import oracle as O
        pair = pairs()[name]
        q, strand = G.query(pair, {'minus': minus})
        _cache[name, minus] = O.ungapped_hsps(pair.T, q, strand, O.default_params(chain=0))
    return _cache[name, minus]


def _set(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cmp(got, exp, tag):
    a = np.sort(got[COLS], order=COLS)
    b = np.sort(exp[COLS], order=COLS)
    sa, sb = set(map(tuple, a.tolist())), set(map(tuple, b.tolist()))
    assert a.size == b.size and sa == sb, (tag, a.size, b.size, 'engine only', sorted(sa - sb)[:3], 'oracle only', sorted(sb - sa)[:3])


def _generic(err):
    """the generic-walk hits of every batch, from the MIMEO_K4_STATS lines"""
    return [int(m) for m in re.findall(r'\[k4\] units \d+ walk queue \d+ walked \d+ generic (\d+)', err)]


@pytest.mark.parametrize('minus', [0, 1])
@pytest.mark.parametrize('path,name', [(p[0], n) for p in PATHS for n in ('R', 'RN') if (p[0], n) != ('rerun', 'RN')])   # (four cases overflow nothing)
def test_resumed_walks_equal_the_oracle(eng, monkeypatch, capfd, path, name, minus):
    pair = pairs()[name]
    q, strand = G.query(pair, {'minus': minus})
    g = eng.Genome(['t', 'q'], [pair.T, q])
    _set(monkeypatch, dict(dict(PATHS)[path], MIMEO_K4_STATS='1'))
    capfd.readouterr()
    got = eng.ungapped_hsps(g, 0, g, 1, strand, eng.default_params(chain=0))
    reruns = eng.stats()['queue_reruns']
    err = capfd.readouterr().err
    _set(monkeypatch, {})
    g.close()
    generic = _generic(err)
    print(path, name, minus, 'generic-walk hits per batch', generic, 'reruns', reruns)
    # without walks that outlive the frame the comparison proves nothing about the hand-over
    assert generic and generic[-1] > 0, err
    assert (reruns >= 1) == (path == 'rerun'), (path, reruns)
    _cmp(got, expected(name, minus), (path, name, minus))


def test_one_batched_call_over_the_cut_out_cases(eng, monkeypatch, capfd):
    """every case of the pair without N as a scaffold pair of its own, flush with both ends, in one align_pairs call without the
    gapped stage: walks that run out of sequence after exactly 64 and 65 steps exist only here"""
    from oracle import oracle as O
    O.lib()
    cuts = pairs()['R'].cutouts()
    n = len(cuts)
    prm = dict(gapped=0, hspthresh=1500)
    pending = oracle_pool.start([(lambda t, q: O.align_pair(t, q, O.default_params(**prm)), t.tobytes(), q.tobytes()) for t, q in cuts], cap=16)
    g = eng.Genome(['t%d' % i for i in range(n)] + ['q%d' % i for i in range(n)], [t for t, _ in cuts] + [q for _, q in cuts])
    _set(monkeypatch, {'MIMEO_K4_STATS': '1'})
    capfd.readouterr()
    got = eng.align_pairs(g, None, [(i, n + i) for i in range(n)], eng.default_params(**prm))
    err = capfd.readouterr().err
    _set(monkeypatch, {})
    exp = pending.results()
    g.close()
    generic = _generic(err)
    print('batched', 'generic-walk hits per batch', generic)
    assert sum(generic) > 0, err
    rows = 0
    for i, e in enumerate(exp):
        a = np.sort(got[(got['tid'] == i) & (got['qid'] == n + i)][oracle_pool.ACOLS], order=oracle_pool.ACOLS)
        b = np.sort(e[oracle_pool.ACOLS], order=oracle_pool.ACOLS)
        assert a.size == b.size and (a == b).all(), (i, a, b)
        rows += a.size
    assert rows >= n
