"""K6's take per group and round on seeded pairs (tests/k6_round_cases.py): more copies than the old cap of 32 anchors and than the
new limit, one long collinear copy (the guard), a chain longer than the 512 ranks k6_pick used to look at, a near pair that is not
swallowed.  One scaffold pair and the plus strand per case, so one group.  Records must equal the oracle's under every take;
the rounds and the DP jobs that MIMEO_K6_STATS reports (`[k6] jobs` lines on stderr) must be those of the CPU model of k6_pick /
k6_resolve, which tests/test_host_k6_rounds.py holds to hand-worked groups."""
import numpy as np
import pytest

from tests import k6_round_cases as R
from tests import oracle_pool

pytestmark = pytest.mark.gpu

COLS = oracle_pool.ACOLS
ENV = ('MIMEO_K6_BMAX', 'MIMEO_K6_STATS')
SIZES = (R.OLD_CAP + 1, 40, R.LIMIT + 1)
_cache = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


COLLINEAR = {'collinear': 150000, 'collinear-long': 450000}


def pair(name):
    """(T, Q, the oracle's plus-strand records, the ranked anchors), made once; the two oracle calls side by side"""
    if name not in _cache:
        if isinstance(name, int):
            T, Q, _ = R.distinct_pairs(name, seed=2700 + name)
        elif name in COLLINEAR:
            T, Q = R.collinear_pair(COLLINEAR[name], seed=27)
        elif name == 'fragmented':
            T, Q = R.fragmented_pairs(30, 12, seed=279)
        else:
            T, Q = R.near_miss_pair(seed=271)
        exp, anchors = oracle_pool.run([(oracle_pool.align_unit, T, Q, 0), (R.ranked_anchors, T, Q)], cap=2)
        _cache[name] = (T, Q, exp, anchors)
    return _cache[name]


def run(eng, monkeypatch, capfd, T, Q, take=None):
    """the engine's plus-strand records at the take (None: the default) and the half extensions of every round that ran a DP"""
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    if take is not None:
        monkeypatch.setenv('MIMEO_K6_BMAX', str(take))
    monkeypatch.setenv('MIMEO_K6_STATS', '1')
    g = eng.Genome(['t', 'q'], [T, Q])
    capfd.readouterr()
    got = eng.align_pair(g, 0, g, 1, eng.default_params(strand=1))
    err = capfd.readouterr().err
    assert not eng.failed_pairs()
    g.close()
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    jobs = [int(l.split('jobs ')[1].split()[0]) for l in err.splitlines() if l.startswith('[k6] jobs')]
    print('take', take, 'rounds', len(jobs), 'jobs', jobs[:12], 'total', sum(jobs))
    return got, jobs


def same(got, exp, tag):
    a, b = oracle_pool._table(got), oracle_pool._table(exp)
    assert a.shape == b.shape, (tag, a.shape[0], b.shape[0])
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (tag, a[bad[:3]].tolist(), b[bad[:3]].tolist())


@pytest.mark.parametrize('n', SIZES)
def test_distinct_copies_one_round_up_to_the_limit(eng, monkeypatch, capfd, n):
    T, Q, exp, anchors = pair(n)
    assert exp.size == n                                       # every planted copy is one alignment
    for take in (None, 1, 4, 32):
        got, jobs = run(eng, monkeypatch, capfd, T, Q, take)
        same(got, exp, (n, take))
        model = R.predict(anchors, exp, R.default_take(1, take))
        assert jobs == model['jobs'], (n, take, jobs[:12], model['jobs'][:12])
        if take is None:
            assert len(jobs) == (1 if n <= R.LIMIT else 2), (n, jobs)
        if take == 32 and n == R.OLD_CAP + 1:
            assert len(jobs) == 2, jobs


@pytest.mark.parametrize('name', sorted(COLLINEAR))
def test_collinear_copy_costs_no_more_than_at_the_old_cap(eng, monkeypatch, capfd, name):
    """the guard: the far-apart HSPs of one long alignment beyond a round's first 32 wait, as they did when 32 was the cap.  At 150 kbp
    the near rule alone keeps the round below 32 anchors; at 450 kbp more than 32 HSPs lie further than NEAR_POS from each other, and
    without the guard the limit's take would run them all (the model says so before the engine is asked)"""
    T, Q, exp, anchors = pair(name)
    assert exp.size == 1 and len(anchors) > 40, (exp.size, len(anchors))
    if name == 'collinear-long':
        free, held = R.predict(anchors, exp, R.LIMIT, guard=False), R.predict(anchors, exp, R.LIMIT)
        assert sum(free['jobs']) > sum(held['jobs']) == 2 * R.GUARD_FREE, (free['jobs'], held['jobs'])
    got, jobs = run(eng, monkeypatch, capfd, T, Q)
    same(got, exp, 'default')
    got32, jobs32 = run(eng, monkeypatch, capfd, T, Q, 32)
    same(got32, exp, 32)
    assert sum(jobs) <= sum(jobs32), (jobs, jobs32)
    assert jobs == R.predict(anchors, exp, R.LIMIT)['jobs'] and jobs32 == R.predict(anchors, exp, 32)['jobs']


def test_chain_longer_than_the_old_scan_window_is_one_round(eng, monkeypatch, capfd):
    """30 copies in ~20 HSPs each and 12 short ones that rank beyond 512: k6_pick's window (PICK_SCAN) now holds the whole chain, as it
    holds the chains of a benchmark row (480 HSPs a group, up to 628).  At a window of 512 the model needs a second round"""
    T, Q, exp, anchors = pair('fragmented')
    assert exp.size == 42 and len(anchors) > 512
    model = R.predict(anchors, exp, R.LIMIT)
    assert max(model['accepted']) >= 512 and model['rounds'] == 1 and R.predict(anchors, exp, R.LIMIT, scan=512)['rounds'] == 2
    got, jobs = run(eng, monkeypatch, capfd, T, Q)
    same(got, exp, 'default')
    assert jobs == model['jobs'], (jobs, model['jobs'])
    got, jobs = run(eng, monkeypatch, capfd, T, Q, 32)
    same(got, exp, 32)
    assert jobs == R.predict(anchors, exp, 32)['jobs'], jobs


def test_near_pair_that_is_not_swallowed_takes_two_rounds(eng, monkeypatch, capfd):
    T, Q, exp, anchors = pair('near')
    assert exp.size == 2
    for take in (None, 1, 4, 32):
        got, jobs = run(eng, monkeypatch, capfd, T, Q, take)
        same(got, exp, take)
        assert len(jobs) == 2 and jobs == R.predict(anchors, exp, R.default_take(1, take))['jobs'], (take, jobs)
