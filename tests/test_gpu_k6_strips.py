"""k6_dp1's two strip widths on DESIGNED halves (tests/k6_strip_cases.py): halves that fill the narrow first window to its last
strips, reach the last strip but one late, after a slide and in row 1 (the state moves to the full width), jump over it or outgrow the
window in row 0 (the half runs again), with the query's end inside the window and strips entering on the right at either width, on
both sides of the anchor.  That the cases reach those events is asserted on the CPU
(tests/test_host_k6_strips.py).  Here the engine must equal the oracle on every case, report per half what the prediction says
(MIMEO_K6_STATS: rows, the band of the 14-column layout, the best cell), and widen and restart exactly the predicted halves."""
import numpy as np
import pytest

from tests import k6_cases as K
from tests import k6_strip_cases as KS
from tests import oracle_pool

pytestmark = pytest.mark.gpu

COLS = oracle_pool.ACOLS
ENV = ('MIMEO_K6_SCORE_CAP', 'MIMEO_K6_BMAX', 'MIMEO_K6_STATS')
NPARTS = 4
_cache = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def part(k):
    if 'cases' not in _cache:
        _cache['cases'] = KS.cases()
    return _cache['cases'][k::NPARTS]


def _stats(err):
    """of the first round of a call's MIMEO_K6_STATS output: the line of the full strip width (restarted, widened) and the per-job lines"""
    lines = err.splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith('[k6] jobs'))
    assert lines[k - 1].startswith('[k6] full strip width: restarted '), lines[k - 1]
    f = lines[k - 1].split()
    restarted, widened, jobs = int(f[5]), int(f[7]), int(f[9])
    assert jobs == int(lines[k].split('jobs ')[1].split()[0])
    job = {}
    for l in lines[k + 2:k + 2 + jobs]:
        assert l.startswith('  [k6] job '), l
        f = l.split(':')[1].split()
        job[int(f[1])] = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
    return (restarted, widened), job


@pytest.mark.parametrize('k', range(NPARTS))
def test_designed_halves_equal_the_oracle_and_change_width_as_predicted(eng, monkeypatch, capfd, k):
    """one anchor per round with statistics: the first round's two jobs are the halves of the top anchor"""
    from oracle import oracle as O
    O.lib()
    cases = part(k)
    pending = oracle_pool.start([(lambda c: O.align_pair(c.T, c.Q, O.default_params(**c.oracle_kw())), s.case) for s in cases], cap=16)
    K.prepare([s.case for s in cases], threads=16)
    got, seen = {}, {}
    for s in cases:
        c = s.case
        for e in ENV:
            monkeypatch.delenv(e, raising=False)
        monkeypatch.setenv('MIMEO_K6_BMAX', '1')
        monkeypatch.setenv('MIMEO_K6_STATS', '1')
        g = eng.Genome(['t', 'q'], [c.T, c.Q])
        capfd.readouterr()
        got[s.name] = eng.align_pair(g, 0, g, 1, eng.default_params(strand=2 if c.minus else 1, **c.params))
        seen[s.name] = _stats(capfd.readouterr().err)
        assert not eng.failed_pairs(), s.name
        g.close()
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    for s, exp in zip(cases, pending.results()):
        a, b = got[s.name][COLS], exp[COLS]
        assert exp.size >= 1 and a.size == b.size, (s.name, a.size, b.size)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (s.name, a[bad[:3]], b[bad[:3]])
        counts, job = seen[s.name]
        hs = s.analyse()
        assert counts == (sum(p['restarted'] for _, p in hs), sum(p['widened'] for _, p in hs)), (s.name, counts, [p['first'] for _, p in hs])
        for (w, p), direction in zip(hs, (-1, 1)):
            want = dict(rows=p['rows'], maxcols=p['maxcols'], i=w.best[1], j=w.best[2], rebased=int(p['rebases'] > 0))
            assert job[direction] == want, (s.name, direction, p['kernel'], job[direction], want)
