"""The designed halves of tests/k6_strip_cases.py, on the CPU: every case reaches the event of k6_dp1's narrow first pass that it was
built for, and the prediction at 14 columns per lane is tests/k6_cases.route on all of k6_cases' own cases.

tests/test_gpu_k6_strips.py holds the engine to the oracle and to the prediction on these cases; that pins the widening and the
restart only if the cases really fill the narrow window to its last strips, reach the last strip but one gradually, right after a
slide and in row 1, jump over it, outgrow the window in row 0, with the query's end inside the window and with strips entering on
the right, before and after the change of width.  Those are conditions on the inputs, proven here with the band walk."""
import collections

import pytest

from tests import k6_cases as K
from tests import k6_strip_cases as KS

_cache = {}


def strip_cases():
    if 'cases' not in _cache:
        cases = KS.cases()
        K.prepare([c.case for c in cases])
        _cache['cases'] = cases
    return _cache['cases']


def test_every_case_reaches_its_event(capsys):
    cases = strip_cases()
    assert len({c.name for c in cases}) == len(cases)
    seen = collections.Counter()
    for c in cases:
        c.check()
        for want, (w, p) in zip(c.want, c.analyse()):
            if want is not None:
                seen[want['event'], p['kernel']] += 1
    with capsys.disabled():
        print('\n[k6 strips] %d cases, designed halves by (event at %d columns per lane, finishing kernel): %s' % (len(cases), KS.W1, dict(seen)))


def test_the_families_cover_the_edges_of_the_narrow_window():
    """the last live strip 59, 60 and 61 without an event; a widening late in the half, after a slide, and in row 1; the window
    outgrown in one row and in row 0; restarted halves that the pass at 14 finishes and that it loses to the 2048-column kernel; the
    main events on both sides of the anchor; EDGE and plain rows and fresh strips at either width"""
    by = collections.defaultdict(set)
    for c in strip_cases():
        for side, (want, (w, p)) in enumerate(zip(c.want, c.analyse())):
            if want is None:
                continue
            by[want['event'], want.get('widest'), want['kernel']].add(side)
            if want['event'] == 'widen':
                by['slid' if want.get('slid') else 'row1' if p['first']['event'][1] == 1 else 'late'].add(side)
            for k in ('edge', 'plain', 'fresh', 'edge2', 'plain2', 'fresh2'):
                if want.get(k):
                    by[k, want['event']].add(side)
    for widest in (59, 60, 61):
        assert by['fit', widest, 'lean'], widest
    for key in (('widen', None, 'lean'), ('jump', None, 'lean'), ('row0', None, 'lean'), ('row0', None, 'wide'), 'late', 'row1'):
        assert by[key] == {0, 1}, key
    assert by['slid']
    for k in ('edge', 'plain', 'fresh'):
        assert by[k, 'fit'] and by[k, 'widen'] and by[k + '2', 'widen'], k
        assert by[k + '2', 'jump'] or by[k + '2', 'row0'], k


def test_what_leaves_the_narrow_pass_is_what_it_says():
    """no designed half hides a second reason: the narrow pass finishes, hands over or gives up for the window, and a half that
    restarts is finished by the pass at 14 or leaves it for the band alone"""
    for c in strip_cases():
        for w, p in c.analyse():
            if p['first'] is None:
                continue
            ev = p['first']['event']
            assert ev is None or ev[0] in KS.RESTARTS + ('widen',), (c.name, ev)
            assert p['restarted'] + p['widened'] == (ev is not None), c.name
            if p['restarted']:
                assert p['kernel'] == 'lean' or p['lean'][0] in ('band', 'row0'), (c.name, p)


@pytest.mark.parametrize('name', sorted(K.FAMILIES))
def test_the_prediction_at_14_columns_is_the_route(name):
    """predict(.., w1=14) adds nothing to k6_cases.route, and strip_pass at 14 is route's lean kernel, on every case of k6_cases"""
    for c in K.prepare(K.FAMILIES[name]()):
        O, E, Y = c.oey
        _, hs = c.analyse()
        for w, r in hs:
            sc = r['kernel'] == 'shortcut'
            p = KS.predict(w, O, E, Y, c.cap or K.CAP, shortcut=sc, w1=KS.FULL)
            assert {k: p[k] for k in r} == r and p['first'] is None and not p['restarted'] and not p['widened'], c.name
            if sc or r['lean'] == ('penalties', 0, 0):
                continue
            first = KS.strip_pass(w, KS.FULL)
            if r['lean'] is None:
                assert first['event'] is None and first['maxcols'] == r['maxcols'] and first['fresh'] == r['fresh'], (c.name, first, r)
            else:
                assert first['event'] == (r['lean'][0], r['lean'][1]), (c.name, first, r)
