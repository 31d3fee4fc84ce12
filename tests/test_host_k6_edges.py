"""The designed pairs of tests/k6_cases.py, on the CPU: the band walk is held to the oracle on every case, and what the families
reach in the DP cascade of K6 is ASSERTED from `route`.

tests/test_gpu_k6_edges.py holds the engine to the oracle on these cases.  That pins the hand-overs of the cascade only if the cases
really reach them: a half kept by one strip and lost by one strip in either register kernel, row 0 deciding through min(lenB, .),
every residue of lenB against the strip widths, 65 534 and 65 535 rows, slides of several strips, shortcuts whose last word is
partial, later cells that return to the best score.  Those are conditions on the inputs, proven here with a walk that shares no
code with the oracle or the engine.  A family that misses a condition is to be changed; the condition is not.

Run with -s for one line per family: cases, routes reached, widest band, largest slide."""
import collections

import numpy as np
import pytest

from oracle import oracle as O
from tests import k6_cases as K
from tests import oracle_pool
from tests import spec_v1 as S

FIVE = ('tstart', 'tend', 'qstart', 'qend', 'score')
_cache = {}


def family(name):
    """(cases, [(anchor, [(walk, route), (walk, route)])], the oracle's records) of a family, computed once"""
    if name not in _cache:
        cases = K.prepare(K.FAMILIES[name]())
        runs = {}                                          # the score cap is the engine's: one oracle run serves both
        for c in cases:
            runs.setdefault((c.T, c.Q, tuple(sorted(c.oracle_kw().items()))), c)
        pending = oracle_pool.start([(lambda c: O.align_pair(c.T, c.Q, O.default_params(**c.oracle_kw())), c) for c in runs.values()], cap=8)
        an = [c.analyse() for c in cases]
        res = dict(zip(runs, pending.results()))
        _cache[name] = (cases, an, [res[c.T, c.Q, tuple(sorted(c.oracle_kw().items()))] for c in cases])
    return _cache[name]


def halves_of(name):
    """(case, side 0 / 1, walk, route) of every half of a family"""
    cases, an, _ = family(name)
    return [(c, k, w, r) for c, (_, hs) in zip(cases, an) for k, (w, r) in enumerate(hs)]


def by_name(name, case_name):
    cases, an, _ = family(name)
    k = [c.name for c in cases].index(case_name)
    return cases[k], an[k]


# ------------------------------------------------------------------------------------------------ the walk against the oracle
@pytest.mark.parametrize('name', sorted(K.FAMILIES))
def test_the_walk_joined_at_the_anchor_is_the_oracles_first_alignment(name, capsys):
    cases, an, exp = family(name)
    assert len({c.name for c in cases}) == len(cases)
    for c, e in zip(cases, exp):
        assert e.size, c.name
        assert tuple(int(e[0][k]) for k in FIVE) == c.expected(), c.name
    hs = halves_of(name)
    routes = collections.Counter(r['kernel'] for _, _, _, r in hs)
    why = collections.Counter((k, r[k][0]) for _, _, _, r in hs for k in ('lean', 'wide') if r[k])
    with capsys.disabled():
        print('\n[k6 cases] family %s: %d cases, halves finished %s, given up %s, widest band %d columns, widest k6_dp_any row %d, '
              'largest slide %d strips, most rebases %d'
              % (name, len(cases), dict(routes), {'%s %s' % k: v for k, v in sorted(why.items())}, max(r['maxcols'] for _, _, _, r in hs),
                 max(r['ncols'] for _, _, _, r in hs), max(r['slide'] for _, _, _, r in hs), max(r['rebases'] for _, _, _, r in hs)))


def test_family_t_equals_the_plain_python_restatement():
    """full matrices only fit there, and take 2 s a pair.  Every case but the two at y-drop 70 000, whose query of 3000 bases stays
    live from end to end: 10^6 cells of plain Python each, and the same Z, gap and tie as the two T-rowtie cases that do run"""
    cases, _, exp = family('T')
    for c, e in zip(cases, exp):
        if c.oey[2] != 9400:
            assert c.name in ('T-rowtie-r-any', 'T-rowtie-l-any')
            continue
        spec = S.align_strand(c.T.decode(), c.Q.decode(), c.minus)
        got = [tuple(int(r[k]) for k in ('tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand')) for r in e]
        assert got == spec, c.name


def test_the_c_walk_is_the_numpy_walk_row_by_row():
    """tests/k6_walk.c walks the long halves; here both walk every other case of families S (short pairs) and T, some of Q
    and I, and the W pair at two y-drops"""
    picked = [c for c in family('S')[0] if 'rows' not in c.name][::2] + family('T')[0][::2] + family('Q')[0][::25] + family('I')[0][::6]
    picked += [by_name('W', n)[0] for n in ('W-y9400', 'W-y18000')]
    n = 0
    for c in picked:
        at, aq = c.anchor()
        o, e, y = c.oey
        for A, B in K.halves(c.T, c.Qs, at, aq):
            if len(A) > 5000 or y > 100000 and len(A) * len(B) > 300000:
                continue
            a, b = K.walk(A, B, o, e, y), K.walk_c(A, B, o, e, y)
            assert a.best == b.best, c.name
            assert np.array_equal(a.lo, b.lo) and np.array_equal(a.hi, b.hi) and np.array_equal(a.bests, b.bests), c.name
            n += 1
    assert n > 25


# ------------------------------------------------------------------------------------------------ family W
def _w_grid(e=30):
    """(y-drop, route of the left half, route of the right half) of the W pair's grid at gap extension e, plus strand, production cap"""
    cases, an, _ = family('W')
    return sorted((c.oey[2], hs[0][1], hs[1][1]) for c, (_, hs) in zip(cases, an) if c.oey[1] == e and not c.minus and not c.cap)


@pytest.mark.parametrize('e', [30, 15, 60])
def test_w_grid_crosses_both_change_overs(e):
    """both halves: lean in the first rows of the grid, k6_dp_any in the last, each route once and in order; at gap extension 30 the
    grid's steps across every change-over are 100 at the most (the ride-alongs at 15 and 60 run either side of theirs)"""
    g = _w_grid(e)
    assert all(r['kernel'] == 'lean' for _, a, b in g[:2 if e == 30 else 1] for r in (a, b))
    assert all(r['kernel'] == 'any' for _, a, b in g[-2:] for r in (a, b))
    for side in (1, 2):
        ks = [x[side]['kernel'] for x in g]
        assert ks == sorted(ks, key=('lean', 'wide', 'any').index), (e, side, ks)
        for a, b in (('lean', 'wide'), ('wide', 'any')):
            k = ks.index(b)
            assert ks[k - 1] == a, (e, side)
            if e == 30:
                assert g[k][0] - g[k - 1][0] <= 100 and g[k - 1][0] - g[k - 2][0] <= 100 and g[k + 1][0] - g[k][0] <= 100, (side, g[k][0])


def test_w_halves_kept_and_lost_by_one_strip_and_row_0():
    hs = [r for _, _, _, r in halves_of('W') + halves_of('Q')]
    assert any(r['kernel'] == 'lean' and r['maxcols'] == 882 for r in hs)            # 63 strips: one short of the window
    assert any(r['kernel'] == 'wide' and r['maxcols'] == 2016 for r in hs)
    for k in ('lean', 'wide'):
        assert any(r[k] and r[k][0] == 'band' and r[k][1] > 1 and r[k][2] == 63 for r in hs), k    # the last strip, in a later row
        assert any(r[k] and r[k][0] == 'row0' for r in hs), k
    g = {y: (a, b) for y, a, b in _w_grid()}
    for y0, y1, k in ((26830, 26860, 'lean'), (60850, 60880, 'wide')):
        assert all(r[k] and r[k][0] == 'band' for r in g[y0]), (y0, g[y0])           # hi_0 = 881 / 2015: row 0 fits, a later row does not
        assert all(r[k] and r[k][0] == 'row0' for r in g[y1]), (y1, g[y1])


def test_w_under_the_low_cap_and_on_the_minus_strand():
    hs = halves_of('W')
    capped = [r for c, _, _, r in hs if c.cap]
    assert any(r['kernel'] == 'any' and r['wide'][0] == 'cap' and r['rebases'] > 0 for r in capped)
    assert any(r['kernel'] == 'lean' for r in capped)                                # the lean kernel knows no cap
    assert {r['kernel'] for c, _, _, r in hs if c.minus} == {'lean', 'wide', 'any'}


def test_k6_dp_any_rows_of_every_width_class():
    """ncols decides how many columns a thread of k6_dp_any takes: one (ncols <= 1024), two, more"""
    n = [r['ncols'] for name in K.FAMILIES for _, _, _, r in halves_of(name) if r['kernel'] == 'any']
    assert any(x <= 1024 for x in n) and any(1024 < x <= 2048 for x in n) and any(x > 2048 for x in n)


def test_every_kernel_finishes_many_halves():
    """what the GPU file's route check holds the engine to: each way through the cascade, in dozens of halves"""
    n = collections.Counter(r['kernel'] for name in K.FAMILIES for _, _, _, r in halves_of(name))
    assert min(n[k] for k in ('shortcut', 'lean', 'wide', 'any')) >= 15, n


# ------------------------------------------------------------------------------------------------ family Q
def _ending(c, hs):
    """the half of a Q / R-short / I case that runs into the designed sequence end: (walk, route)"""
    side = 0 if c.name.split('-')[1][0] == 'l' else 1
    return hs[side]


def test_q_every_residue_of_lenb_in_every_kernel():
    cases, an, _ = family('Q')
    seen = collections.defaultdict(set)
    for c, (_, hs) in zip(cases, an):
        w, r = _ending(c, hs)
        if c.name.startswith('Q-t'):
            continue
        assert w.lenB == int(c.name.split('-')[1][1:]), c.name                        # the anchor is where it was designed
        assert w.rows >= min(w.lenB, w.lenA) - 12, c.name                             # the homology runs to the query's end
        group = 'small' if w.lenB < 100 else '896' if w.lenB < 1000 else '2048'
        seen[group, r['kernel']].add(w.lenB)
    full = lambda s, m: {x % m for x in s} == set(range(m))
    assert full(seen['small', 'lean'], 14) and full(seen['small', 'lean'], 32) and len(seen['small', 'wide']) >= 8
    assert {15, 16, 31, 32, 33, 63, 64, 65} <= seen['small', 'lean'] and {15, 32, 63, 64, 65} <= seen['small', 'wide']
    assert full(seen['896', 'lean'], 14) and full(seen['896', 'wide'], 32) and full(seen['896', 'wide'], 14)
    assert full(seen['2048', 'any'], 32) and full(seen['2048', 'any'], 14) and len(seen['2048', 'wide']) >= 6 and len(seen['2048', 'lean']) >= 4
    # min(lenB, .) decides row 0: 880 and 881 columns stay, 882 go on; 2014 and 2015 stay, 2016 go on
    y = {c.name: _ending(c, hs)[1] for c, (_, hs) in zip(cases, an)}
    assert y['Q-r880']['kernel'] == y['Q-r881']['kernel'] == 'lean' and y['Q-r882']['lean'][0] == 'row0'
    assert y['Q-r2014']['kernel'] == y['Q-r2015']['kernel'] == 'wide' and y['Q-r2016']['wide'][0] == 'row0'
    assert y['Q-r2047']['ncols'] == 2048 and y['Q-r2048']['ncols'] == 2049
    ends = [(c, _ending(c, hs)[0]) for c, (_, hs) in zip(cases, an) if c.name.startswith('Q-t')]
    assert len(ends) >= 3 and all(w.lenA < w.lenB and w.rows == w.lenA for _, w in ends)   # the target ends first
    assert sum(c.minus for c in cases) >= 4


# ------------------------------------------------------------------------------------------------ family R
def test_r_row_counts_and_their_finishers():
    cases, an, _ = family('R')
    for c, (_, hs) in zip(cases, an):
        side, rows = c.name.split('-')[1][0], int(c.name.split('-')[1][1:])
        w, r = hs[0 if side == 'l' else 1]
        assert w.lenA == rows and w.rows == rows, c.name                            # alive in its last row
        if rows in K.R_LONG:
            want = 'lean' if rows < 65535 else 'any' if c.cap else 'wide'
            assert r['kernel'] == want, (c.name, r)
            if rows >= 65535:
                assert r['lean'] == ('rows', 65535, 0)
            if want == 'any':
                assert r['wide'][0] == 'cap' and r['ncols'] <= 1024 and r['rebases'] >= 20, (c.name, r)
        else:
            assert r['kernel'] == 'lean'
    for side in 'rl':
        rows = {int(c.name.split('-')[1][1:]) for c in cases if c.name.split('-')[1][0] == side}
        assert rows >= set(K.R_LONG) and {c.name for c in cases} >= {'R-%s%d-cap' % (side, n) for n in K.R_LONG}, side
    assert {int(c.name.split('-')[1][1:]) for c in cases} == set(K.R_LONG) | set(K.R_SHORT)


# ------------------------------------------------------------------------------------------------ family S
def test_s_slides_of_two_strips_in_both_register_kernels():
    hs = halves_of('S')
    assert any(r['kernel'] == 'lean' and r['slide'] >= 2 for _, _, _, r in hs)
    assert any(r['kernel'] == 'wide' and r['slide'] >= 2 and r['lean'][0] == 'rows' for _, _, _, r in hs)
    assert all(max(r['slide'] for r in (a[1], b[1])) >= 2 for _, (a, b) in family('S')[1])
    # strips that came in on the right (lane + shift >= 64) and held live cells: any half longer than the window
    every = [r for name in K.FAMILIES for _, _, _, r in halves_of(name)]
    assert any(r['kernel'] == 'lean' and r['fresh'] for r in every) and any(r['kernel'] == 'wide' and r['fresh'] for r in every)


# ------------------------------------------------------------------------------------------------ family I
def test_i_shortcuts_taken_and_defeated_as_designed():
    cases, an, _ = family('I')
    taken, defeated, control = set(), collections.Counter(), set()
    for c, (_, hs) in zip(cases, an):
        _, sn, change = c.name.split('-', 2)
        n = int(sn[1:])
        w, r = _ending(c, hs)
        if change in ('none', 'beyond'):
            assert r['kernel'] == 'shortcut' and min(w.lenA, w.lenB) == n and w.best[1:] == (n, n), c.name
            (taken if change == 'none' else control).add(n)
        else:
            assert r['kernel'] != 'shortcut', c.name
            if n > 33 or change == 'sub-first':
                assert min(w.lenA, w.lenB) == n, c.name             # (a change inside the window of n <= 33 may move the anchor by a base or two)
            defeated[change] += 1
    assert taken == set(K.I_N) and {n for n in K.I_N if n % 32 == 31} <= control
    assert set(defeated) == set(K.I_CHANGES[1:5]) and sum(defeated.values()) == 2 * len(K.I_N)
    assert {(c.name.split('-')[1][0], _ending(c, hs)[0].lenA < _ending(c, hs)[0].lenB) for c, (_, hs) in zip(cases, an)} == {(a, b) for a in 'rl' for b in (True, False)}


# ------------------------------------------------------------------------------------------------ family T
def test_t_ties_are_where_they_were_designed():
    cases, an, _ = family('T')
    for c, ((at, aq), hs) in zip(cases, an):
        kind, side = c.name.split('-')[1:3]
        k = 0 if side == 'l' else 1
        A, B = K.halves(c.T, c.Qs, at, aq)[k]
        o, e, y = c.oey
        w = K.walk(A, B, o, e, y)
        bs, bi, bj = w.best
        if kind == 'return':
            assert (bi + 2, bj + 2) in w.ties and w.rows > bi + 2, c.name        # the best score again, two rows on
        elif kind == 'rowtie':
            assert bi == w.lenA and (bi, bj + K.T2_GAP) in w.ties, c.name           # ... and T2_GAP columns on, in the last row
            threads = 1024 if y == 70000 else 256                                    # k6_dp_any; k6_trace under paths=True
            assert hs[k][1]['kernel'] == ('any' if y == 70000 else 'lean')
            assert K.dp_waves(w, bi, bj, threads, o, e, y) != K.dp_waves(w, bi, bj + K.T2_GAP, threads, o, e, y), c.name
        else:
            i = 110 + 60 + 10 - (side == 'l')                                         # the last of the ten C rows
            kept = K.walk(A, B, o, e, y, keep=(i,)).kept[i]
            u = np.where(kept[1] > K.LIVE, kept[1] + e * np.arange(kept[1].size), K.DEAD)
            src = np.flatnonzero(u == u.max()) + kept[0]
            assert src.tolist() == [i, i + 2], (c.name, src)                          # two sources of the column gap, one arriving score
            assert bi > i + 100 and bj - bi == 14, c.name                             # the best cell lies behind that gap
