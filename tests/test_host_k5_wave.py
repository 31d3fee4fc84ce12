"""The model of the wave chain kernel's steps (tests/k5_wave_cases.py) held to groups worked by hand, the coverage proof of the designed
sets (one predicate per family, asserted over the model's output: no GPU), the C oracle's chain held to the rule in plain Python on
the designed sets, and what the random sets of tests/test_gpu_chain.py reach of the same kernel."""
import numpy as np
import pytest

from tests import k5_wave_cases as W

N, T, O, V, I = W.NONE, W.TREE, W.ONWAY, W.WINDOW, W.INTILE


def _hsps(rows):
    from oracle import oracle as Or
    h = np.zeros(len(rows), dtype=Or.HSP)
    for f, col in zip(('tstart', 'qstart', 'length', 'score'), zip(*rows)):
        h[f] = col
    return h


# Groups worked by hand.  Rows are (tstart, qstart, length, score) in sorted order.  A group of up to 64 HSPs is one step (tile_end = n):
# a tile when some member starts at or behind the smallest end behind the first start, a wave otherwise.
HAND = {
    # ends (target) 15 18 20, (query) 15 46 20.  The smallest end > 10 is 15, member 2 starts on it: a tile; its window is what ends at or
    # before member 2's start: 1 (member 0).  Member 2 follows member 0 (15 <= 15 in both): 50 + 40 = 90 < member 1's 100.
    'three': dict(rows=[(10, 10, 5, 50), (12, 40, 6, 100), (15, 15, 5, 40)],
                  tcnt=[0, 0, 1], qcnt=[0, 2, 1], qpos=[1, 3, 2], epos=[0, 1, 2], steps=[(0, 3, False, 0, 0, 1)],
                  census=(3, 1, 0, 0, 1, 1, 1), best=[50, 100, 90], pred=[-1, -1, 0], src=[N, N, I], flags=[0, 1, 0]),
    # all four start before the first end (150): a wave, nothing is asked but the (empty) tree.  Target ends 150 160 170 159: E = 0 3 1 2.
    # Two chains of 30: the earliest end wins.
    'wave-of-four': dict(rows=[(100, 100, 50, 10), (110, 300, 50, 30), (120, 200, 50, 30), (149, 500, 10, 5)],
                         tcnt=[0, 0, 0, 0], qcnt=[0, 2, 1, 3], qpos=[1, 3, 2, 4], epos=[0, 2, 3, 1], steps=[(0, 4, True, 0, 0, 0)],
                         census=(4, 0, 1, 4, 0, 0, 0), best=[10, 30, 30, 5], pred=[-1, -1, -1, -1], src=[N, N, N, N], flags=[0, 1, 0, 0]),
    # ends that equal starts (`<=`): member 2 (10, 10) follows member 0 (ends 10, 10) but not member 1 (query end 30); member 3 (10, 30)
    # follows both, 7 against 7: the earlier.  Member 4 (20, 40) follows 2 and 3 (12 against 12, query ends 20 and 40 <= 40): member 2.
    # Member 5 (query start 9) follows nobody: 13 = member 4's 13, the earlier end wins: chain 4, 2, 0.
    'ties-on-ends': dict(rows=[(0, 0, 10, 7), (0, 20, 10, 7), (10, 10, 10, 5), (10, 30, 10, 5), (20, 40, 5, 1), (25, 9, 5, 13)],
                         tcnt=[0, 0, 2, 2, 4, 5], qcnt=[0, 3, 1, 4, 5, 0], qpos=[1, 4, 3, 5, 6, 2], epos=[0, 1, 2, 3, 4, 5],
                         steps=[(0, 6, False, 0, 0, 5)], census=(6, 1, 0, 0, 5, 1, 5), best=[7, 7, 12, 12, 13, 13], pred=[-1, -1, 0, 0, 2, -1],
                         src=[N, N, I, I, I, N], flags=[1, 0, 1, 0, 1, 0], tied={3: {I: 2}, 4: {I: 2}}),
    # two diagonals of six, a_i = (100 + 20 i, same, 20) at 10 and b_i = (105 + 20 i, 400 + 20 i, 20) at 11, interleaved in the target.  a_i
    # follows a_(i-1) only (the b lie behind it in the query); b_i follows a_j and b_j for j < i: 11 i against 10 i, b_(i-1).
    # tcnt[a_i] = i + max(0, i - 1), tcnt[b_i] = 2 i; qcnt[a_i] = i, qcnt[b_i] = 6 + i.
    'two-diagonals': dict(rows=[r for i in range(6) for r in ((100 + 20 * i, 100 + 20 * i, 20, 10), (105 + 20 * i, 400 + 20 * i, 20, 11))],
                          tcnt=[0, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10], qcnt=[0, 6, 1, 7, 2, 8, 3, 9, 4, 10, 5, 11],
                          qpos=[1, 7, 2, 8, 3, 9, 4, 10, 5, 11, 6, 12], epos=list(range(12)), steps=[(0, 12, False, 0, 0, 10)],
                          census=(12, 1, 0, 0, 10, 1, 10), best=[10, 11, 20, 22, 30, 33, 40, 44, 50, 55, 60, 66],
                          pred=[-1, -1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9], src=[N, N] + [I] * 10, flags=[0, 1] * 6),
}


@pytest.mark.parametrize('name', list(HAND))
def test_model_on_groups_worked_by_hand(name):
    from oracle import oracle as Or
    g = HAND[name]
    h = _hsps(g['rows'])
    m = W.model(h[::-1])                                               # the model sorts
    assert [tuple(r) for r in zip(*(m.sorted[f].tolist() for f in ('tstart', 'qstart', 'length', 'score')))] == g['rows']
    for f in ('tcnt', 'qcnt', 'qpos', 'epos', 'best', 'pred', 'flags'):
        assert getattr(m, f).tolist() == g[f], (name, f, getattr(m, f).tolist())
    assert [(t.a, t.b, t.pure, t.c, t.ca, t.cend) for t in m.steps] == g['steps']
    assert tuple(m.census[k] for k in ('n', 'tiles', 'waves', 'members', 'window', 'chunks', 'widest')) == g['census']
    assert m.src == g['src']
    assert {k: d for k, d in enumerate(m.tied) if len(d) > 1 or max(d.values(), default=0) > 1} == g.get('tied', {})
    assert W.rule(h)[3].tolist() == g['flags'] and (Or.chain_hsps(h)['flags'] & 1).tolist() == g['flags']


def test_model_on_a_run_of_130_in_closed_form():
    """Three steps cannot be had below 65 HSPs.  The run of 130 (`tiny/tail2`): HSP k starts on the end of k - 1, so tcnt[k] = qcnt[k] =
    k, the smallest end behind a step's first start is the second member's start: tiles [0, 64) [64, 128) [128, 130) with c = 0, 0, 64,
    ca = 0, 64, 128 and cend = 63, 127, 129: windows 63, 127, 65.  The predecessor of k is k - 1: a member of the tile, but for k = 64
    and 128, whose predecessor ended on the tile's first start: on the way (a run never asks the tree for anything that matters)."""
    h, m = W.case('tiny', 'tail2')
    assert m.tcnt.tolist() == m.qcnt.tolist() == list(range(130)) and m.qpos.tolist() == list(range(1, 131))
    assert [(t.a, t.b, t.pure, t.c, t.ca, t.cend) for t in m.steps] == [(0, 64, False, 0, 0, 63), (64, 128, False, 0, 64, 127), (128, 130, False, 64, 128, 129)]
    assert W.census_line(m) == '[k5w] group 0: n 130 tiles 3 waves 0 (members 0) window entries 255 chunks 5 widest 127'
    assert m.pred.tolist() == list(range(-1, 129)) and m.src == [N] + [I] * 63 + [O] + [I] * 63 + [O, I]
    assert m.best.tolist() == [4500 * (k + 1) for k in range(130)] and m.inserts.tolist() == list(range(1, 129))


def test_model_on_a_window_of_two_in_closed_form():
    """`small-window/w2-window`, the smallest group with all four sources: a run of 64 (10 bases each from 1000: a tile, c = 0), a wave of
    64 long HSPs from 2000 and two spacers (2064, 2065) that end at 2167 and 2168, the tile X of 64 from 2167: c = 64 (the wave's first
    start lies behind the whole run), ca = 65 (the run and the first spacer), cend = 66.  X's first member finds the first spacer on
    the way, the members with a high query start behind it the second in the window, those with a low query start the run's last HSP in
    the tree."""
    h, m = W.case('small-window', 'w2-window')
    assert [(t.a, t.b, t.pure, t.c, t.ca, t.cend) for t in m.steps] == [(0, 64, False, 0, 0, 63), (64, 130, True, 0, 64, 64), (130, 194, False, 64, 65, 66)]
    assert m.sorted['tstart'][[128, 129, 130, 131]].tolist() == [2064, 2065, 2167, 2168] and m.te[[128, 129]].tolist() == [2167, 2168]
    assert m.epos[[63, 128, 129]].tolist() == [63, 64, 65]
    x = range(130, 194)
    assert m.src[130] == O and m.pred[130] == 128
    assert all((m.src[k], m.pred[k]) == ((T, 63) if (k - 130) % 3 == 1 and k != 193 else (V, 129)) for k in x[1:])
    assert m.best[193] == 64 * 900 + 21000 + int(m.sorted['score'][193]) and m.flags[[63, 129, 193]].all() and m.flags.sum() == 66


@pytest.mark.parametrize('family,name', W.CASES, ids=['%s/%s' % c for c in W.CASES])
def test_designed_set_shows_what_it_exists_for(family, name):
    """the coverage proof: the predicate of the family's row over the model's output, and what holds for every group"""
    h, m = W.case(family, name)
    print(family, name, W.check(family, name, m))
    print(W.census_line(m))
    assert 2 <= h.size <= 6000 and m.steps[0].c == m.steps[0].ca == 0
    for i, t in enumerate(m.steps):
        assert t.pure or t.b - t.a >= 2                                # a lone member is a wave
        assert t.pure or i == 0 or t.c < t.ca < t.cend                 # a later tile's window: one entry on the way, one behind, at least
    assert sum(t.b - t.a for t in m.steps) == m.n and len(W.CASES) < 100


def test_designed_sets_reach_the_edges_between_them():
    """what a reviewer looks for, in one place: the windows, waves, ranks, ties and scores that the random sets do not reach"""
    wins, waves, asked, put, pairs, top = set(), set(), set(), set(), set(), 0
    for family, name in W.CASES:
        m = W.case(family, name)[1]
        wins |= {t.cend - t.c for t in m.steps if not t.pure}
        waves |= {t.b - t.a for t in m.steps if t.pure}
        asked |= set(m.queries.tolist())
        put |= set(m.inserts.tolist())
        on = np.flatnonzero(m.flags)
        pairs |= {(a, b) for k in on for a in m.tied[k] for b in m.tied[k] if a < b or (a == b and m.tied[k][a] > 1)}
        top = max(top, int(m.best.max()))
    assert {1, 2, 7, 8, 9, 56, 57, 448, 449, 1000, 3000} <= wins
    assert {1, 2, 64, 65, 511, 512, 513, 1025} <= waves
    assert {0, 1024, 1025, 2048} <= asked and {1024, 1025, 2049, 4097, 5000} <= put
    assert {(T, V), (I, V), (I, I), (O, T)} <= pairs, pairs          # on the best chain, so in the flags
    assert 1 << 32 < top < 1 << 39


@pytest.mark.parametrize('family', list(W.FAMILIES))
def test_c_oracle_chain_against_the_rule_on_designed_sets(family):
    """the second witness where the oracle's own tie rule carries everything: `orc_chain_hsps` against DESIGN.md §2 rule 5 in plain
    Python (tests/test_oracle_golden.py does the same on random sets) on every designed set of up to 1500 HSPs; the model's flags, a
    third statement, on all of them.  domain-top: the rule works in Python integers, the oracle in int64: both hold 2.1 * 10^11."""
    from oracle import oracle as Or
    done = 0
    for name in W.FAMILIES[family]:
        h, m = W.case(family, name)
        got = Or.chain_hsps(h)
        for f in ('tstart', 'qstart', 'length', 'score', 'raw_score'):
            assert np.array_equal(got[f], m.sorted[f]), (name, f)
        assert np.array_equal(got['flags'] & 1, m.flags), name
        if h.size <= 1500:
            s, best, pred, flags = W.rule(h)
            assert np.array_equal(got['flags'] & 1, flags), name
            assert best == m.best.tolist() and pred == m.pred.tolist(), name
            done += 1
    assert done >= min(2, len(W.FAMILIES[family]))


def test_what_the_random_sets_of_test_gpu_chain_reach():
    """The four random kinds of tests/test_gpu_chain.py (`_make`, the wave kernel's seed, its sizes from 63 up) under the model.  They
    reach all four sources, and `ties` thousands of cross-source ties (the flags show the few that lie on the best chain; no set says
    which).  They do NOT reach, and the designed sets do:
      * a tile window of 1 to 7 entries (the share floor of 8, where six of the seven wavefronts get nothing): the smallest is 15, in
        `rectangles`; 44 in the other kinds;
      * a window above 448 entries (a share beyond one chunk of 64) outside `rectangles` (up to 1 933 there, from 1 024 HSPs on, at
        whatever entry the best chain happens to pass); random, collinear and ties stay at 140 and below;
      * a wave of 64 members (wave_end == tile_end), of 512 or of 513 (one trip of the 512-thread loop or two); waves of more than one
        member occur in `rectangles` alone;
      * a chain score above 2^32 or a coordinate near 2^31.
    Two wrong kernels were built to see the difference, both right on every random set and wrong here: one that skips a window of
    fewer than 8 entries (small-window fails), one that packs the low 32 bits of a chain score (domain-top fails)."""
    from tests.test_gpu_chain import _make
    rng = np.random.default_rng(20260 + len('wave'))
    seen = {}
    for kind in ('random', 'collinear', 'rectangles', 'ties'):
        wins, waves, srcs, cross, top = [], [], set(), 0, 0
        for n in (1, 2, 3, 63, 64, 65, 127, 129, 511, 1023, 1024, 1025, 2047, 2049, 3000, 4097, 9000):
            h = _make(kind, n, rng)                                    # every size is drawn: the stream the GPU test sees
            if n < 63:
                continue
            m = W.model(h)
            wins += [t.cend - t.c for t in m.steps if not t.pure]
            waves += [t.b - t.a for t in m.steps if t.pure]
            srcs |= set(m.src)
            cross += sum(1 for d in m.tied if len(d) > 1)
            top = max(top, int(m.best.max()), int(m.te.max()), int(m.qe.max()))
        seen[kind] = (min(wins), max(wins), sorted(set(w for w in waves if w > 1)), cross)
        print(kind, 'windows %d .. %d' % (min(wins), max(wins)), 'waves of more than one:', seen[kind][2][:6], '..', seen[kind][2][-3:], 'cross-source ties', cross)
        assert min(wins) >= (15 if kind == 'rectangles' else 44) and top < 1 << 32
        assert srcs == {N, T, O, V, I}
        assert not {64, 512, 513} & set(waves)
        if kind != 'rectangles':
            assert max(wins) <= 140 and not seen[kind][2]
    assert seen['rectangles'][1] > 448 and seen['rectangles'][2] and seen['ties'][3] > 1000
