"""The model of K6's rounds (tests/k6_round_cases.py: simulate) on hand-worked groups, and the take it is run with.  CPU only; the
engine is held to the same model in tests/test_gpu_k6_rounds.py."""
import pytest

from tests import k6_round_cases as R


def far(i):
    """anchor i of a group of unrelated copies: 100 000 target bases and 50 000 diagonals from its neighbours"""
    return (50000 + 100000 * i, 1000 + 50000 * i)


def small_box(a, h=300):
    return (a[0] - h, a[0] + h, a[1] - h, a[1] + h)


def run(anchors, take, boxes=None, **kw):
    boxes = boxes or {}
    return R.simulate(anchors, lambda r: boxes.get(r, small_box(anchors[r])), take, **kw)


def test_the_default_take():
    """200 groups of a C4 row and the 32 of C5MID come out at the limit; thousands of small groups share the budget; at least one"""
    assert R.default_take(200) == R.LIMIT and R.default_take(32) == R.LIMIT and R.default_take(1) == R.LIMIT
    edge = R.ROUND_ANCHORS // R.LIMIT                       # the most groups that still take the limit each
    assert R.default_take(edge) == R.LIMIT and R.default_take(edge + 1) == R.LIMIT - 1
    assert R.default_take(4096) == R.ROUND_ANCHORS // 4096 and R.default_take(R.ROUND_ANCHORS) == 1 and R.default_take(10 ** 6) == 1
    assert R.default_take(200, env=32) == 32 and R.default_take(200, env=0) == 1 and R.default_take(200, env=1000) == R.LIMIT
    assert R.RESOLVE_NEW >= R.LIMIT


@pytest.mark.parametrize('n, take, jobs', [
    (32, 32, [64]), (32, R.LIMIT, [64]),                  # exactly the old cap: one round either way
    (33, 32, [64, 2]), (33, R.LIMIT, [66]),               # old cap + 1: the second round is the cap's, and goes with it
    (40, 32, [64, 16]), (40, R.LIMIT, [80]),
    (R.LIMIT, R.LIMIT, [2 * R.LIMIT]), (R.LIMIT + 1, R.LIMIT, [2 * R.LIMIT, 2]),          # the new limit and limit + 1
    (129, 32, [64] * 4 + [2]), (5, 1, [2] * 5),
])
def test_unrelated_copies_take_ceil_n_over_take_rounds(n, take, jobs):
    anchors = [far(i) for i in range(n)]
    out = run(anchors, take)
    assert out['jobs'] == jobs and out['rounds'] == len(jobs)
    assert out['accepted'] == list(range(n)) and out['wasted'] == []
    assert out == run(anchors, take, guard=False)     # more than GUARD_DIAG diagonals apart: the guard does nothing


@pytest.mark.parametrize('take', [1, 2, 32, R.LIMIT])
def test_a_deferred_fragment_that_is_swallowed_costs_nothing(take):
    """F is 700 bases and 50 diagonals from A and inside A's alignment: it waits for A's DP and is skipped by A's box"""
    anchors = [(10000, 10000), (10700, 10650)]
    out = run(anchors, take, boxes={0: (9000, 12000, 9000, 12000)})
    assert out['jobs'] == [2] and out['accepted'] == [0] and out['wasted'] == [] and out['invocations'] == 1


@pytest.mark.parametrize('take', [1, 2, 32, R.LIMIT])
def test_a_deferred_fragment_that_is_not_swallowed_takes_a_second_round(take):
    anchors = [(10000, 10000), (10700, 10650)]
    out = run(anchors, take)                          # A's box ends 300 bases from A
    assert out['jobs'] == [2, 2] and out['accepted'] == [0, 1] and out['wasted'] == []


def test_pending_anchors_defer_too_and_only_twice():
    """B near A; C near B, not near A; D near C only.  Round 1: A and C run, B waits (A scheduled), D waits (C scheduled).  The replay
    stops at B, so C stays pending.  Round 2: B runs; D is near the pending C and waits a second time.  Round 3: D runs.  With E
    near D as well: E has waited twice by round 3 and runs beside D"""
    A, B, C, D = (10000, 10000), (12000, 11900), (19000, 18800), (26000, 25700)
    out = run([A, B, C, D], R.LIMIT)
    assert out['jobs'] == [4, 2, 2] and out['accepted'] == [0, 1, 2, 3] and out['wasted'] == []
    E = (27000, 26750)       # near D (250 diagonals from C too, 8000 bases: near C)
    out = run([A, B, C, D, E], R.LIMIT)
    assert out['jobs'] == [4, 2, 4] and out['accepted'] == [0, 1, 2, 3, 4]


def collinear(n, step=20000, drift=7):
    """the HSPs of one long collinear alignment: `step` bases apart (not near), the diagonal drifting by `drift` per HSP"""
    return [(100000 + step * i, 90000 + step * i - drift * i) for i in range(n)]


def test_the_guard_holds_a_collinear_group_to_the_old_cap():
    """rank 0's alignment holds every anchor.  Without the guard the limit's take runs all 50 DPs; with it the first 32 only, which is
    what the take of 32 runs"""
    anchors = collinear(50)
    whole = {0: (0, 10 ** 7, 0, 10 ** 7)}
    assert run(anchors, R.LIMIT, boxes=whole, guard=False)['jobs'] == [100]
    new, old = run(anchors, R.LIMIT, boxes=whole), run(anchors, 32, boxes=whole)
    assert new['jobs'] == old['jobs'] == [64] and new['accepted'] == [0] and len(new['wasted']) == 31
    assert run(anchors, 33, boxes=whole)['jobs'] == [64] and run(anchors, 31, boxes=whole)['jobs'] == [62]


def test_the_guard_keeps_no_count_and_never_stalls():
    """70 anchors on one band, none swallowed (short boxes): every round takes 32, as the take of 32 does, however often an anchor waited"""
    anchors = collinear(70)
    new, old = run(anchors, R.LIMIT), run(anchors, 32)
    assert new['jobs'] == old['jobs'] == [64, 64, 12] and new['accepted'] == list(range(70))


def test_the_guard_lets_other_diagonals_through():
    """40 collinear HSPs swallowed by rank 0, ranked above 40 unrelated copies: the round takes 32 of the band and all the others"""
    band, others = collinear(40), [far(i + 100) for i in range(40)]
    anchors = band + others
    out = run(anchors, R.LIMIT, boxes={0: (0, 2 * 10 ** 6, 0, 2 * 10 ** 6)})
    assert out['jobs'] == [2 * (32 + 40)] and out['accepted'] == [0] + list(range(40, 80)) and len(out['wasted']) == 31
    assert run(anchors, 32, boxes={0: (0, 2 * 10 ** 6, 0, 2 * 10 ** 6)})['jobs'] == [64, 64, 16]


def test_the_guard_counts_the_band():
    """unrelated copies land on each other's diagonals now and then: past the 32nd, an anchor with fewer than GUARD_COUNT scheduled
    ones within the band is taken, with GUARD_COUNT it waits"""
    base = [far(i) for i in range(32)]
    for members in (1, R.GUARD_COUNT - 1, R.GUARD_COUNT):
        mates = [(5 * 10 ** 6 + 20000 * k, 5 * 10 ** 6 - 4 * 10 ** 6 + 20000 * k + 9 * k) for k in range(members)]    # one band, far from base
        late = (9 * 10 ** 6, 5 * 10 ** 6 + 100)                                                                        # on that band
        out = run(mates + base + [late], R.LIMIT)
        want = [2 * (members + 33)] if members < R.GUARD_COUNT else [2 * (members + 32), 2]
        assert out['jobs'] == want and out['wasted'] == [], (members, out['jobs'])


def test_the_scan_window_and_the_accept_list():
    """PICK_SCAN ranks per pick: swallowed fragments that fill the window between two copies cost the copy behind them a round of its
    own (and no DP for themselves); one fragment fewer and it runs in the first"""
    A, Z = far(0), far(50)
    for nfrag, jobs in ((R.PICK_SCAN - 1, [2, 2]), (R.PICK_SCAN - 2, [4])):
        frag = [(A[0] + 10 + i % 900, A[1] + 10 + i % 900) for i in range(nfrag)]      # inside A's box below
        out = run([A] + frag + [Z], R.LIMIT, boxes={0: (A[0] - 1000, A[0] + 1000, A[1] - 1000, A[1] + 1000)})
        assert out['accepted'] == [0, nfrag + 1] and out['jobs'] == jobs and out['wasted'] == []
