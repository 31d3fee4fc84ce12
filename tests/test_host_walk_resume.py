"""The designed diagonals of tests/walk_resume_cases.py, on the CPU: that they sit on the hand-over of a walk from the walk kernel
to k4_extend_generic (64 steps from the seed end, per direction) is ASSERTED with the plain walk of tests/gapfree_cases.py, and
the oracle is held to the second restatement (tests/spec_v1.py) on them.  tests/test_gpu_walk_resume.py holds the engine to the
oracle on the same pairs.  A family that misses a condition is to be changed; the condition is not."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import gapfree_cases as G
from tests import spec_v1 as S
from tests import walk_resume_cases as W

COLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
HAND_OVER = 64
_cache = {}


def pairs():
    if 'pairs' not in _cache:
        _cache['pairs'] = W.pairs()
    return _cache['pairs']


def heads(name):
    if ('heads', name) not in _cache:
        _cache['heads', name] = W.head_walks(pairs()[name])
    return _cache['heads', name]


def group(name):
    g = W.family()[1][name]
    return [heads('R')[i] for i in g]


def test_every_head_starts_with_its_core():
    """the arithmetic of walk_resume_cases rests on it: left step s of the head is column et - s, right step s column et + s - 1"""
    recipes, groups = W.family()
    R = pairs()['R']
    for name, rng in groups.items():
        for i in rng:
            want = recipes[i].index('=' * 30) if name != 'found' else recipes[i].index('=' * 19)
            assert heads('R')[i]['t'] - R.cases[i][0] == want, (name, i)


def test_left_walks_around_the_hand_over():
    hs = group('left')
    assert all(h['right_stop'] < HAND_OVER for h in hs)                       # only the left walk can be handed over
    assert set(W.STOPS) <= {h['left_stop'] for h in hs}
    # a best prefix that ends just before, at and just behind the hand-over, of a walk that goes on past it
    assert set(W.BESTS) <= {h['left_best'] for h in hs if h['left_stop'] > HAND_OVER}
    # ... and walks that end inside the frame, whose hits never reach k4_extend_generic, beside them
    assert any(h['left_stop'] <= HAND_OVER for h in hs) and any(h['left_stop'] > HAND_OVER for h in hs)


def test_right_walks_around_the_hand_over_beside_a_left_walk_that_finished_early():
    hs = group('right')
    assert all(h['left_stop'] < HAND_OVER and h['left_best'] > 0 for h in hs)  # the finished left walk's best and bk are handed over
    assert set(W.STOPS) <= {h['right_stop'] for h in hs}
    assert set(W.BESTS) <= {h['right_best'] for h in hs if h['right_stop'] > HAND_OVER}
    assert any(h['right_stop'] <= HAND_OVER for h in hs)


def test_both_walks_beyond_the_hand_over():
    """the left walk is alive after 64 steps: its record is written, the right walk has not begun"""
    hs = group('both')
    both = [h for h in hs if h['left_stop'] > HAND_OVER and h['right_stop'] > HAND_OVER]
    assert len(both) >= 4
    assert any(h['left_stop'] == HAND_OVER + 1 and h['right_stop'] == HAND_OVER + 1 for h in both)
    assert any(h['left_stop'] == HAND_OVER and h['right_stop'] > HAND_OVER for h in hs)      # the left walk ends ON the edge
    assert any(h['left_stop'] > 256 and h['right_stop'] > 256 for h in both)


def test_walks_of_255_256_257_steps():
    """LONG_WINDOWS counts from the seed: 256 steps end in k4_extend_generic, 257 go to k4_extend_long"""
    assert [h['left_stop'] for h in group('long_left')] == list(W.LONG)
    assert [h['right_stop'] for h in group('long_right')] == list(W.LONG)
    assert all(h['left_stop'] < HAND_OVER for h in group('long_right'))


def test_an_earlier_seed_hit_just_behind_the_hand_over():
    """the follower's left walk is alive when it reaches the end of the nearest earlier seed hit, at step 64 (the frame's last),
    65, 66 and 70"""
    R = pairs()['R']
    steps = []
    for i in W.family()[1]['found']:
        hits = heads('R')[i]['hits']
        assert len(hits) == 2, hits                                           # one head, one follower, nothing between
        steps.append(hits[1] - hits[0])
        assert W.left_walk_of(R, R.cases[i], hits[1])[2] > steps[-1]
    assert steps == list(W.FOUND)


def test_a_query_n_at_steps_64_and_65():
    RN = pairs()['RN']
    q = np.frombuffer(RN.Q, np.uint8)
    left, right = [], []
    for h, (t0, q0, n) in zip(heads('RN'), RN.cases):
        (col,) = np.flatnonzero(q[q0:q0 + n] == ord('N'))
        et = h['et'] - t0
        if col < et:
            left.append(et - col)
            assert h['left_stop'] > left[-1] + 8 and h['right_stop'] < HAND_OVER   # the walk survives the N
        else:
            right.append(col - et + 1)
            assert h['right_stop'] > right[-1] + 8 and h['left_stop'] < HAND_OVER
    assert left == [64, 65] and right == [64, 65]


def test_the_sequence_ends_at_the_hand_over_in_the_cut_out_scaffolds():
    """limit reached after exactly 64 and 65 steps: the walk is alive when it runs out of sequence"""
    R = pairs()['R']
    cuts = W.cut_head_walks(R)
    groups = W.family()[1]
    for side, name in (('left', 'limit_left'), ('right', 'limit_right')):
        got = []
        for i in groups[name]:
            h, n = cuts[i], R.cases[i][2]
            room = h['et'] if side == 'left' else n - h['et']
            assert h[side + '_stop'] == room and h[side + '_best'] == room, (name, h)    # no x-drop: the columns ran out
            got.append(room)
        assert got == [64, 65], (name, got)


@pytest.mark.parametrize('name,minus', [('R', 0), ('R', 1), ('RN', 0)])
def test_oracle_equals_the_second_restatement(name, minus):
    pair = pairs()[name]
    q, strand = G.query(pair, {'minus': minus})
    got = O.ungapped_hsps(pair.T, q, strand, O.default_params(chain=0))
    exp = S.ungapped_hsps(pair.T.decode(), S.revcomp(q.decode()) if strand else q.decode(), 3000, 910, True, True)
    assert sorted(tuple(int(h[c]) for c in COLS) for h in got) == sorted(exp)
    assert len(exp) >= len(pair.cases) // 2
