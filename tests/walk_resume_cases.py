"""Designed diagonals for the hand-over of a walk from the walk kernel to k4_extend_generic ("K4 — the hits K34
passes on"): the walk kernel serves 64 steps per direction from its frame and hands a walk that is still alive on WITH ITS STATE
(running score, best prefix and where); k4_extend_generic resumes at step 65.  TEST INFRASTRUCTURE, built from the recipes of
tests/gapfree_cases.py; what the cases cover is asserted with its plain walk in tests/test_host_walk_resume.py.

Every case is  LEFT + 'xxx' + core of 30 + 'xxx' + RIGHT.  Three transversions cost less than the x-drop and leave no seed window
across them, so the diagonal's first seed hit (its head) starts with the core: left step s of the head is the column 22 + len(LEFT) - s
of the copy, right step s the column 21 + len(LEFT) + s.  An arm phased from its outer end closes on two matches (the best prefix
is the whole arm) and eight dip columns behind it stop the walk at once, so

    left  arm a:  best prefix 22 + a, stop 30 + a            right arm b:  best prefix 14 + b, stop 22 + b
"""
from tests import gapfree_cases as G

STOPS = (63, 64, 65, 66, 95, 96, 97)            # around the hand-over (64) and the end of the first resumed window (96)
BESTS = (63, 64, 65)
LONG = (255, 256, 257)                          # LONG_WINDOWS * 32 = 256 steps from the seed: the hand-off to k4_extend_long
FOUND = (64, 65, 66, 70)                        # left step at which an earlier seed hit's end is reached
SHORT_L, SHORT_R = 'd' * 8, 'd' * 8             # a walk that finishes early: left stop 30, right stop 22
CORE = '=' * 30


def _case(left, right):
    return left + 'xxx' + CORE + 'xxx' + right


def left_arm(a, k=0):
    return 'd' * 8 + G.arm(a, 4 + k % 3, 2, 'l')


def right_arm(b, k=0):
    return G.arm(b, 4 + k % 3, 2, 'r') + 'd' * 8


def _with(s, i, c):
    return s[:i] + c + s[i + 1:]


def gap(g):
    """g seedless columns between two seed windows: three transversions at either end, a transversion every fourth column between"""
    return 'xxx' + G.arm(g - 6, 4, 1, 'l') + 'xxx'


def family():
    """(recipes, groups): groups names the index ranges of the kinds of case"""
    out, groups = [], {}

    def add(name, recipes):
        groups[name] = range(len(out), len(out) + len(recipes))
        out.extend(recipes)

    # the left walk stops / has its best prefix around the hand-over, the right walk finishes early
    add('left', [_case(left_arm(a, a), SHORT_R) for a in list(range(31, 46)) + list(range(63, 70))])
    # ... and the right walk, beside a left walk that finishes early
    add('right', [_case(SHORT_L, right_arm(b, b)) for b in list(range(39, 53)) + list(range(71, 78))])
    # both walks beyond the hand-over: the left one is handed over, the right one starts in k4_extend_generic
    add('both', [_case(left_arm(a, a), right_arm(b, b)) for a, b in ((35, 43), (36, 44), (34, 50), (50, 42), (90, 120), (227, 235))])
    # 255, 256, 257 steps
    add('long_left', [_case(left_arm(s - 30, s), SHORT_R) for s in LONG])
    add('long_right', [_case(SHORT_L, right_arm(s - 22, s)) for s in LONG])
    # a follower whose left walk reaches the end of the nearest earlier seed hit at step s: one seed window, g = s - 19 seedless
    # columns, the follower's window
    add('found', ['d' * 8 + 'xxx' + '=' * 19 + gap(s - 19) + '=' * 19 + 'xxx' + 'd' * 8 for s in FOUND])
    # the sequence ends after exactly 64 and 65 steps (as cut-out scaffolds: Pair.cutouts): no dips, the arm is flush with the end
    add('limit_left', [_case(G.arm(s - 22, 5, 2, 'l'), SHORT_R) for s in (64, 65)])
    add('limit_right', [_case(SHORT_L, G.arm(s - 14, 5, 2, 'r')) for s in (64, 65)])
    return out, groups


def family_n():
    """a query N at steps 64 and 65 of the left walk, and of the right walk beside a left walk that finishes early.  A pair of its
    own: a strand that holds an N takes the walk kernel's full-plane variant, the others would follow it there."""
    out = []
    for s in (64, 65):
        left = left_arm(60)
        out.append(_case(_with(left, len(left) + 22 - s, 'n'), SHORT_R))
    for s in (64, 65):
        out.append(_case(SHORT_L, _with(right_arm(70), s - 15, 'n')))
    return out


def pairs():
    """name -> Pair"""
    return {'R': G.build(116, family()[0]), 'RN': G.build(117, family_n())}


def head_walks(pair, xdrop=910):
    """the plain walk on the head of every designed diagonal: gapfree_cases.extended_hits(...)[0]"""
    ex = [G.extended_hits(pair.T, pair.Q, c, xdrop) for c in pair.cases]
    assert all(ex)
    return [e[0] for e in ex]


def cut_head_walks(pair, xdrop=910):
    """... and of every cut-out scaffold pair"""
    ex = [G.extended_hits(t.tobytes(), q.tobytes(), (0, 0, t.size), xdrop) for t, q in pair.cutouts()]
    assert all(ex)
    return [e[0] for e in ex]


def left_walk_of(pair, case, t, xdrop=910):
    """the plain left walk of the seed hit at target t of a designed diagonal: (best, best prefix length, steps)"""
    d = case[1] - case[0]
    base = max(0, -d)
    a, b, _ = G.columns(pair.T, pair.Q, d, base, t + 19)
    return G.walk(G.HOXD70[a, b][::-1], xdrop)
