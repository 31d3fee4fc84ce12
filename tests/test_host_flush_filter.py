"""The sharp filter of K34's walk-queue flush (tests/flush_filter_spec.py restates k34_filter.h: pair_needs_walk_sharp) against
the exact walk of tests/spec_v1.py: a pair it dismisses must be one for which the exact walk emits nothing — no follower (no
earlier seed hit of the diagonal ends where the left walk arrives), both walks over inside the frame (80 steps to the left of the
seed end, 64 to the right), and a score below the threshold.  On the designed diagonals of tests/gapfree_cases.py, which put
stops, dips and seed windows on the block edges, and on 10^5 seeded random diagonals with a planted seed hit, a fifth of them
within 192 bases of a sequence end on either side.  The GPU side of the same change is tests/test_gpu_flush_filter.py."""
import numpy as np
import pytest

from tests import flush_filter_spec as F
from tests import gapfree_cases as G
from tests import spec_v1 as S

LEFT_STEPS, RIGHT_STEPS = 80, 64


def walks(Tu, Qu, t, q, xdrop):
    """rule 3 as spec_v1.extend walks it, with what extend does not return: per side (best, steps taken, length of the first best
    prefix); a walk ends with the step that trips the x-drop or when the columns run out.  Held to extend's own score, start and
    length by the caller."""
    et, eq = t + 19, q + 19
    out = []
    for n, col in ((min(et, eq), lambda k: (Tu[et - 1 - k], Qu[eq - 1 - k])), (min(len(Tu) - et, len(Qu) - eq), lambda k: (Tu[et + k], Qu[eq + k]))):
        run = best = steps = length = 0
        for k in range(n):
            run += S.score(*col(k))
            steps = k + 1
            if run > best:
                best, length = run, k + 1
            if run < best - xdrop:
                break
        out.append((best, steps, length))
    return out


def is_seed_hit(Tu, Qu, T, t, q, transitions):
    """rule 2 for one pair of windows (T: the target with its case)"""
    if t < 0 or q < 0 or t + 19 > len(Tu) or q + 19 > len(Qu):
        return False
    if any(c not in 'ACGT' for c in T[t:t + 19]) or any(c not in 'ACGT' for c in Qu[q:q + 19]):
        return False
    mism = [(Tu[t + k], Qu[q + k]) for k in S.CARE if Tu[t + k] != Qu[q + k]]
    if not mism:
        return True
    return bool(transitions) and len(mism) == 1 and mism[0] in S.TRANSITION


def check_dismissed(T, Q, t, q, xdrop, hspthresh, transitions, tag):
    """the three properties of a dismissed pair, from the exact walk"""
    Tu, Qu = S.upper(T), S.upper(Q)
    (lb, ls, ll), (rb, rs, rl) = walks(Tu, Qu, t, q, xdrop)
    ts, qs, length, raw, rend = S.extend(Tu, Qu, t, q, xdrop)
    assert (ts, length, raw, rend) == (t + 19 - ll, ll + rl, lb + rb, t + 19 + rl), tag      # the step counter walks as extend does
    assert ls <= LEFT_STEPS and rs <= RIGHT_STEPS, (tag, 'a walk leaves the frame', ls, rs)
    assert raw < hspthresh, (tag, 'the score reaches the threshold', raw)
    for k in range(1, ls + 1):                                                               # every boundary the left walk reaches
        assert not is_seed_hit(Tu, Qu, T, t - k, q - k, transitions), (tag, 'a follower', k)


# ------------------------------------------------------------------------------------------------ designed families
@pytest.mark.parametrize('name', ['A', 'AX', 'B6', 'B6N', 'B6M', 'B78', 'C', 'D', 'E'])
def test_no_designed_diagonal_is_dismissed_wrongly(name):
    """every seed hit of every designed diagonal (every third case of the large families), under every parameter set of its
    family: frames straight from the two sequences, soft-masked and N columns included"""
    if 'suites' not in _cache:
        _cache['suites'] = G.suites(every=3)
    pair, runs = _cache['suites'][name]
    runs = [r for r in (runs or [{}, {'hspthresh': 1500}]) if not r.get('minus')]
    T, Q = pair.T.decode(), pair.Q.decode()
    seen = dismissed = 0
    for run in runs:
        xdrop, hsp, tr = run.get('xdrop', 910), run.get('hspthresh', 3000), run.get('transitions', 1)
        hits = []
        for t0, q0, n in pair.cases:
            d = q0 - t0
            hits += [(t, t + d) for t in G.diagonal_hits(pair.T, pair.Q, d, max(0, t0 - 60), min(len(T), t0 + n + 60), bool(tr))]
        a, b, nflag = F.frames(pair.T, pair.Q, hits)
        need = F.sharp_needs_walk(a, b, nflag, xdrop, hsp, bool(tr))
        seen += len(hits)
        for i in np.flatnonzero(~need):
            dismissed += 1
            check_dismissed(T, Q, hits[i][0], hits[i][1], xdrop, hsp, tr, (name, run, hits[i]))
    print('%s: %d seed hits on the designed diagonals, %d dismissed by the sharp filter' % (name, seen, dismissed))
    assert seen > 0
    # Families AX (cores of 19 + r columns between dips), C (cores of 19 .. 45 columns) and E (one window behind 24 transversions)
    # hold isolated heads that score too little: there the rule does dismiss, and each dismissal was walked above.  The other
    # families are long similarity with seeds all along: for them this test proves that nothing designed is dismissed at all.
    assert (dismissed > 0) == (name in DISMISSING), (name, dismissed)


_cache = {}
DISMISSING = ('AX', 'C', 'E')


def test_designed_cut_outs_with_frames_over_both_sequence_ends():
    """the cut-out scaffold pairs (the copy flush with both ends of its scaffolds): every frame hangs over a sequence end"""
    if 'suites' not in _cache:
        _cache['suites'] = G.suites(every=3)
    cuts = G.batched_cutouts(_cache['suites'], every=2)[0]
    seen = dismissed = 0
    for tb, qb in cuts:
        T, Q = tb.tobytes(), qb.tobytes()
        hits = [(t, t) for t in G.diagonal_hits(T, Q, 0, 0, min(len(T), len(Q)))]
        if not hits:
            continue
        a, b, nflag = F.frames(T, Q, hits)
        for hsp in (3000, 1500):
            need = F.sharp_needs_walk(a, b, nflag, 910, hsp)
            seen += len(hits)
            for i in np.flatnonzero(~need):
                dismissed += 1
                check_dismissed(T.decode(), Q.decode(), hits[i][0], hits[i][1], 910, hsp, 1, ('cut', hits[i]))
    print('cut-outs: %d seed hits, %d dismissed' % (seen, dismissed))
    assert seen > 0 and dismissed == 0      # (every cut-out is one copy from end to end: seeds all along, nothing to dismiss)


# ------------------------------------------------------------------------------------------------ random diagonals
NRANDOM, WIDTH, C0 = 100_000, 704, 352       # diagonals; columns generated per diagonal; column of the planted seed's first base


def random_diagonals(seed, n):
    """n diagonals of WIDTH columns, a seed hit planted at column C0 of each: target and query rows (ASCII), and the part of each
    row that is its sequence [lo, hi).  Half of them are unrelated sequence around the planted hit — the isolated hits that
    flood a scan — half carry similarity of 50 .. 95 % identity over 0 .. 150 columns to either side of it, transitions and
    transversions in equal parts.  A fifth have an end of the target within 192 bases of the hit, a fifth an end of the query."""
    rng = np.random.default_rng(seed)
    t = rng.integers(0, 4, (n, WIDTH))
    q = rng.integers(0, 4, (n, WIDTH))
    col = np.arange(WIDTH)[None, :]
    related = rng.random(n) < 0.5
    left, right = rng.integers(0, 151, n), rng.integers(0, 151, n)
    inside = related[:, None] & (col >= C0 - left[:, None]) & (col < C0 + 19 + right[:, None])
    rate = rng.uniform(0.05, 0.5, n)[:, None]
    mut = rng.random((n, WIDTH)) < rate
    kind = rng.choice(np.array([2, 1, 3]), size=(n, WIDTH), p=[0.5, 0.25, 0.25])    # xor 2: the transition; xor 1, xor 3: the transversions
    sim = np.where(mut, t ^ kind, t)
    q = np.where(inside, sim, q)
    care = C0 + F.CARE
    q[:, care] = t[:, care]                                  # the planted seed hit ...
    one = rng.random(n) < 0.5                                # ... half of them with one transition at a care position
    at = care[rng.integers(0, 12, n)]
    q[one, at[one]] ^= 2
    tlo, thi, qlo, qhi = (np.zeros(n, dtype=np.int64), np.full(n, WIDTH), np.zeros(n, dtype=np.int64), np.full(n, WIDTH))
    u = rng.random(n)
    near = rng.integers(0, 192, n)
    tlo = np.where(u < 0.1, C0 - near, tlo)
    thi = np.where((u >= 0.1) & (u < 0.2), C0 + 19 + near, thi)
    qlo = np.where((u >= 0.2) & (u < 0.3), C0 - near, qlo)
    qhi = np.where((u >= 0.3) & (u < 0.4), C0 + 19 + near, qhi)
    both = (u >= 0.4) & (u < 0.45)                            # a short pair: all four ends near
    tlo, qlo = np.where(both, C0 - near, tlo), np.where(both, C0 - rng.integers(0, 192, n), qlo)
    thi, qhi = np.where(both, C0 + 19 + rng.integers(0, 192, n), thi), np.where(both, C0 + 19 + rng.integers(0, 192, n), qhi)
    return t, q, related, (tlo, thi, qlo, qhi)


def test_random_diagonals_with_a_planted_seed_hit():
    """10^5 seeded diagonals: no dismissed pair is a follower, leaves the frame or reaches the threshold — and the share of the
    pairs the cheap filter passes that the sharp filter dismisses, printed (the walk-queue entries the flush filter saves)"""
    t, q, related, (tlo, thi, qlo, qhi) = random_diagonals(20261, NRANDOM)
    col = np.arange(C0 - F.FRAME_LEFT, C0 - F.FRAME_LEFT + F.FRAME)
    a, b = t[:, col].copy(), q[:, col].copy()
    outside = (col[None, :] < tlo[:, None]) | (col[None, :] >= thi[:, None])
    a[outside] = 0
    outside = (col[None, :] < qlo[:, None]) | (col[None, :] >= qhi[:, None])
    b[outside] = 0
    nflag = np.zeros(NRANDOM, dtype=bool)
    letters = np.frombuffer(b'ACGT', np.uint8)
    checked = 0
    for xdrop, hsp, tr in ((910, 3000, True), (910, 1500, True), (500, 3000, False)):
        # (without transitions only the exact planted hits are seed hits)
        rows = np.arange(NRANDOM) if tr else np.flatnonzero((t[:, C0 + F.CARE] == q[:, C0 + F.CARE]).all(1))
        sharp = F.sharp_needs_walk(a[rows], b[rows], nflag[rows], xdrop, hsp, tr)
        cheap = F.cheap_needs_walk(a[rows], b[rows], nflag[rows], xdrop, hsp, tr)
        for name, sel in (('unrelated', ~related[rows]), ('related', related[rows]), ('all', np.ones(rows.size, dtype=bool))):
            passed = cheap & sel
            print('xdrop %d hspthresh %d transitions %d, %s: %d pairs, cheap filter passes %d (%.1f %%), sharp filter dismisses %d of those (%.1f %%)'
                  % (xdrop, hsp, tr, name, int(sel.sum()), int(passed.sum()), 100.0 * passed.sum() / max(1, sel.sum()),
                     int((passed & ~sharp).sum()), 100.0 * (passed & ~sharp).sum() / max(1, passed.sum())))
        # the pairs the flush filter sees are those the cheap filter passed; the rule must hold for every pair all the same
        todo = rows[np.flatnonzero(~sharp)]
        if (xdrop, hsp, tr) != (910, 3000, True):
            todo = todo[::4]                                  # the default parameters in full, a quarter under the others
        for i in todo:
            T = letters[t[i, tlo[i]:thi[i]]].tobytes().decode()
            Q = letters[q[i, qlo[i]:qhi[i]]].tobytes().decode()
            check_dismissed(T, Q, C0 - tlo[i], C0 - qlo[i], xdrop, hsp, tr, (int(i), xdrop, hsp, tr))
            checked += 1
    print('%d dismissed pairs walked exactly' % checked)
    assert checked > NRANDOM // 2


# ------------------------------------------------------------------------------------------------ the earlier-seed-hit proof
# Columns with exact scores, (target, query): identical A 91, identical C 100, A against C -114, A against G (a transition) -31.
# With these the filter's bounds ARE the scores (no A/T or C/G transversion: U is exact and nb stays 0), so a walk can be put
# on the edge of the x-drop.
COLS = {'a': (0, 0), 'c': (1, 1), 'v': (0, 1), 'i': (0, 2)}
SCORE = {'a': 91, 'c': 100, 'v': -114, 'i': -31}
CARE_SET = set(int(c) for c in F.CARE)


def _filler(n, lo, hi, start, floor):
    """n columns that take the running score from `start` down into [lo, hi] without ever going below `floor`: mostly -114
    columns, so that no seed window fits, spread evenly, the last ones negative"""
    for x in range(n, 0, -1):                                  # x columns of -114, y of -31, the rest +91
        for y in range(n - x + 1):
            z = n - x - y
            end = start - 114 * x - 31 * y + 91 * z
            if not lo <= end <= hi:
                continue
            left, out, run = {'v': x, 'i': y, 'a': z}, [], start
            for k in range(n):
                line = start + (end - start) * (k + 1) / n     # the straight line from start to end
                order = ('v', 'i', 'a') if run > line else ('a', 'i', 'v')
                c = next(c for c in order if left[c])
                left[c] -= 1
                run += SCORE[c]
                out.append(c)
            runs = np.cumsum([SCORE[c] for c in out]) + start
            if runs.min() >= floor:
                return ''.join(out)
    raise AssertionError('no filler')


def edge_diagonal(s, alive, xdrop=910):
    """a diagonal whose head at column C0 has an earlier seed hit — one transition at its care offset 18 — ending exactly where
    left step s arrives (its window: steps s + 1 .. s + 19).  Left side in walking order: the head's own seed (care columns
    identical, the others -114: no shifted window passes), two -114 columns, eleven +100 columns — the best prefix ends at the
    32-step checkpoint, so the filter's lower bound IS the best score B —, then a filler that sinks to just above B - xdrop at
    step s (alive: the exact walk is still going when it arrives there, and finds the earlier hit: a FOLLOWER) or to far below it
    by step 56 (not alive: the walk is over before, the hit is a head).  The earlier hit's own columns then carry the
    score below B - xdrop at the 80-step checkpoint in the alive case too: the stop IS proven there, and only the veto of
    boundary s stands between the pair and a wrong dismissal.  The right walk dies at once (sixteen -114 columns)."""
    left = ''.join('a' if (18 - j) in CARE_SET else 'v' for j in range(19)) + 'vv' + 'c' * 11
    best = sum(SCORE[c] for c in left)
    floor = best - xdrop
    window = ''.join(('i' if o == 18 else 'a') if o in CARE_SET else 'v' for o in range(18, -1, -1))      # steps s + 1 .. s + 19
    part = sum(SCORE[c] for c in window[:79 - s])             # what the window adds up to the 80-step checkpoint
    n = s + 1 - len(left)
    if alive:
        assert part < 0, (s, part)
        left += _filler(n, floor, floor - part - 1, best, floor)
    else:
        left += _filler(24, floor - 400, floor - 250, best, floor - 400)          # over by step 56 ...
        left += ('vai' * 9)[:n - 24]                                               # ... and sinking on
    left += window
    rng = np.random.default_rng(1000 + s)
    t, q = rng.integers(0, 4, WIDTH), rng.integers(0, 4, WIDTH)
    q[:C0 + 19 - len(left)] = (t[:C0 + 19 - len(left)] + 1 + 2 * rng.integers(0, 2, C0 + 19 - len(left))) & 3   # beyond: transversions only
    for j, c in enumerate(left):
        t[C0 + 18 - j], q[C0 + 18 - j] = COLS[c]
    for j in range(16):
        t[C0 + 19 + j], q[C0 + 19 + j] = COLS['v']
    letters = np.frombuffer(b'ACGT', np.uint8)
    return letters[t].tobytes(), letters[q].tobytes(), best


EDGE_STEPS = (63, 65, 69)     # the boundaries at which the earlier hit's columns dip below their start before the 80-step checkpoint


@pytest.mark.parametrize('s', EDGE_STEPS)
def test_an_earlier_seed_hit_at_the_edge_of_the_x_drop_is_never_dismissed(s):
    """the exact walk is alive when it reaches boundary s and finds the earlier hit there, the stop is proven at the 80-step
    checkpoint and not at the 64-step one: the rule keeps the pair — because of boundary s alone: a rule that looked at
    steps 0 .. 59 only (s = 63), or not at steps 64 .. 79 (s = 65, 69), would dismiss a follower"""
    T, Q, best = edge_diagonal(s, alive=True)
    Tu, Qu = T.decode(), Q.decode()
    (lb, ls, ll), _ = walks(Tu, Qu, C0, C0, 910)
    assert lb == best and ls > s + 1, (lb, best, ls)                                  # alive beyond boundary s ...
    assert is_seed_hit(Tu, Qu, Tu, C0 - s - 1, C0 - s - 1, True)                      # ... where an earlier seed hit ends
    assert not any(is_seed_hit(Tu, Qu, Tu, C0 - k, C0 - k, True) for k in range(1, s + 1))
    a, b, nflag = F.frames(T, Q, [(C0, C0)])
    assert F.sharp_needs_walk(a, b, nflag)[0], 'a follower is dismissed'
    if s < 64:
        assert not F.sharp_needs_walk(a, b, nflag, early_steps=60)[0], 'the case does not pin steps 60 .. 63'
    else:
        assert not F.sharp_needs_walk(a, b, nflag, late_steps=(64, 64))[0], 'the case does not pin steps 64 .. 79'
        assert F.sharp_needs_walk(a, b, nflag, late_steps=(64, s + 1))[0]


@pytest.mark.parametrize('s', (65, 69, 72, 79))
def test_an_earlier_seed_hit_behind_a_proven_stop_does_not_keep_the_pair(s):
    """the same diagonal with the walk over before step 64: the stop is proven within 64 steps, the boundaries 64 .. 79 do not
    count, and the pair is dismissed — rightly: the exact walk never arrives at the earlier hit"""
    T, Q, best = edge_diagonal(s, alive=False)
    Tu, Qu = T.decode(), Q.decode()
    assert is_seed_hit(Tu, Qu, Tu, C0 - s - 1, C0 - s - 1, True)
    a, b, nflag = F.frames(T, Q, [(C0, C0)])
    assert not F.sharp_needs_walk(a, b, nflag)[0], 'not dismissed'
    check_dismissed(Tu, Qu, C0, C0, 910, 3000, 1, ('edge', s))


def test_a_second_seed_hit_at_every_offset_to_the_left_of_the_head():
    """otherwise unrelated diagonals with a second seed hit — exact, or with one transition at a care position — 1 .. 80 columns
    to the left of the planted one, 150 of each, and the same with the second window broken by a transversion at a care
    position.  Up to 64 columns away the real one always keeps the pair; further away it does not once the stop is proven
    within 64 steps, and then the walk never reaches it; the broken one keeps nothing.  No dismissed pair is a follower."""
    per = 150
    rng = np.random.default_rng(77)
    letters = np.frombuffer(b'ACGT', np.uint8)
    dismissed = {True: np.zeros(81, dtype=int), False: np.zeros(81, dtype=int)}
    for real in (True, False):
        for k in range(1, 81):
            t, q = rng.integers(0, 4, (per, WIDTH)), rng.integers(0, 4, (per, WIDTH))
            for c0 in (C0 - k, C0):                                  # the second window first: the planted hit wins where they overlap
                q[:, c0 + F.CARE] = t[:, c0 + F.CARE]
            free = [c for c in F.CARE if C0 - k + c < C0]            # care columns of the second window outside the planted one
            at = C0 - k + rng.choice(free, per)
            kind = rng.integers(0, 2, per) if real else np.full(per, 2)
            rows = np.arange(per)
            q[rows, at] = np.where(kind == 0, q[rows, at], np.where(kind == 1, q[rows, at] ^ 2, q[rows, at] ^ 1))
            col = np.arange(C0 - F.FRAME_LEFT, C0 - F.FRAME_LEFT + F.FRAME)
            need = F.sharp_needs_walk(t[:, col], q[:, col], np.zeros(per, dtype=bool))
            if real and k <= 64:
                assert need.all(), (k, 'a pair with an earlier seed hit %d columns back is dismissed' % k)
            for i in np.flatnonzero(~need):
                dismissed[real][k] += 1
                check_dismissed(letters[t[i]].tobytes().decode(), letters[q[i]].tobytes().decode(), C0, C0, 910, 3000, 1, (real, k, int(i)))
    print('dismissed with a real second hit, by distance:', dismissed[True][60:].tolist())
    print('dismissed with a broken one: %d of %d' % (dismissed[False].sum(), 80 * per))
    assert dismissed[True][65:].min() > 0 and dismissed[False][1:].min() > 0
