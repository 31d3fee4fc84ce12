"""The sharp filter that K34's first pass runs where it flushes its staged pairs (k34_filter.h: pair_needs_walk_sharp), restated
on seed FRAMES with numpy, and the cheap filter in front of it (pair_needs_walk) in the same form.

TEST INFRASTRUCTURE.  A frame is the 192 columns [p - 109, p + 83) around a seed start p (common.h): column 109 is the seed's
first base, column 128 the first step of the right walk, column 127 the first step of the left walk.  Here a frame is a row of
base codes (A0 C1 G2 T3), the target's and the query's of one seed hit side by side; columns outside a sequence are A on both
sides, as the planes' zero padding makes them, and a frame that holds a non-ACGT base is flagged and always walked.  Every
function takes N frames at once: a (N, 192) target codes, b (N, 192) query codes, nflag (N,) bool.

The rule (three proofs; a pair is DISMISSED when all hold, and the exact walk then emits nothing for it):
  1. both walks provably stop at a 16-step checkpoint — 80 steps to the left, 64 to the right: an upper bound U of the prefix
     score lies more than xdrop below a lower bound of the prefix score at an earlier checkpoint.  Per block, from the column
     classes: U += 91 n + 9 (identical C/G) - 122 (transitions) - 205 (transversions) - 9 (A/T or C/G transversions); the
     lower bound takes 2 more off every one of the latter;
  2. no seed window of the diagonal that passes 12of19 (one transition at a care position allowed) ENDS where one of the left
     steps 0 .. 63 arrives, nor where one of the steps 64 .. 79 does unless the stop was proven within 64 steps: the hit is a
     head.  The window that ends where step s arrives starts at column 108 - s;
  3. the bounds of the two best prefixes — per block: U at its start + 100 per identical column — sum to less than hspthresh.
"""
import numpy as np

FRAME, FRAME_LEFT = 192, 109
CARE = np.array([i for i, c in enumerate('1110100110010101111') if c == '1'])
CARE10 = np.array([0, 1, 2, 4, 7, 8, 11, 13, 15, 16])
LEFT_BLOCKS = [np.arange(127 - 16 * j - 15, 127 - 16 * j + 1) for j in range(5)]        # steps 16 j .. 16 j + 15
RIGHT_BLOCKS = [np.arange(128 + 16 * j, 128 + 16 * j + 16) for j in range(4)]


def frames(T, Q, hits):
    """frames of the seed hits (t, q) of two sequences (bytes; the target's case is ignored): a, b, nflag"""
    code = np.full(256, 4, dtype=np.int64)
    for i, c in enumerate(b'ACGT'):
        code[c] = code[c + 32] = i
    out = []
    for s, pos in ((T, [h[0] for h in hits]), (Q, [h[1] for h in hits])):
        c = code[np.frombuffer(s, np.uint8)]
        idx = np.asarray(pos, dtype=np.int64)[:, None] - FRAME_LEFT + np.arange(FRAME)[None, :]
        inside = (idx >= 0) & (idx < c.size)
        out.append(np.where(inside, c[np.clip(idx, 0, c.size - 1)], 0))
    a, b = out
    nflag = (a == 4).any(axis=1) | (b == 4).any(axis=1)
    return np.where(a == 4, 0, a), np.where(b == 4, 0, b), nflag


def _sharp_side(x, cg, blocks, xdrop):
    """proof 1 and the bound of proof 3 on one side: (stop after each block, bound of the best prefix)"""
    n = x.shape[0]
    U, lomax, ub, nb = (np.zeros(n, dtype=np.int64) for _ in range(4))
    stop, stops = np.zeros(n, dtype=bool), []
    for idx in blocks:
        xb = x[:, idx]
        dv, dt = ((xb & 1) == 1).sum(1), (xb == 2).sum(1)
        da, db = ((xb == 0) & cg[:, idx]).sum(1), (xb == 3).sum(1)
        ub = np.maximum(ub, U + 100 * (len(idx) - dv - dt))
        U = U + 91 * len(idx) + 9 * da - 122 * dt - 205 * dv - 9 * db
        nb = nb + db
        stop = stop | (U + xdrop < lomax)
        lomax = np.maximum(lomax, U - 2 * nb)
        stops.append(stop)
    return stops, ub


def _possible(x, start, care, transitions, exact):
    """may a seed window that starts at column `start` be a seed hit?  exact: the 12of19 rule; else fewer than two mismatches
    at the given care positions (K34's cheap superset)"""
    w = x[:, start + care]
    nm = (w != 0).sum(1)
    if not exact:
        return nm < 2 if transitions else nm == 0
    return ((nm <= 1) & (((w & 1) == 1).sum(1) == 0)) if transitions else nm == 0


def sharp_needs_walk(a, b, nflag, xdrop=910, hspthresh=3000, transitions=True, early_steps=64, late_steps=(64, 80)):
    """pair_needs_walk_sharp: True = the pair goes to the exact walk.  early_steps / late_steps are the shipped rule's; a test
    passes others only to show that a designed case would be dismissed wrongly by a rule that looked at fewer boundaries."""
    x = a ^ b
    cg = (a == 1) | (a == 2)
    lstops, lub = _sharp_side(x, cg, LEFT_BLOCKS, xdrop)
    rstops, rub = _sharp_side(x, cg, RIGHT_BLOCKS, xdrop)
    veto = np.zeros(a.shape[0], dtype=bool)
    for s in range(early_steps):
        veto |= _possible(x, 108 - s, CARE, transitions, True)
    late = np.zeros(a.shape[0], dtype=bool)
    for s in range(*late_steps):
        late |= _possible(x, 108 - s, CARE, transitions, True)
    veto |= late & ~lstops[3]                     # steps 64 .. 79 only count while no stop is proven within 64
    return nflag | ~(lstops[4] & rstops[3] & (lub + rub < hspthresh) & ~veto)


def _cheap_side(x, widths, first, step, xdrop):
    n = x.shape[0]
    up, lo, lomax, ub = (np.zeros(n, dtype=np.int64) for _ in range(4))
    stop, stops, pos = np.zeros(n, dtype=bool), [], first
    for w in widths:
        idx = np.arange(pos, pos + step * w, step)
        xb = x[:, idx]
        pn, pv = (xb != 0).sum(1), ((xb & 1) == 1).sum(1)
        ub = np.maximum(ub, up + 100 * w - 100 * pn)
        up = up + 100 * w - 131 * pn - 83 * pv
        lo = lo + 91 * w - 122 * pn - 94 * pv
        stop = stop | (up + xdrop < lomax)
        lomax = np.maximum(lomax, lo)
        stops.append(stop)
        pos += step * w
    return stops, ub


def cheap_needs_walk(a, b, nflag, xdrop=910, hspthresh=3000, transitions=True):
    """pair_needs_walk (K34's filter in front of the staging): blocks of 24 columns, two popcounts per block, ten care positions"""
    x = a ^ b
    lstops, lub = _cheap_side(x, (24, 24, 24, 24), 127, -1, xdrop)
    rstops, rub = _cheap_side(x, (24, 24, 16), 128, 1, xdrop)
    veto = np.zeros(a.shape[0], dtype=bool)
    for s in range(96):
        alive = np.ones(a.shape[0], dtype=bool) if s < 24 else ~lstops[s // 24 - 1]
        veto |= alive & _possible(x, 108 - s, CARE10, transitions, False)
    return nflag | ~(lstops[3] & rstops[2] & (lub + rub < hspthresh) & ~veto)
