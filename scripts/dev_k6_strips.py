#!/usr/bin/env python3
"""development aid, CPU only: what a narrower first strip width would save k6_dp1, from the exact live band of seeded half extensions.

120 halves built like synth_genome's copies (a consensus of 300 .. 6000 bases, two copies of it with substitution divergence
U[0, 0.15] and indel rate 0.005 each, 3 kbp of unrelated sequence behind either) go through tests/k6_cases.walk_c, which gives the
first and last live column of every row.  A row of the lean kernel at ws columns per lane is taken to cost (36 ws + 85) / 589 of a
row at 14 (VALU instructions of the gfx950 build: 169 + 267 in the two unrolled blocks of 14 cells, the rest for the cross-lane scan,
the row maximum and the slide), whatever part of its 64 ws columns is live.  Per first width the table gives the halves that outgrow
the window and the cost of all rows against one pass at 14 when such a half runs again from row 1 at 14, and when it moves its state
to 14 columns per lane after the first row that ends with the last strip but one live and goes on (what k6_dp1 does from 7; a row
that jumps over that strip, or row 0, runs again); last the ladder 7 -> 11 -> 14 of the second kind, which is not built.

This is a model of instruction counts, not a measurement: DESIGN.md (section 4 K6, section 7 item 4) sets the kernel times of an MI355X beside it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mimeo_amd.synth import _mutate   # noqa: E402
from tests import k6_cases as K       # noqa: E402

FULL = 14


def cost(ws):
    return (36.0 * ws + 85.0) / (36.0 * FULL + 85.0)


def half(seed):
    rng = np.random.Generator(np.random.PCG64(seed))
    cons = rng.integers(0, 4, size=int(rng.integers(300, 6001)), dtype=np.uint8)
    a, b = (np.concatenate([_mutate(rng, cons, float(rng.random()) * 0.15, 0.005), rng.integers(0, 4, size=3000, dtype=np.uint8)]) for _ in range(2))
    return K.walk_c(a, b)


def leaves(w, ws):
    """the first row that does not fit 64 strips of ws columns (0: row 0), the first row that ends with strip 62 live, or None"""
    if w.hi[0] >= 63 * ws:
        return 0, 0
    rl = w.hi[1:] // ws - w.lo[:-1] // ws
    over, last = np.flatnonzero(rl >= 63), np.flatnonzero(rl >= 62)
    return (int(over[0]) + 1 if over.size else None), (int(last[0]) + 1 if last.size else None)


def main():
    walks = [half(1000 + k) for k in range(120)]
    rows = np.array([w.rows for w in walks])
    widest = np.array([int((w.hi[1:] - w.lo[1:] + 1).max()) for w in walks])
    span = np.concatenate([w.hi[1:] - w.lo[1:] + 1 for w in walks])
    print('halves %d, rows per half: mean %.0f; widest band of a half: %d .. %d columns; live span of a row: mean %.0f median %.0f 90th percentile %.0f'
          % (len(walks), rows.mean(), widest.min(), widest.max(), span.mean(), np.median(span), np.percentile(span, 90)))
    computed = 0
    for w in walks:                                           # k6_dp1: 448 cells a row up to the handover, 896 after it
        over, last = leaves(w, 7)
        n7 = w.rows if last is None else (0 if over is not None and over <= last else last)
        computed += 448 * n7 + 896 * (w.rows - n7)
    print('live share of the cells computed per row: %.2f at 14 columns per lane throughout, %.2f from 7 with the handover'
          % (span.sum() / (896.0 * rows.sum()), span.sum() / float(computed)))
    total = float(rows.sum())
    print('first width (window) | halves that outgrow it | cost, run again at 14 | cost, go on at 14')
    for ws in (7, 10, 11, 12):
        n, again, goon = 0, 0.0, 0.0
        for w in walks:
            over, last = leaves(w, ws)
            if over is None:
                again += w.rows * cost(ws)
            else:
                n += 1
                again += max(over - 1, 0) * cost(ws) + w.rows
            # go on: the state moves in the row that ends with strip 62 live; a row that jumps over it, or row 0, runs again
            if last is None:
                goon += w.rows * cost(ws)
            elif over is not None and over <= last:
                goon += max(over - 1, 0) * cost(ws) + w.rows
            else:
                goon += last * cost(ws) + (w.rows - last)
        print('%2d (%3d) | %3.0f %% | %.2f | %.2f' % (ws, 64 * ws, 100.0 * n / len(walks), again / total, goon / total))
    ladder = 0.0
    for w in walks:
        a = leaves(w, 7)[1]
        b = leaves(w, 11)[1]
        a = w.rows if a is None else a
        b = w.rows if b is None else max(a, b)
        ladder += a * cost(7) + (b - a) * cost(11) + (w.rows - b)
    print('ladder 7 -> 11 -> 14, going on at each step: %.2f' % (ladder / total))


if __name__ == '__main__':
    main()
