"""Designed (target, query) pairs for the gap-free stage (rules 2-4) and a plain walk that says what they cover.

TEST INFRASTRUCTURE.  Every other test of the stage draws its similarity at random; here each case is ONE designed diagonal in
random sequence, built from column recipes, so that a walk stops exactly on a block or window edge of the engine, a dip costs
exactly `xdrop`, a score is exactly `hspthresh`, and a later hit ends exactly at a dismissed head's reach.  Cases lie `SPACING`
bases apart, case k on diagonal q - t = 7 k + 11, a forced transversion just outside both ends of its copy.

A recipe is a string, one letter per column of the copy:
    =  identical column                                         x  transversion (the target's base decides the cost)
    c  identical C or G (exactly 100)                           v  A/C or G/T transversion (exactly -114)
    d  dip: query A against target T (exactly -123)             i  transition (-31)
    n  dip: query N (-100)                                      m  identical column, the target's base in lower case
`=`, `x`, `i` and `m` keep the target's random base; the others write the target too.

The walk (`walk`, `extended_hits`) is rule 3 of DESIGN.md §2 written from the text of tests/spec_v1.extend with numpy prefix sums;
it shares nothing with the oracle or the engine and exists to PROVE coverage (tests/test_host_gapfree_edges.py), not to check results.
"""
import numpy as np

SPACING = 1000
SEED = '1110100110010101111'
CARE = np.array([i for i, c in enumerate(SEED) if c == '1'])
NONCARE = [3, 5, 6, 9, 10, 12, 14]
CODE = np.full(256, 4, dtype=np.int64)
for _i, _c in enumerate(b'ACGT'):
    CODE[_c] = _i
    CODE[_c + 32] = _i
HOXD70 = np.array([[91, -114, -31, -123, -100], [-114, 100, -125, -31, -100], [-31, -125, 100, -114, -100],
                   [-123, -31, -114, 91, -100], [-100, -100, -100, -100, -100]], dtype=np.int64)
BASES = np.frombuffer(b'ACGT', dtype=np.uint8)
TRANSVERSIONS = {ord('A'): b'CT', ord('C'): b'AG', ord('G'): b'CT', ord('T'): b'AG'}
TRANSITION = {ord('A'): ord('G'), ord('G'): ord('A'), ord('C'): ord('T'), ord('T'): ord('C')}
COMPLEMENT = np.full(256, ord('N'), dtype=np.uint8)
for _a, _b in zip(b'ACGTacgt', b'TGCAtgca'):
    COMPLEMENT[_a] = _b


def revcomp(q):
    return COMPLEMENT[np.frombuffer(q, dtype=np.uint8)][::-1].tobytes()


# ---------------------------------------------------------------------------------------------- recipes
def arm(n, period, phase, anchor):
    """seedless arm of n columns: a transversion wherever the distance from the `anchor` end ('l' or 'r') is phase mod period.
    With period 4..6 no 19-window inside it passes 12of19; with phase >= 2 its anchor end closes on two matches, which outweigh
    any one transversion, so a best prefix can end exactly there."""
    s = ''.join('x' if d % period == phase else '=' for d in range(n))
    return s if anchor == 'l' else s[::-1]


def _pp(k):
    """period and phase of case k: all of 4..6 and every phase, two in three of them >= 2"""
    period = 4 + k % 3
    return period, (k // 3) % period


def family_a(every=1):
    """walk lengths: core 30, left arm 0..300 beside a right arm of 40, right arm 0..300 beside a left arm of 40, both long"""
    out = []
    for a in range(0, 301):
        p, ph = _pp(a)
        out.append(arm(a, p, ph, 'l') + '=' * 30 + arm(40, 5, 2, 'r'))
    for b in range(0, 301):
        p, ph = _pp(b + 1)
        out.append(arm(40, 5, 2, 'l') + '=' * 30 + arm(b, p, ph, 'r'))
    for k, n in enumerate((250, 256, 257, 300, 400)):
        out.append(arm(n, 4 + k % 3, 2, 'l') + '=' * 30 + arm(n, 4 + (k + 1) % 3, 3, 'r'))
    return out[::every]


WANTED_BEST = (31, 32, 33, 63, 64, 65, 79, 80, 81, 95, 96, 97, 255, 256, 257)


def family_a_exact():
    """walks of chosen lengths.  Stops: eight dip columns (984 > 910) end a walk at once, so with arms phased from the core the
    stop steps follow the arm lengths one by one; an exact core of 19 + r columns stops the right walk at step r + 8, and 8 is the
    least a walk at x-drop 910 can stop at.  Best prefixes: arms phased from their outer end close on two matches, so the prefix is the whole arm."""
    out = ['d' * 8 + '=' * (19 + r) + 'd' * 8 for r in range(83)]
    out += ['d' * 8 + arm(k, p, 2, 'r') + '=' * 30 + arm(k, p, 2, 'l') + 'd' * 8
            for k in list(range(0, 100)) + list(range(212, 250)) for p in (4, 5, 6)]
    for L in WANTED_BEST:
        out += [arm(L - 19 + e, 5, 2, 'l') + '=' * 30 for e in range(5)]     # a window may reach a few columns into the arm ...
        out.append(arm(L - 22, 6, 2, 'l') + 'xxx' + '=' * 30)                # ... but not across three transversions
        out.append('=' * 30 + arm(L - 11, 5, 2, 'r'))
    return out


def _no_seed_prefix(s):
    """s columns in front of a core in which no seed window can start"""
    return 'x' * s if s < 3 else '=' * (s - 3) + 'xxx'


def family_ends():
    """for the cut-out scaffolds (Pair.cutouts): copies whose only seed window ends 0..11 columns before the copy does, and begins
    1..7 columns after it does — walks that run out of sequence after 0..11 steps to the right, after 20..26 to the left.  No
    x-drop can stop a walk that early: a column costs at most 125, and the seed holds at most seven mismatches."""
    return ['=' * (19 + r) for r in range(12)] + [_no_seed_prefix(s) + '=' * 19 for s in range(1, 8)]


def family_b(dips, every=1, dip='d', core='='):
    """x-drop dips: core 40, seedless gap g = 0..99 closing on the dip, dip of m columns, rescue 120 (seeded, or a seedless arm that
    opens with matches); on the right and, mirrored, on the left.  One gap in five closes on a mismatch instead: its best
    prefix ends before the dip and the boundary x-drop changes nothing."""
    out = []
    for m in dips:
        for g in range(0, 100, every):
            p, ph = _pp(g)
            if g % 5 != 4:
                ph = max(ph, 2)
            else:
                ph = g // 5 % 2
            for rescue in ('=' * 120, arm(120, 4 + g % 3, 2 + g % 2, 'l')):
                r = core * 40 + arm(g, p, ph, 'r') + dip * m + rescue
                out.append(r)
                out.append(r[::-1])
    return out


def family_c():
    """thresholds: exact cores of 19..45 columns between random flanks, random / mononucleotide-rich / dinucleotide-rich"""
    out = []
    for n in range(19, 46):
        out += [('=' * n, None), ('=' * n, None), ('=' * n, 'mono'), ('=' * n, 'di')]
    return out


def family_d():
    """reach: head X in a 46-column core whose best prefix ends at the core's end (= the diagonal's reach), then one column that is
    a transition when Y's seed is to end at reach + 1 (its care offset 18) and a transversion otherwise, four dip columns (X stops:
    31 + 492 > 500; a walk that starts behind the transition does not: 492), a seeded rescue.  Y's window ends at reach + delta
    and carries one or two transversions on its non-care offsets."""
    out = []
    for delta in (-1, 0, 1):
        for j, o in enumerate(NONCARE):
            for two in (False, True):
                core = ['='] * 46
                start = 46 + delta - 19          # Y's window within the copy
                core[start + o] = 'x'
                if two:
                    core[start + NONCARE[(j + 3) % 7]] = 'x'
                out.append((''.join(core) + ('i' if delta == 1 else 'x') + 'dddd' + '=' * 120, delta))
    return out


def family_e(nsteps, rescue):
    """the pre-filter's strict comparison: one seed window behind 24 transversions — C / G columns with a transversion on its
    non-care offset 3, so that the window one column earlier shows two mismatches to K34's ten-position seed test and nothing
    vetoes a dismissal — then a right walk whose running score falls to exactly -xdrop at step `nsteps` and never lower: eight
    -114 columns, then (+100, -114) pairs; then a rescue.  On the right every match is worth the filter's upper bound for a
    match and every transversion its upper bound for a transversion, so the bound is the score: `<` must leave the walk alive
    where `<=` proves a stop.  xdrop for the case = e_xdrop(nsteps)."""
    assert nsteps >= 8 and nsteps % 2 == 0
    return 'x' * 24 + 'cccx' + 'c' * 15 + 'v' * 8 + 'cv' * ((nsteps - 8) // 2) + ('=' * 200 if rescue == 'seeded' else arm(238, 4, 3, 'l'))


def e_xdrop(nsteps):
    return 8 * 114 + 14 * ((nsteps - 8) // 2)


# ---------------------------------------------------------------------------------------------- pairs
class Pair:
    """T, Q: bytes; cases: (t0, q0, n) of every copy; meta: whatever the family attached to each case"""

    def __init__(self, T, Q, cases, meta):
        self.T, self.Q, self.cases, self.meta = T, Q, cases, meta

    def cutouts(self):
        """every copy as a scaffold pair of its own, flush with both ends"""
        t, q = np.frombuffer(self.T, np.uint8), np.frombuffer(self.Q, np.uint8)
        return [(t[t0:t0 + n].copy(), q[q0:q0 + n].copy()) for t0, q0, n in self.cases]


def _low_complexity(rng, n, kind):
    unit = BASES[rng.permutation(4)[:1 if kind == 'mono' else 2]]
    s = np.resize(unit, n).copy()
    noise = rng.random(n) < 0.15
    s[noise] = BASES[rng.integers(0, 4, int(noise.sum()))]
    return s


def build(seed, recipes):
    """recipes: strings, or (string, extra) tuples — extra 'mono' / 'di' makes the target's segment low-complexity first and is
    kept, like anything else, as the case's meta"""
    rng = np.random.default_rng(seed)
    K = len(recipes)
    T = BASES[rng.integers(0, 4, SPACING * (K + 1))].copy()
    Q = BASES[rng.integers(0, 4, SPACING * (K + 1) + 7 * K + 11)].copy()
    cases, meta = [], []
    for k, r in enumerate(recipes):
        extra = None
        if isinstance(r, tuple):
            r, extra = r
        n = len(r)
        assert n + 2 <= SPACING - 100
        t0 = SPACING * (k + 1)
        q0 = t0 + 7 * k + 11
        if extra in ('mono', 'di'):
            T[t0:t0 + n] = _low_complexity(rng, n, extra)
        for j, c in enumerate(r):                          # target first
            if c in 'cv':
                T[t0 + j] = ord('CG'[rng.integers(0, 2)]) if c == 'c' else BASES[rng.integers(0, 4)]
            elif c == 'd':
                T[t0 + j] = ord('T')
        for j in list(range(n)) + [-1, n]:
            c = r[j] if 0 <= j < n else 'x'
            t = int(T[t0 + j])
            if c in '=cm':
                b = t
            elif c == 'x':
                b = TRANSVERSIONS[t][rng.integers(0, 2)]
            elif c == 'v':
                b = {ord('A'): ord('C'), ord('C'): ord('A'), ord('G'): ord('T'), ord('T'): ord('G')}[t]
            elif c == 'i':
                b = TRANSITION[t]
            elif c == 'd':
                b = ord('A')
            else:
                assert c == 'n', c
                b = ord('N')
            Q[q0 + j] = b
            if c == 'm':
                T[t0 + j] = t | 0x20
        cases.append((t0, q0, n))
        meta.append(extra)
    return Pair(T.tobytes(), Q.tobytes(), cases, meta)


# ---------------------------------------------------------------------------------------------- the plain walk
def columns(T, Q, d, lo, hi):
    """codes of the columns t = lo .. hi - 1 of diagonal q = t + d (upper case; 4 = not ACGT) and the target's case"""
    t = np.frombuffer(T, np.uint8)[lo:hi]
    q = np.frombuffer(Q, np.uint8)[lo + d:hi + d]
    return CODE[t], CODE[q], (t >= 97)


def diagonal_hits(T, Q, d, lo, hi, transitions=True):
    """rule 2 on one diagonal: the t of every seed hit whose window lies within [lo, hi)"""
    a, b, lower = columns(T, Q, d, lo, hi)
    bad = (a == 4) | (b == 4) | lower
    mism = a != b
    tv = mism & ((a ^ b) & 1 == 1)                        # A0 C1 G2 T3: a transition keeps the low bit
    w = np.lib.stride_tricks.sliding_window_view
    if hi - lo < 19:
        return []
    ok = ~w(bad, 19).any(axis=1)
    nm = w(mism, 19)[:, CARE].sum(axis=1)
    nt = w(tv, 19)[:, CARE].sum(axis=1)
    ok &= (nm <= 1) & (nt == 0) if transitions else (nm == 0)
    return [lo + int(i) for i in np.flatnonzero(ok)]


def walk(scores, xdrop):
    """rule 3, one side: `scores` in walking order.  (best, length of the first best prefix, steps taken): the walk stops after
    the step that leaves the running score more than xdrop below the best so far, or when the columns run out"""
    run = np.cumsum(scores)
    best = np.maximum(np.maximum.accumulate(run), 0) if run.size else run
    stop = np.flatnonzero(run < best - xdrop)
    steps = int(stop[0]) + 1 if stop.size else int(run.size)
    if steps == 0 or run[:steps].max() <= 0:
        return 0, 0, steps
    k = int(np.argmax(run[:steps]))
    return int(run[k]), k + 1, steps


def extended_hits(T, Q, case, xdrop=910, transitions=True, margin=60, reach_limit=1500):
    """rule 3's scan of one designed diagonal: for every hit that is extended (not skipped), a dict with its seed end, both best
    prefix lengths, both stop steps, the raw score and the reach it leaves; 'hits' of the first entry lists every hit's t"""
    t0, q0, n = case
    d = q0 - t0
    lo, hi = max(0, t0 - margin, -d + 0), min(len(T), t0 + n + margin, len(Q) - d)
    base, top = max(0, -d, t0 - reach_limit), min(len(T), len(Q) - d, t0 + n + reach_limit)   # a sequence end is a real end
    a, b, _ = columns(T, Q, d, base, top)
    sc = HOXD70[a, b]
    hits = diagonal_hits(T, Q, d, lo, hi, transitions)
    out, reach = [], 0
    for t in hits:
        et = t + 19
        if et <= reach:
            continue
        lb, ll, ls = walk(sc[:et - base][::-1], xdrop)
        rb, rl, rs = walk(sc[et - base:], xdrop)
        reach = et + rl
        out.append(dict(t=t, et=et, left_best=ll, right_best=rl, left_stop=ls, right_stop=rs, raw=lb + rb, reach=reach,
                        start=et - ll, hits=hits))
    return out


# ---------------------------------------------------------------------------------------------- K34's cheap bounds
K34_LEFT, K34_RIGHT = (24, 24, 24, 24), (24, 24, 16)


def k34_proven_block(a, b, xdrop, widths, strict=True):
    """pair_needs_walk's stop proof on one side (k34_filter.h: bound_block2), from the column codes in walking order: the index of
    the first block after which the walk is proven to have stopped, None if none is, and whether `up + xdrop == lomax` held at
    a checkpoint.  Columns behind a sequence end are identical, as the planes' zero padding makes them."""
    up = lomax = lo = 0
    proven, touched, pos = None, False, 0
    pad = np.zeros(max(0, sum(widths) - len(a)), dtype=np.int64)
    a, b = np.concatenate([a, pad]), np.concatenate([b, pad])
    for j, w in enumerate(widths):
        aa, bb = a[pos:pos + w], b[pos:pos + w]
        pn = int((aa != bb).sum())
        pv = int(((aa != bb) & (((aa ^ bb) & 1) == 1)).sum())
        up += 100 * w - 131 * pn - 83 * pv
        lo += 91 * w - 122 * pn - 94 * pv
        touched |= up + xdrop == lomax
        if proven is None and (up + xdrop < lomax if strict else up + xdrop <= lomax):
            proven = j
        lomax = max(lomax, lo)
        pos += w
    return proven, touched


def k4_proven_block(a, b, xdrop, nblocks=4, strict=True):
    """hit_needs_walk's stop proof on the right side (k4_device.h: bound_window with 16-step blocks, the walk-queue kernel's
    filter and MIMEO_HEAVY=v1's), from the column codes in walking order, as k34_proven_block.  Its upper bound U counts a
    match 91 (100 for C / G), a transition -31, a transversion -114 (-123 where the high bits differ too: A/T, C/G); the lower
    bound takes 2 more off each of the latter."""
    U = nb = lomax = 0
    proven, touched = None, False
    pad = np.zeros(max(0, 16 * nblocks - len(a)), dtype=np.int64)
    a, b = np.concatenate([a, pad]), np.concatenate([b, pad])
    for j in range(nblocks):
        x, y = a[16 * j:16 * j + 16], b[16 * j:16 * j + 16]
        dv = (x != y) & (((x ^ y) & 1) == 1)
        dt = (x != y) & ~dv
        da = (x == y) & ((x == 1) | (x == 2))
        db = dv & (((x ^ y) & 2) == 2)
        U += 91 * 16 + 9 * int(da.sum()) - 122 * int(dt.sum()) - 205 * int(dv.sum()) - 9 * int(db.sum())
        nb += int(db.sum())
        touched |= U + xdrop == lomax
        if proven is None and (U + xdrop < lomax if strict else U + xdrop <= lomax):
            proven = j
        lomax = max(lomax, U - 2 * nb)
    return proven, touched


K34_CARE10 = (0, 1, 2, 4, 7, 8, 11, 13, 15, 16)


def k34_needs_walk(T, Q, t, d, xdrop, hspthresh, strict=True):
    """pair_needs_walk (k34_filter.h) restated for a hit at target t on diagonal q = t + d, transitions allowed, away from the
    sequence ends and from N: False = the filter dismisses the hit.  A dismissal needs a stop proof on both sides, the bound of
    the two best prefixes below hspthresh, and no possible earlier seed hit of the diagonal (fewer than two mismatches on ten
    care positions) ending where the left walk arrives before its proven stop.  strict=False is the filter with `<=`."""
    et = t + 19
    a, b, _ = columns(T, Q, d, et - 128, et + 64)
    n = a != b
    left_a, left_b, right_a, right_b = a[32:128][::-1], b[32:128][::-1], a[128:], b[128:]

    def possible(step):
        return sum(int(n[108 - step + c]) for c in K34_CARE10) < 2

    def side(aa, bb, widths):
        up = lo = lomax = ub = 0
        stop, pos, stops = False, 0, []
        for w in widths:
            x, y = aa[pos:pos + w], bb[pos:pos + w]
            pn, pv = int((x != y).sum()), int(((x != y) & (((x ^ y) & 1) == 1)).sum())
            ub = max(ub, up + 100 * w - 100 * pn)
            up += 100 * w - 131 * pn - 83 * pv
            lo += 91 * w - 122 * pn - 94 * pv
            stop = stop or (up + xdrop < lomax if strict else up + xdrop <= lomax)
            lomax = max(lomax, lo)
            stops.append(stop)
            pos += w
        return stop, ub, stops

    lstop, lub, lstops = side(left_a, left_b, K34_LEFT)
    rstop, rub, _ = side(right_a, right_b, K34_RIGHT)
    veto = any(possible(s) for s in range(24))
    for j in range(3):
        if not lstops[j]:
            veto = veto or any(possible(s) for s in range(24 * (j + 1), 24 * (j + 2)))
    return not (lstop and rstop and lub + rub < hspthresh and not veto)


# ---------------------------------------------------------------------------------------------- what the tests run
def _runs(*variants):
    return [dict(v) for v in variants]


def suites(every=1):
    """name -> (Pair, parameter sets).  A parameter set holds hspthresh / xdrop / transitions / entropy for default_params and
    'minus': the query is handed over reverse-complemented and strand 1 asked for, which must find the designed diagonals again.
    every = k keeps every k-th case of a family (the Python restatement is slow).  Family C's thresholds come from its own
    HSPs: c_runs."""
    e4 = every if every > 1 else 4
    out = {
        'A': (build(101, family_a(every)), _runs({}, {'minus': 1}, {'transitions': 0})),
        'AX': (build(109, family_a_exact()[::every] + family_ends()[::min(every, 3)]), _runs({}, {'minus': 1}, {'hspthresh': 1500, 'entropy': 0})),
        'B6': (build(102, family_b([6], every)), _runs({'xdrop': 737}, {'xdrop': 738}, {'xdrop': 739}, {'xdrop': 738, 'minus': 1})),
        'B6N': (build(103, family_b([6], e4, dip='n')), _runs({'xdrop': 599}, {'xdrop': 600}, {'xdrop': 601})),
        'B6M': (build(104, family_b([6], e4, core='m')), _runs({'xdrop': 738})),
        'B78': (build(105, family_b([7, 8], e4)), _runs({}, {'transitions': 0})),
        'C': (build(106, family_c()[::every]), None),
        'D': (build(107, family_d()[::min(every, 3)]),
              _runs({'xdrop': 500, 'hspthresh': 6000}, {'xdrop': 500, 'hspthresh': 1500}, {'xdrop': 500, 'hspthresh': 6000, 'transitions': 0},
                    {'xdrop': 500, 'hspthresh': 6000, 'minus': 1})),
        'E': (build(108, [family_e(n, r) for n in E_STEPS for r in ('seeded', 'seedless')]),
              _runs(*[{'xdrop': e_xdrop(n), 'hspthresh': 6000} for n in E_STEPS])),
    }
    return out


E_STEPS = (16, 24, 32, 48, 64)     # right-walk checkpoints of hit_needs_walk (16, 32, 48, 64) and of pair_needs_walk (24, 48, 64)


def batched_cutouts(suites, every=5, oracle_every=5):
    """the cut-out scaffold pairs of the one batched call: every fifth case of families A, AX and B6 (a pair costs the engine's
    unit-per-pair path some 7 ms) and all of family_ends, which only mean something cut out.  Returns (pairs, checked): the
    indexes of the pairs that the call gives to the oracle as well — all of family_ends and every fifth of the others (the
    oracle spends 0.3 s of a CPU on a pair however small: its seed table)."""
    out, checked = [], []
    for name in ('A', 'AX', 'B6'):
        cuts = suites[name][0].cutouts()
        ends = len(family_ends()) if name == 'AX' else 0
        body = cuts[:len(cuts) - ends][::every]
        checked += list(range(len(out), len(out) + len(body), oracle_every))
        out += body
        checked += list(range(len(out), len(out) + ends))
        out += cuts[len(cuts) - ends:]
    return out, checked


def pick(values, n=6):
    """up to n of the distinct values, spread over their range"""
    v = sorted(set(int(x) for x in values))
    return v if len(v) <= n else [v[round(i * (len(v) - 1) / (n - 1))] for i in range(n)]


def c_runs(hsps, n=6):
    """family C: `hsps` = its HSPs at hspthresh 1500 with the entropy factor on.  n = six raw and six adjusted scores s; each is run
    as hspthresh = s and s + 1, with and without the entropy factor.  Returns (raw scores, adjusted scores, parameter sets)."""
    raw, adj = pick(hsps['raw_score'], n), pick(hsps['score'], n)
    runs = [{'hspthresh': s + k, 'entropy': e} for s in sorted(set(raw + adj)) for k in (0, 1) for e in (1, 0)]
    return raw, adj, runs


def query(pair, run):
    """(query bytes, strand) of a parameter set"""
    return (revcomp(pair.Q), 1) if run.get('minus') else (pair.Q, 0)


def engine_kw(run):
    return {k: v for k, v in run.items() if k != 'minus'}
