"""The wave chain kernel's steps: a model of k5w_prepare / k5w_stats / k5_chain_wave (mimeo_amd/csrc/k5_wave.hip) and designed HSP sets
for every edge of it.

TEST INFRASTRUCTURE, beside tests/k6_round_cases.py.  `model` restates, for ONE group and from the kernels' text, how the wave kernel
cuts the sorted HSPs into steps and where every member's best predecessor comes from; it shares no code with the oracle or the engine.
Names as in k5_wave.hip: the HSPs lie in (tstart, qstart, length) order; E = the HSPs ordered by (target end, sorted order);
tcnt[k] / qcnt[k] = how many target / query ends are <= tstart[k] / qstart[k]; qpos[i] = 1-based rank of i by (query end, sorted order).

* A step begins at member a: next_end = the smallest target end > tstart[a]; wave_end = the first member >= a whose tstart >= next_end;
  tile_end = min(a + 64, n).  wave_end >= tile_end: the step is the pure wave [a, wave_end) (no member precedes another); otherwise the
  tile [a, tile_end).  c = the tcnt of the step before's first member (0 for the first step), ca = tcnt[a], cend = tcnt[b - 1].
* The census (`MIMEO_K5_STATS`, k5w_stats): n, tiles, waves, members of waves, window entries (cend - c per tile, summed), chunks
  (ceil(w / 64) per tile, summed), widest window.
* The source of a member's best predecessor (DESIGN.md §2 rule 5: best chain score, ties to the earliest predecessor in sorted order;
  only a positive chain is one), e = its position in E:  `tree` e < c (in the tree, visibly, when the step begins);  `on-the-way`
  c <= e < ca (in the window, put into the tree during the step);  `window` ca <= e < cend;  `tile` a member of the same tile;  `none`.
  A pure wave puts E[c, ca) into the tree BEFORE it asks: all its predecessors are `tree`.  The model asserts what the kernel relies
  on: a wave's members find every predecessor in E[.. ca), a tile's in E[.. cend) or in the tile.
* `tied[k]` = {source: how many candidates of that source reach the best chain score}: more than one key is a cross-source tie.
* The tree (n <= 2^22: blocks of 1024 ranks): every member asks for the prefix maximum over the first qcnt[k] ranks; every E[x] with
  x < the last step's ca is inserted at rank qpos.  `nblk`, `queries`, `inserts` report them.

Three facts the model shows about windows (tests/test_host_k5_wave.py holds them): a group of up to 64 HSPs is ONE step; a lone last
member is a pure wave of one, never a tile; a tile behind another step has at least one `on-the-way` and one later entry in its window,
so a window of ONE entry exists only in a group's first tile, and that entry is a member of the tile itself (not final: unused).

The designed sets (FAMILIES) are built from three primitives — a stack (k HSPs that all start before any of them ends), a run (a
collinear run, each HSP starting at the previous end) and spacers (HSPs that end in a chosen number between two starts) — and each
comes with the property it exists for as a predicate over the model's output (`check`).  Where the chain flags are all the engine
shows, the member that carries the property gets a score bonus: the best chain runs through it, so a wrong predecessor changes flags."""
import functools
from types import SimpleNamespace

import numpy as np

TILE = 64                   # CH_TILE
WAVE_THREADS = 512          # CW_THREADS
SHARES, SHARE_MIN = 7, 8    # the window is dealt to wavefronts 1 .. 7, 8 entries a share at least
BLOCK_SHIFT = 10            # tree blocks of 1024 ranks while n <= 2^22
TOP = 0x7FFFFF00            # scaffolds are shorter than 2^31 - 256 bases
NONE, TREE, ONWAY, WINDOW, INTILE = 'none', 'tree', 'on-the-way', 'window', 'tile'
_SRC = (TREE, ONWAY, WINDOW, INTILE)


# ---- the model --------------------------------------------------------------------------------------------------------------------
def sort_hsps(h):
    return h[np.lexsort((h['length'], h['qstart'], h['tstart']))]


def share_of(w):
    """entries per wavefront of a window of w entries"""
    return max((w + SHARES - 1) // SHARES, SHARE_MIN)


def model(h):
    s = sort_hsps(np.asarray(h))
    n = s.size
    assert 2 <= n <= 1 << 22
    ts, qs, ln, sc = (s[f].astype(np.int64) for f in ('tstart', 'qstart', 'length', 'score'))
    te, qe = ts + ln, qs + ln
    idx = np.arange(n)
    eorder, qorder = np.lexsort((idx, te)), np.lexsort((idx, qe))      # stable sorts of the sorted HSPs by end
    epos, qpos = np.empty(n, np.int64), np.empty(n, np.int64)
    epos[eorder], qpos[qorder] = idx, idx + 1
    kte, kqe = te[eorder], qe[qorder]
    tcnt, qcnt = np.searchsorted(kte, ts, 'right'), np.searchsorted(kqe, qs, 'right')   # bisect(.., upper)
    steps, a, c = [], 0, 0
    while a < n:
        next_end = kte[tcnt[a]]                                        # tcnt[a] < n: the HSP itself ends behind its start
        wave_end = a + int(np.searchsorted(ts[a:], next_end, 'left'))
        tile_end = min(a + TILE, n)
        pure = wave_end >= tile_end
        b = wave_end if pure else tile_end
        steps.append(SimpleNamespace(a=a, b=b, pure=pure, c=c, ca=int(tcnt[a]), cend=int(tcnt[b - 1]), wave_end=wave_end, tile_end=tile_end))
        c, a = int(tcnt[a]), b
    tiles = [t for t in steps if not t.pure]
    wins = [t.cend - t.c for t in tiles]
    census = dict(n=n, tiles=len(tiles), waves=len(steps) - len(tiles), members=sum(t.b - t.a for t in steps if t.pure),
                  window=sum(wins), chunks=sum((w + TILE - 1) // TILE for w in wins), widest=max(wins, default=0))
    best, pred = np.zeros(n, np.int64), np.full(n, -1, np.int64)
    src, tied, step_of = [NONE] * n, [{} for _ in range(n)], np.zeros(n, np.int64)
    for si, t in enumerate(steps):
        for k in range(t.a, t.b):
            step_of[k] = si
            cand = np.flatnonzero((te[:k] <= ts[k]) & (qe[:k] <= qs[k]) & (best[:k] > 0))
            if cand.size:
                top = cand[best[cand] == best[cand].max()]
                where = []
                for i in top:
                    if t.pure:
                        assert i < t.a and epos[i] < t.ca, 'a wave asks the tree alone'
                        where.append(TREE)
                    elif i >= t.a:
                        where.append(INTILE)
                    else:
                        assert epos[i] < t.cend, 'a tile sees E[.. cend) and itself'
                        where.append(TREE if epos[i] < t.c else ONWAY if epos[i] < t.ca else WINDOW)
                pred[k], src[k] = top[0], where[0]                     # the earliest of the best
                tied[k] = {w: where.count(w) for w in _SRC if w in where}
                best[k] = best[top[0]]
            best[k] += sc[k]
    flags = np.zeros(n, np.uint32)
    k = int(np.argmax(best))                                           # the first maximum
    while k >= 0:
        flags[k] = 1
        k = int(pred[k])
    last_ca = steps[-1].ca
    ins = eorder[:last_ca]
    return SimpleNamespace(n=n, sorted=s, te=te, qe=qe, tcnt=tcnt, qcnt=qcnt, qpos=qpos, epos=epos, steps=steps, census=census, best=best, pred=pred,
                           src=src, tied=tied, step_of=step_of, flags=flags, nblk=((n - 1) >> BLOCK_SHIFT) + 1, queries=qcnt,
                           inserts=qpos[ins[best[ins] > 0]])


def census_line(m, group=0):
    """the line chain_wave_groups prints for the group under MIMEO_K5_STATS"""
    c = m.census
    return '[k5w] group %d: n %d tiles %d waves %d (members %d) window entries %d chunks %d widest %d' % (
        group, c['n'], c['tiles'], c['waves'], c['members'], c['window'], c['chunks'], c['widest'])


def rule(h):
    """DESIGN.md §2 rule 5 in plain Python (Python integers): (the sorted HSPs, best, pred, flags)"""
    s = sort_hsps(np.asarray(h))
    ts, qs, ln, sc = (s[f].tolist() for f in ('tstart', 'qstart', 'length', 'score'))
    te, qe = [a + b for a, b in zip(ts, ln)], [a + b for a, b in zip(qs, ln)]
    best, pred = [0] * s.size, [-1] * s.size
    for j in range(s.size):
        b, p, tj, qj = 0, -1, ts[j], qs[j]
        for i in range(j):
            if te[i] <= tj and qe[i] <= qj and best[i] > b:
                b, p = best[i], i
        best[j], pred[j] = b + sc[j], p
    flags = np.zeros(s.size, dtype=np.uint32)
    k = max(range(s.size), key=lambda j: (best[j], -j))               # first maximum
    while k >= 0:
        flags[k] = 1
        k = pred[k]
    return s, best, pred, flags


# ---- primitives -------------------------------------------------------------------------------------------------------------------
def _finish(rows, n, seed):
    """rows of (tstart, qstart, length, score) -> a shuffled _ffi.HSP array of exactly n unique HSPs"""
    from mimeo_amd import _ffi
    r = np.array(rows, dtype=np.int64).reshape(-1, 4)
    assert r.min() >= 0 and (r[:, :2] + r[:, 2:3]).max() <= TOP and r[:, 2].min() > 0
    h = np.zeros(r.shape[0], dtype=_ffi.HSP)
    h['tstart'], h['qstart'], h['length'], h['score'] = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
    h['raw_score'] = h['score'] + 7
    assert np.unique(r[:, :3], axis=0).shape[0] == h.size == n, (n, h.size)
    return h[np.random.default_rng(seed).permutation(n)]


def run(t0, q0, count, length=50):
    """a collinear run: each HSP starts where the one before ended (`<=` makes it a predecessor)"""
    return [(t0 + i * length, q0 + i * length, length, 90 * length) for i in range(count)]


def stack(t0, qstarts, length, scores):
    """HSPs on consecutive target bases that all start before any of them ends"""
    assert len(qstarts) <= length
    return [(t0 + j, q, length, sc) for j, (q, sc) in enumerate(zip(qstarts, scores))]


def spacers(t0, ends, q0, scores, qstep=10):
    """a stack whose members end at the given (ascending) target positions"""
    assert t0 + len(ends) <= ends[0] and list(ends) == sorted(ends)
    return [(t0 + i, q0 + qstep * i, e - (t0 + i), sc) for i, (e, sc) in enumerate(zip(ends, scores))]


# ---- the families -----------------------------------------------------------------------------------------------------------------
def tiny(name):
    if name == 'n2-chain':
        return _finish(run(1000, 1000, 2), 2, 1)
    if name == 'n2-overlap':
        return _finish([(1000, 1000, 50, 4500), (1010, 3000, 50, 4400)], 2, 2)
    if name == 'n3':
        return _finish([(1000, 1000, 50, 4500), (1050, 1050, 60, 5400), (1020, 5000, 40, 3600)], 3, 3)
    cnt = int(name[4:])                                                # 'tail1', 'tail2', 'tail63': two full tiles, then cnt
    return _finish(run(1000, 1000, 2 * TILE + cnt), 2 * TILE + cnt, cnt)


def pure(k):
    """a run of 128 (two tiles: the tree's content), a stack of k on it, three HSPs behind"""
    rows = run(1000, 1000, 128)                                        # ends at 7400 in both sequences
    rows += stack(8000, [900 + ((j * 37) % 140) * 50 for j in range(k)], 2000, [180000 + (j * 7919) % 1000 for j in range(k)])
    rows += run(12000, 20000, 3)
    return _finish(rows, 128 + k + 3, k)


def window(w, star):
    """A run of 64 (a tile); a pure wave of 64 long HSPs and w spacers; the tile X of 64 whose window the w spacers are: the first j end at
    or before X's first start (`on-the-way`), the others behind it and at or before X's last start.  Spacer scores rise with the end, so
    the best predecessor of a member of X with a high qstart is the spacer that ended last before it starts.  `star` names the member of
    X that gets the bonus: 'onway' = the first, 'window' = the last, ('share', v) = the one whose best predecessor is entry 64 of wavefront
    v's share (the first of its second chunk), ('deep', v) = entry 400 of that share.  Scores are stated here, not 90 per base: the long
    HSPs must not win, the spacers must rank by end."""
    j = 8 if w >= 64 else max(1, w // 2)
    tx = 2064 + w + j + 100
    ends = [tx - (j - 1 - i) for i in range(j)] + [tx + 1 + i for i in range(w - j)]
    span = max(63, w - j)
    starts = {tx + (m * span) // 63 for m in range(TILE)}
    keep = {tx, tx + span}
    per = share_of(w)
    if isinstance(star, tuple):
        o = (star[1] - 1) * per + (64 if star[0] == 'share' else 400)
        assert j <= o < min(w, star[1] * per)
        keep.add(ends[o])
        star_t = ends[o]
    else:
        star_t = tx if star == 'onway' else tx + span
    starts |= keep
    for t in sorted(starts - keep):
        if len(starts) > TILE:
            starts.discard(t)
    starts = sorted(starts)
    assert len(starts) == TILE
    rows = run(1000, 1000, 64, 10)
    rows += stack(2000, [30000 + 7 * i for i in range(64)], 100000, [500] * 64)
    rows += spacers(2064, ends, 3000, [20000 + 1000 * i for i in range(w)])
    xlen = span + 5000
    for m, t in enumerate(starts):
        q = 400000 + 13 * m if (m % 3 != 1 or t == star_t) else 3050 + 10 * ((m * 5) % w)
        rows.append((t, q, xlen, 90 * xlen + m + (10 ** 7 if t == star_t else 0)))
    return _finish(rows, 64 + 64 + w + 64, w)


def window_one():
    """a window of one entry: the group's first tile, one member of which ends before the last one starts"""
    rows = [(1000, 1000, 10, 900)] + [(1000 + 2 * m, 2000 + 700 * ((m * 11) % 63), 500, 45000 + m) for m in range(1, 64)]
    rows += run(2000, 60000, 6)
    return _finish(rows, 70, 1)


def intra(n):
    return _finish(run(1000, 1000, n), n, n)


STRANDS, CLOSERS = 130, 70


def tree_blocks(n):
    """n - 70 HSPs of 10 bases, one every 10 target bases (E = the sorted order, every step a tile), in STRANDS interleaved strands: HSP i
    is piece i // STRANDS of strand i % STRANDS, and the strands lie one behind the other in the query, the last strand first.  A chain
    steps from a strand to the same or a later band, one piece or more onward.  A few strands are heavy (5000 a piece against 900), each
    for its share of the pieces: the one that holds query rank 5, the ones at ranks 1024 and 2048, the topmost.  The best chain follows
    them: its predecessors lie 130 HSPs back (in the tree for sure) and it climbs from block to block of the tree.  Behind them in the
    target 70 closers below every query start: ranks 1 .. 70, so a strand HSP of query rank p asks for 70 + p entries and sits at rank
    71 + p; every prefix 0 .. n - 1 is asked for once, and the closers' tiles put every strand HSP (rank n too) into the tree."""
    ns = n - CLOSERS
    i = np.arange(ns)
    key = (STRANDS - 1 - i % STRANDS) * ns + i // STRANDS
    pi = np.empty(ns, np.int64)
    pi[np.argsort(key)] = i
    sched = []
    for want in (5, 1024 - CLOSERS if 1024 - CLOSERS < ns - 1 else ns // 2, 2048 - CLOSERS, ns - 1):
        if want < ns:
            strand = int(np.flatnonzero(pi == want)[0]) % STRANDS
            if strand not in sched:
                sched.append(strand)
    pieces = -(-ns // STRANDS)
    rows = []
    for k in range(ns):
        heavy = sched[(k // STRANDS) * len(sched) // pieces] == k % STRANDS
        rows.append((1000 + 10 * k, 1000 + 100 * int(pi[k]), 10, 5000 if heavy else 900 + (k * 2654435761 >> 7) % 400))
    rows += [(1000 + 10 * ns + 10 * j, 10 * j, 10, 100) for j in range(CLOSERS)]
    return _finish(rows, n, n)


def cross_ties(member):
    """All scores 3000, all lengths 40.  A stack A of 64 (one tstart, query ends from 2040 up): in the tree when the tile begins.  A wave B of 64 at
    tstart 1100 (query ends up to 990) and B' of 3 at 1110 (query ends up to 540): B ends on the tile's first start (on-the-way), B'
    behind it (window).  The tile: x0, x1 (query ends 140, 190) with no predecessor; ONE member y that sees a chosen mix of them, all
    with chain score 3000; z, which only y precedes among the members.  The best chain is z, y and the EARLIEST of y's tied candidates."""
    rows = [(1000, 2000 + 50 * j, 40, 3000) for j in range(64)]
    rows += [(1100, 600 + 5 * j, 40, 3000) for j in range(64)]
    rows += [(1110, 400 + 50 * j, 40, 3000) for j in range(3)]
    rows += [(1140, 100, 40, 3000), (1141, 150, 40, 3000)]
    rows.append({'all-but-tile': (1150, 9000, 40, 3000),      # A, B, B': tree, on-the-way and window tie; x0 and x1 have not ended
                 'all': (1185, 9000, 40, 3000),               # ... and x0, x1: four sources
                 'window-tile': (1186, 560, 40, 3000),        # B' and x0, x1
                 'tile-tile': (1187, 195, 40, 3000)}[member]) # x0 and x1
    rows.append((1300, 9500, 40, 3000))
    return _finish(rows, 135, len(member))


def equal_ends(n, seed):
    """starts on a lattice of 40 bases, lengths of 40, 80 and 120: a few dozen distinct ends, and most ends are another HSP's start"""
    rng = np.random.default_rng(seed)
    side = int(np.sqrt(n)) + 10
    r = np.stack([rng.integers(0, side, 4 * n) * 40 + 1000, rng.integers(0, side, 4 * n) * 40 + 1000, rng.integers(1, 4, 4 * n) * 40], 1)
    _, first = np.unique(r, axis=0, return_index=True)
    r = r[np.sort(first)[:n]]
    return _finish([(t, q, l, 90 * l + int(x)) for (t, q, l), x in zip(r.tolist(), rng.integers(0, 50, n))], n, seed)


def domain_top(shifted):
    """21 collinear HSPs of 10^8 bases at 100 per base among 200 small ones; shifted: the largest end is TOP"""
    rng = np.random.default_rng(39)
    big = 10 ** 8
    rows = [(1000 + i * big, 1000 + i * big, big, 100 * big) for i in range(21)]
    for t, q, l in zip(rng.integers(0, 21 * big - 1000, 200), rng.integers(0, 21 * big - 1000, 200), rng.integers(30, 400, 200)):
        rows.append((int(t), int(q), int(l), 90 * int(l)))
    d = TOP - (1000 + 21 * big) if shifted else 0
    return _finish([(t + d, q + d, l, s) for t, q, l, s in rows], 221, 39)


# family -> {set name: (generator, arguments)}
FAMILIES = {
    'tiny': {k: (tiny, (k,)) for k in ('n2-chain', 'n2-overlap', 'n3', 'tail1', 'tail2', 'tail63')},
    'pure': {'k%d' % k: (pure, (k,)) for k in (64, 65, 511, 512, 513, 1025)},
    'small-window': dict([('w1', (window_one, ()))] + [('w%d-%s' % (w, s), (window, (w, s))) for w in (2, 7, 8, 9, 56, 57) for s in ('onway', 'window')]),
    'wide-window': dict([('w448', (window, (448, 'window'))), ('w449-share1', (window, (449, ('share', 1)))), ('w449-share6', (window, (449, ('share', 6)))),
                         ('w1000-share2', (window, (1000, ('share', 2)))), ('w1000-share7', (window, (1000, ('share', 7)))),
                         ('w3000-share4', (window, (3000, ('share', 4)))), ('w3000-deep7', (window, (3000, ('deep', 7))))]),
    'intra-tile': {'run%d' % n: (intra, (n,)) for n in (64, 200)},
    'tree-blocks': {'n%d' % n: (tree_blocks, (n,)) for n in (1023, 1024, 1025, 2047, 2049, 4097, 5000)},
    'cross-ties': {k: (cross_ties, (k,)) for k in ('all-but-tile', 'all', 'window-tile', 'tile-tile')},
    'equal-ends': {'n%d' % n: (equal_ends, (n, n)) for n in (600, 1500)},
    'domain-top': {'base': (domain_top, (False,)), 'shifted': (domain_top, (True,))},
}
CASES = [(f, k) for f, sets in FAMILIES.items() for k in sets]


@functools.lru_cache(maxsize=None)
def case(family, name):
    """(the HSPs, their model): made once"""
    gen, args = FAMILIES[family][name]
    h = gen(*args)
    h.setflags(write=False)
    return h, model(h)


# ---- what each family exists for --------------------------------------------------------------------------------------------------
def _chain(m):
    return np.flatnonzero(m.flags)


def check(family, name, m):
    """asserts the property of the family's row over the model's output; returns a line for the test's log"""
    args = FAMILIES[family][name][1]
    on = _chain(m)
    last = m.steps[-1]
    if family == 'tiny':
        assert last.b == m.n and last.b - last.a < TILE            # a short last step: its look-ahead fetch lies beyond n
        if name.startswith('tail'):
            cnt = int(name[4:])
            assert [(t.a, t.b, t.pure) for t in m.steps[:2]] == [(0, 64, False), (64, 128, False)] and len(m.steps) == 3
            assert last.b - last.a == cnt and last.pure == (cnt == 1)   # a lone last member is a wave of one
        else:
            assert len(m.steps) == 1 and last.pure == (name == 'n2-overlap')
        return 'last step %d members, %s' % (last.b - last.a, 'wave' if last.pure else 'tile')
    if family == 'pure':
        k, = args
        w = [t for t in m.steps if t.pure]
        assert len(w) == 1 and w[0].b - w[0].a == k and w[0].a == 128
        assert (w[0].wave_end == w[0].tile_end) == (k == 64)
        kinds = {m.src[i] for i in range(w[0].a, w[0].b)}
        assert kinds == {TREE, NONE}
        assert any(w[0].a <= i < w[0].b and m.src[i] == TREE for i in on)
        assert len({int(m.qcnt[i]) for i in range(w[0].a, w[0].b)}) > 32
        return 'wave of %d, trips of the 512-thread loop %d' % (k, (k + WAVE_THREADS - 1) // WAVE_THREADS)
    if family in ('small-window', 'wide-window'):
        if name == 'w1':
            t = m.steps[0]
            assert not t.pure and t.cend - t.c == 1 and m.epos[0] == 0 and t.ca == 0   # the entry is member 0 of the tile itself
            assert any(m.src[i] == INTILE and m.pred[i] == 0 for i in on)
            return 'first tile, window 1 (a member of the tile)'
        w, star = args
        t = m.steps[2]
        assert len(m.steps) == 3 and m.steps[1].pure and not t.pure and t.b - t.a == TILE and t.b == m.n
        assert t.cend - t.c == w and m.census['widest'] == max(w, 63)   # 63: the run's own tile
        srcs = [m.src[i] for i in range(t.a, t.b)]
        assert ONWAY in srcs and WINDOW in srcs and TREE in srcs
        per = share_of(w)
        assert (per > TILE) == (w > 448)
        sk = [i for i in on if i >= t.a]
        assert len(sk) == 1                                            # the member with the bonus ends the chain
        sk, o = sk[0], int(m.epos[m.pred[sk[0]]]) - t.c
        assert m.src[sk] == (ONWAY if star == 'onway' else WINDOW)
        if isinstance(star, tuple):
            assert o // per == star[1] - 1 and o % per == (64 if star[0] == 'share' else 400)
        return 'window %d, share %d, chain through entry %d of wavefront %d' % (w, per, o % per, o // per + 1)
    if family == 'intra-tile':
        assert all(not t.pure for t in m.steps) and [t.a for t in m.steps] == list(range(0, m.n, TILE))
        assert m.pred.tolist() == list(range(-1, m.n - 1)) and m.flags.all()
        assert all(m.src[k] == (NONE if k == 0 else ONWAY if k % TILE == 0 else INTILE) for k in range(m.n))
        return '%d tiles' % len(m.steps)
    if family == 'tree-blocks':
        n, = args
        assert m.nblk == -(-n // 1024) and (n % 1024 != 0 or n == 1024)
        asked, put = set(m.queries.tolist()), set(m.inserts.tolist())
        assert {q for q in (0, 1023, 1024, 1025, 2047, 2048, n - 1) if q < n} <= asked        # n - 1: the largest a member can ask for
        assert {r for r in (1024, 1025, n) if r <= n} <= put
        assert {int(r - 1) >> BLOCK_SHIFT for r in put} == set(range(m.nblk))
        tr = [(int(m.qcnt[i]) >> BLOCK_SHIFT, int(m.qpos[m.pred[i]] - 1) >> BLOCK_SHIFT) for i in on if m.src[i] == TREE]
        kinds = {m.src[i] for i in on}
        assert len(tr) >= 5 and len(tr) > on.size // 2
        # on the chain: a tree predecessor from a block before the one the prefix ends in, and one from that very block
        assert m.nblk == 1 or any(b < a for a, b in tr), tr
        assert n < 2047 or any(a == b > 0 for a, b in tr), tr
        return 'nblk %d, chain of %d, sources on it %s' % (m.nblk, on.size, sorted(kinds))
    if family == 'cross-ties':
        y = m.n - 2
        want = {'all-but-tile': {TREE: 64, ONWAY: 64, WINDOW: 3}, 'all': {TREE: 64, ONWAY: 64, WINDOW: 3, INTILE: 2},
                'window-tile': {WINDOW: 3, INTILE: 2}, 'tile-tile': {INTILE: 2}}[name]
        assert m.tied[y] == want and m.flags[y] and m.flags[m.n - 1] and on.size == 3
        first = {'all-but-tile': 0, 'all': 0, 'window-tile': 128, 'tile-tile': 131}[name]
        assert m.pred[y] == first == on[0]                             # the earliest of the tied candidates
        return 'ties %s, winner %d' % (want, first)
    if family == 'equal-ends':
        assert np.unique(m.te).size < 80 and np.unique(m.qe).size < 80
        ts, qs = m.sorted['tstart'].astype(np.int64), m.sorted['qstart'].astype(np.int64)
        touch = [i for i in on if m.pred[i] >= 0 and (m.te[m.pred[i]] == ts[i] or m.qe[m.pred[i]] == qs[i])]
        assert len(touch) >= 5                                         # `<=`: a predecessor ends where the HSP starts
        assert m.census['tiles'] > 0
        return '%d target ends, %d on the chain start on their predecessor end' % (np.unique(m.te).size, len(touch))
    if family == 'domain-top':
        assert 1 << 39 > int(m.best.max()) >= 21 * 10 ** 10 > 1 << 37 and on.size >= 21
        assert max(int(m.te.max()), int(m.qe.max())) == (TOP if args[0] else 1000 + 21 * 10 ** 8)
        return 'best chain %d' % int(m.best.max())
    raise AssertionError(family)
