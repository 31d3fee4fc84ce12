"""Designed (target, query) pairs for the gapped stage K6 (rule 7) and a band walk that says which DP kernel
finishes each half extension, and why.

TEST INFRASTRUCTURE.  Every other test of K6 draws its similarity at random, so which of the three DP kernels a half ends in,
and in which row and strip it leaves the one before, is left to chance.  Here every case is ONE pair of scaffolds whose top
anchor and whose two half extensions are known: tests/test_host_k6_edges.py proves from `route` that the families reach the
hand-overs of the cascade, and tests/test_gpu_k6_edges.py holds the engine to the oracle on them.

The walk (`walk`, and `walk_c` = tests/k6_walk.c for long halves) is rule 7 written from its text: row by row, the column
gap as a running maximum of H_k + k E.  It shares no code with the oracle, the engine or tests/spec_v1.py.

`route` restates what decides the way of a half through mimeo_amd/csrc/k6_dp.hip and k6_band.h.  The restatement was checked
against those two files line by line when it was written:
  * shortcut (identical_suffix): the two sequences identical and N-free over n = min(lenA, lenB) bases from the anchor;
  * lean kernel (wave_half_extend_lean): gives up in row 0 iff hi_0 >= 882; in row i iff hi_i // 14 - lo_{i-1} // 14 >= 63 (its
    window starts at the strip of the first live column of the row before); entering row 65 535.  It has NO score cap;
  * 2048-column kernel (wave_half_extend_2048): the same with 32 and 2016, no row limit; after the band test of a row it gives
    up when the best score has passed the cap;
  * k6_dp_any (band_dp): row i has ncols = min(lenB, hi_{i-1} + 1 + ext) - lo_{i-1} + 1 columns, ext = (Y + 200) // E + 2; once
    a row is done and the best score is above the cap, the cells move down by cap // 2.
So a low MIMEO_K6_SCORE_CAP does not move a half that the lean kernel can finish (65 533 or 65 534 rows) to k6_dp_any: it moves
the halves that reach the 2048-column kernel (65 535 rows and more, or a band beyond 882 columns)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
HOXD70 = np.array([[91, -114, -31, -123, -100], [-114, 100, -125, -31, -100], [-31, -125, 100, -114, -100],
                   [-123, -31, -114, 91, -100], [-100, -100, -100, -100, -100]], dtype=np.int64)
CODE = np.full(256, 4, dtype=np.uint8)
for _i, _c in enumerate(b'ACGT'):
    CODE[_c] = _i
    CODE[_c + 32] = _i
BASES = np.frombuffer(b'ACGT', dtype=np.uint8)
COMPLEMENT = np.full(256, ord('N'), dtype=np.uint8)
for _a, _b in zip(b'ACGTacgt', b'TGCAtgca'):
    COMPLEMENT[_a] = _b
DEAD = -(1 << 50)
LIVE = DEAD // 2
CAP = 2_000_000_000
LOW_CAP = 100_000
ROW_LIMIT = 0xFFFF


def revcomp(s):
    return COMPLEMENT[np.frombuffer(bytes(s), dtype=np.uint8)][::-1].tobytes()


# ---------------------------------------------------------------------------------------------- the band walk
class Walk:
    """one half: best = (score, i, j) of the first best cell; lo[i], hi[i] the first / last live column of row i = 0 .. rows;
    bests[i] the best score once row i is done; lenA, lenB what the half had left"""

    def __init__(self, best, lo, hi, bests, lenA, lenB):
        self.best, self.lo, self.hi, self.bests, self.lenA, self.lenB = best, lo, hi, bests, lenA, lenB
        self.rows = len(lo) - 1


def walk(A, B, O=400, E=30, Y=9400, keep=()):
    """rule 7, one side, in numpy.  A, B: base codes (CODE) in walking order.  The Walk also gets `ties`: every live cell (i, j) that
    holds the best score of the rows so far without being the best cell, and `kept`: for the rows listed in `keep`, (first
    column, H, C) of the row before pruning"""
    A, B = np.asarray(A, dtype=np.int64), np.asarray(B, dtype=np.int64)
    lenA, lenB = len(A), len(B)
    hi = min(lenB, (Y - O) // E) if Y >= O + E else 0
    Cp = -O - E * np.arange(hi + 1, dtype=np.int64)
    Cp[0] = 0
    Dp = np.full(hi + 1, DEAD, dtype=np.int64)
    lo = 0
    best = (0, 0, 0)
    los, his, bests, ties, kept = [0], [hi], [0], [], {}
    reach = (Y + 125) // E + 2          # a column gap cannot carry a live cell further: H <= best + 100, I >= best - Y
    for i in range(1, lenA + 1):
        thr = best[0] - Y
        hx = min(lenB, hi + 1 + reach)
        n = hx - lo + 1
        pc = np.full(n, DEAD, dtype=np.int64)
        pd = np.full(n, DEAD, dtype=np.int64)
        pc[:hi - lo + 1] = Cp
        pd[:hi - lo + 1] = Dp
        d = np.maximum(np.where(pd > LIVE, pd - E, DEAD), np.where(pc > LIVE, pc - O - E, DEAD))
        g = np.full(n, DEAD, dtype=np.int64)
        g[1:] = np.where(pc[:-1] > LIVE, pc[:-1] + HOXD70[A[i - 1], B[lo:hx]], DEAD)
        h = np.maximum(g, d)
        k = np.arange(n, dtype=np.int64)
        run = np.maximum.accumulate(np.where(h > LIVE, h + k * E, DEAD))
        ins = np.full(n, DEAD, dtype=np.int64)
        ins[1:] = np.where(run[:-1] > LIVE, run[:-1] - O - k[1:] * E, DEAD)
        c = np.maximum(h, ins)
        alive = (c >= thr) & (c > LIVE)
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        f, l = int(idx[0]), int(idx[-1])
        assert hx == lenB or l < n - 1, 'the walk cut a live row short'
        Cp = np.where(alive, c, DEAD)[f:l + 1]
        Dp = np.where(alive, d, DEAD)[f:l + 1]
        lo, hi = lo + f, lo + l
        if i in keep:
            kept[i] = (lo - f, h.copy(), c.copy())
        m = int(Cp.max())
        if m > best[0]:
            best = (m, i, lo + int(np.argmax(Cp)))
        if m == best[0]:
            ties += [(i, lo + int(x)) for x in np.flatnonzero(Cp == m) if (i, lo + int(x)) != best[1:]]
        los.append(lo)
        his.append(hi)
        bests.append(best[0])
    w = Walk(best, np.array(los, dtype=np.int64), np.array(his, dtype=np.int64), np.array(bests, dtype=np.int64), lenA, lenB)
    w.ties, w.kept = ties, kept
    return w


_lib = None


def _walk_lib():
    """tests/k6_walk.c, built on first use into tests/_build/ like tests/paths_oracle.py builds its own"""
    global _lib
    if _lib is None:
        src, so = os.path.join(HERE, 'k6_walk.c'), os.path.join(HERE, '_build', 'libk6_walk.so')
        if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
            os.makedirs(os.path.dirname(so), exist_ok=True)
            tmp = '%s.%d.tmp' % (so, os.getpid())
            subprocess.check_call([os.environ.get('CC', 'gcc'), '-O2', '-fPIC', '-Wall', '-Wextra', '-std=c11', '-shared', '-o', tmp, src])
            os.replace(tmp, so)
        _lib = C.CDLL(so)
        _lib.k6_walk.restype = C.c_int64
        _lib.k6_walk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_void_p, C.c_void_p]
    return _lib


def walk_c(A, B, O=400, E=30, Y=9400):
    """`walk` by tests/k6_walk.c"""
    A, B = np.ascontiguousarray(A, dtype=np.uint8), np.ascontiguousarray(B, dtype=np.uint8)
    out = np.zeros(3, dtype=np.int64)
    lo, hi, bests = np.zeros(len(A) + 1, np.uint32), np.zeros(len(A) + 1, np.uint32), np.zeros(len(A) + 1, np.int64)
    rows = _walk_lib().k6_walk(A.ctypes.data, len(A), B.ctypes.data, len(B), O, E, Y, out.ctypes.data, lo.ctypes.data, hi.ctypes.data,
                               bests.ctypes.data)
    assert rows >= 0
    rows = int(rows)
    return Walk(tuple(int(x) for x in out), lo[:rows + 1].astype(np.int64), hi[:rows + 1].astype(np.int64), bests[:rows + 1].copy(),
                len(A), len(B))


# ---------------------------------------------------------------------------------------------- the way through the cascade
def _register_kernel(w, strip, limit, row_limit, cap):
    """one of the two register kernels on the walk w: (None, stats) when it finishes the half, else ((reason, row, strip), stats).
    stats: maxcols as the kernel reports it, the largest window slide in strips, whether a strip that entered on the right became live"""
    lo, hi, R = w.lo, w.hi, w.rows
    if hi[0] >= limit:
        return ('row0', 0, int(hi[0]) // strip), None
    base = lo[:-1] // strip                                # window base of row i = 1 .. R, in strips
    rl = hi[1:] // strip - base
    events = []
    over = np.flatnonzero(rl >= 63)
    if over.size:
        events.append((int(over[0]) + 1, 0, 'band', int(rl[over[0]])))
    if row_limit and R >= row_limit - 1 and w.lenA >= row_limit:
        events.append((row_limit, 0, 'rows', 0))
    if cap is not None:
        c = np.flatnonzero(w.bests[1:] > cap)
        if c.size:
            events.append((int(c[0]) + 1, 1, 'cap', 0))   # tested after the band test of the same row
    if events:
        row, _, why, s = min(events)
        return (why, row, s), None
    slide = (lo[1:] // strip - base) if R else np.zeros(0, np.int64)
    return None, dict(maxcols=int((rl.max() + 1) * strip) if R else 0, slide=int(slide.max()) if R else 0,
                      fresh=bool(R and hi.max() >= 64 * strip))


def identical(A, B):
    n = min(len(A), len(B))
    a, b = np.asarray(A[:n]), np.asarray(B[:n])
    return bool(n > 0 and (a == b).all() and (a < 4).all())


def route(w, O=400, E=30, Y=9400, cap=CAP, shortcut=False):
    """which kernel finishes the half of walk w, and what the earlier ones made of it.  dict: kernel ('shortcut', 'lean',
    'wide', 'any'); lean / wide: None or (reason, row, strip) why that kernel gave up ('row0', 'band', 'rows', 'cap'); ncols: the
    widest row of k6_dp_any; slide: the largest window slide of the finishing register kernel, in strips; fresh: a strip that
    came in on the right held a live cell; rebases: how often k6_dp_any moves its cells down; maxcols, rows: what
    MIMEO_K6_STATS reports for the half"""
    r = dict(kernel=None, lean=None, wide=None, ncols=0, slide=0, fresh=False, rebases=0, maxcols=0, rows=w.rows)
    if shortcut:
        r.update(kernel='shortcut', rows=0)
        return r
    lean_ok = E <= (1 << 16) and O <= (1 << 24) and Y <= (1 << 28)
    if lean_ok:
        r['lean'], st = _register_kernel(w, 14, 882, ROW_LIMIT, None)
        if r['lean'] is None:
            r.update(kernel='lean', **st)
            return r
    else:
        r['lean'] = ('penalties', 0, 0)
    r['wide'], st = _register_kernel(w, 32, 2016, 0, cap)
    if r['wide'] is None:
        r.update(kernel='wide', **st)
        return r
    ext = (Y + 200) // E + 2
    r['kernel'] = 'any'
    if w.rows:
        n = min(w.rows + 1, w.lenA)                        # rows that k6_dp_any computes: the live ones and the one that dies
        r['ncols'] = int((np.minimum(w.lenB, w.hi[:n] + 1 + ext) - w.lo[:n] + 1).max())
        r['maxcols'] = int((w.hi[1:] - w.lo[1:] + 1).max())
    s = 0
    for b in np.diff(w.bests):                             # the best score grows by b in a row; above the cap it moves down
        s += int(b)
        if s > cap:
            s -= cap // 2
            r['rebases'] += 1
    return r


# ---------------------------------------------------------------------------------------------- anchors
def best_window(T, Q, ts, qs, length):
    """rule 6: offset of the anchor in an HSP — the centre of its first best 31-column window (numpy, HOXD70)"""
    if length <= 31:
        return length // 2
    t, q = np.frombuffer(T, np.uint8)[ts:ts + length], np.frombuffer(Q, np.uint8)[qs:qs + length]
    cs = np.concatenate([[0], np.cumsum(HOXD70[CODE[t], CODE[q]])])
    return int(np.argmax(cs[31:] - cs[:-31])) + 15


def top_anchor(T, Q, minus=0, **params):
    """(at, aq, hsp) of the first anchor in anchor order (score descending, tstart, qstart, length) among the oracle's chained
    HSPs of the strand; Q as the strand reads (already reverse-complemented for minus)"""
    from oracle import oracle as O
    kw = {k: v for k, v in params.items() if k in ('hspthresh', 'xdrop')}
    # the oracle reverse-complements the query itself for the minus strand
    h = O.ungapped_hsps(T, revcomp(Q) if minus else Q, minus, O.default_params(**kw))
    h = h[(h['flags'] & 1) == 1]
    assert h.size, 'no chained HSP'
    h = h[np.lexsort((h['length'], h['qstart'], h['tstart'], -h['score']))][0]
    off = best_window(T, Q, int(h['tstart']), int(h['qstart']), int(h['length']))
    return int(h['tstart']) + off, int(h['qstart']) + off, h


def halves(T, Q, at, aq):
    """the codes of the (left, right) halves in walking order: ((A, B), (A, B))"""
    t, q = CODE[np.frombuffer(T, np.uint8)], CODE[np.frombuffer(Q, np.uint8)]
    return (t[:at][::-1], q[:aq][::-1]), (t[at:], q[aq:])


class Case:
    """one pair of scaffolds and one strand.  T, Q: bytes as handed to the engine and the oracle; Qs: the designed query, which
    for minus = 1 is the reverse complement of Q, so that the design is found on the minus strand; params: gap_open / gap_extend /
    ydrop; cap: MIMEO_K6_SCORE_CAP or None.  `prepare` finds the anchor of a pair once for all its parameter sets"""

    def __init__(self, name, T, Qs, minus=0, cap=None, **params):
        self.name, self.T, self.Qs, self.minus, self.cap, self.params = name, bytes(T), bytes(Qs), minus, cap, params
        self.Q = revcomp(self.Qs) if minus else self.Qs
        self._an = self._analysis = None

    @property
    def oey(self):
        return self.params.get('gap_open', 400), self.params.get('gap_extend', 30), self.params.get('ydrop', 9400)

    def anchor(self):
        if self._an is None:
            self._an = top_anchor(self.T, self.Qs, self.minus)[:2]
        return self._an

    def analyse(self, use_c=None):
        """(at, aq), the two walks (left, right) and their routes; computed once"""
        if use_c is None and self._analysis is not None:
            return self._analysis
        at, aq = self.anchor()
        O, E, Y = self.oey
        out = []
        for A, B in halves(self.T, self.Qs, at, aq):
            sc = identical(A, B)
            big = len(A) > 600 if use_c is None else use_c      # the numpy walk takes 1 s per 8000 rows
            w = Walk((0, 0, 0), np.zeros(1, np.int64), np.zeros(1, np.int64), np.zeros(1, np.int64), len(A), len(B)) if sc else \
                (walk_c if big else walk)(A, B, O, E, Y)
            if sc:
                n = min(len(A), len(B))
                w.best = (int(np.where((A[:n] == 1) | (A[:n] == 2), 100, 91).sum()), n, n)
            out.append((w, route(w, O, E, Y, self.cap or CAP, shortcut=sc)))
        if use_c is None:
            self._analysis = ((at, aq), out)
        return (at, aq), out

    def expected(self):
        """(tstart, tend, qstart, qend, score) of the top anchor's alignment, query coordinates on the plus strand"""
        (at, aq), ((wl, _), (wr, _)) = self.analyse()
        qs, qe = aq - wl.best[2], aq + wr.best[2]
        if self.minus:
            qs, qe = len(self.Q) - qe, len(self.Q) - qs
        return at - wl.best[1], at + wr.best[1], qs, qe, wl.best[0] + wr.best[0]

    def oracle_kw(self):
        return dict(strand=2 if self.minus else 1, **self.params)


# ---------------------------------------------------------------------------------------------- building blocks
def rand(rng, n):
    return BASES[rng.integers(0, 4, n)].copy()


def substitute(rng, s, rate, keep=()):
    """a copy of s with substitutions at `rate`, none inside the (start, end) ranges of `keep`"""
    s = s.copy()
    m = rng.random(s.size) < rate
    for a, b in keep:
        m[max(0, a):max(0, b)] = False
    idx = np.flatnonzero(m)
    cur = CODE[s[idx]].astype(np.int64)
    s[idx] = BASES[(cur + rng.integers(1, 4, idx.size)) & 3]
    return s


def with_indels(rng, s, indels):
    """s with designed indels [(position in s, n)]: n > 0 inserts n random bases there, n < 0 deletes -n bases"""
    for p, n in sorted(indels, reverse=True):
        s = np.insert(s, p, rand(rng, n)) if n > 0 else np.delete(s, slice(p, p - n))
    return s


def transition(b):
    return {65: 71, 71: 65, 67: 84, 84: 67}[int(b)]


def anchor_site(rng, core, p, mismatch=None, span=None):
    """makes core[p:p + 31] the anchor's window of whatever HSP holds it and returns the columns at which the copy must carry a
    transition.  The window is 31 C / G columns (100 each) between borders of 48 A / T columns (91 each) in which every eighth
    column from the window is a transition; further out every 25th column is one, over span = (first, end) (the anchor's HSP).  So a window that lies
    elsewhere holds a mismatch, and one that overlaps holds A / T columns and, from a shift of 8 on, a transition of the
    border.  mismatch: offset 7 .. 23 of one transition inside the window (so that the half that starts there is no identical
    run): a window that drops it by shifting 8 or more picks up a border transition and eight A / T columns instead."""
    n = core.size
    core[p:p + 31] = np.frombuffer(b'CG', np.uint8)[rng.integers(0, 2, 31)]
    at = np.frombuffer(b'AT', np.uint8)
    a, b = max(0, p - 48), min(n, p + 79)
    core[a:p] = at[rng.integers(0, 2, p - a)]
    core[p + 31:b] = at[rng.integers(0, 2, b - p - 31)]
    tr = [p - 8 * k for k in range(1, 7)] + [p + 30 + 8 * k for k in range(1, 7)]
    lo, hi = span if span else (p - 148, p + 179)
    tr += list(range(p - 48 - 25, lo - 1, -25)) + list(range(p + 78 + 25, hi, 25))
    if mismatch is not None:
        assert 7 <= mismatch <= 23
        tr.append(p + mismatch)
    return [t for t in tr if 0 <= t < n]


def copy_with(core, tr, rng=None, sub=0.0, clean=()):
    """the copy of core: substitutions at rate `sub` outside the `clean` ranges, transitions at the columns tr"""
    mut = substitute(rng, core, sub, keep=clean) if sub else core.copy()
    for t in tr:
        mut[t] = transition(core[t])
    return mut


def joined(*parts):
    return np.concatenate([np.asarray(p, dtype=np.uint8) for p in parts]).tobytes()


_anchor_cache = {}


def prepare(cases, threads=8):
    """finds the anchors of the cases' pairs, each pair once, on a thread pool (the oracle call releases the GIL)"""
    from tests import oracle_pool
    from oracle import oracle as O
    O.lib()
    todo = {}
    for c in cases:
        key = (c.T, c.Qs, c.minus)
        if key not in _anchor_cache and key not in todo:
            todo[key] = c
    for key, an in zip(todo, oracle_pool.run([(lambda c: top_anchor(c.T, c.Qs, c.minus)[:2], c) for c in todo.values()], cap=threads)):
        _anchor_cache[key] = an
    for c in cases:
        c._an = _anchor_cache[(c.T, c.Qs, c.minus)]
    return cases


# ---------------------------------------------------------------------------------------------- family W: window edges
W_SEED = 5


def w_pair():
    """7 kbp at 4 % substitutions, 14 indels of 3 .. 60 bases, random flanks"""
    rng = np.random.default_rng(W_SEED)
    core = rand(rng, 7000)
    mut = substitute(rng, core, 0.04, keep=[(3300, 3700)])
    ind = [(int(p), int(n)) for p, n in zip(rng.integers(200, 6800, 14), rng.choice([-60, -40, -20, -7, -3, 3, 7, 20, 40, 60], 14))
           if not 3200 < p < 3800]
    mutq = with_indels(rng, mut, ind)
    return joined(rand(rng, 500), core, rand(rng, 500)), joined(rand(rng, 300), mutq, rand(rng, 300))


# the W pair's change-overs (left half, right half), found with the walk at steps of 100: lean -> 2048 columns at y-drop 18 300 and
# 21 000, 2048 columns -> k6_dp_any at 45 300 and 47 800; the grid runs 300 to either side of each in steps of 100
W_GRID = ([9400, 13000] + list(range(18000, 18500, 100)) + list(range(20700, 21200, 100)) + [24000, 26830, 26860, 32000]
          + list(range(45000, 45500, 100)) + list(range(47500, 48000, 100)) + [55000, 60850, 60880, 70000])
W_GRID_E = {15: [4700, 10100, 10200, 11500, 11600, 13630, 24400, 24500, 28000, 30640, 33000],
            60: [18800, 31500, 32000, 37000, 37500, 53320, 81000, 81500, 84500, 85000, 121360, 125000]}


def family_w():
    """the W pair over its grid of y-drops; four y-drops also on the minus strand and four under the low cap; the grids at gap
    extension 15 and 60 (the change-overs scale with Y / E)"""
    T, Q = w_pair()
    out = [Case('W-y%d' % y, T, Q, ydrop=y) for y in W_GRID]
    out += [Case('W-y%d-minus' % y, T, Q, minus=1, ydrop=y) for y in (9400, 20900, 45200, 60880)]
    out += [Case('W-y%d-cap' % y, T, Q, cap=LOW_CAP, ydrop=y) for y in (9400, 18300, 26860, 47500)]
    out += [Case('W-e%d-y%d' % (e, y), T, Q, ydrop=y, gap_extend=e) for e, ys in sorted(W_GRID_E.items()) for y in ys]
    return out


# ---------------------------------------------------------------------------------------------- family Q: the query ends inside the window
def end_pair(seed, rem, side, which, far=700, sub=0.06):
    """a homology whose top anchor lies `rem` bases from the end of one scaffold (which = 'q' or 't') on one side ('r' or 'l'),
    the homology running to that end and the other scaffold going on with random bases.  The half that ends there opens with a
    transition, so it is no identical run; between the anchor's site and the end the copy carries substitutions and, when there
    is room, two indels.  far: bases of homology on the other side of the anchor"""
    rng = np.random.default_rng(seed)
    if side == 'l':
        rem += 1                       # the centre of a reversed 31-column window lies one base nearer to the end
    n = far + rem                      # core: [far bases] anchor [rem bases]
    core = rand(rng, n)
    # the anchor's HSP: 420 clean columns before the site and the clean columns after it up to the next indel, so that it
    # outscores every other HSP of the pair, which are shorter and carry the substitutions
    cut = far + (rem // 3 if rem > 400 else rem)
    tr = anchor_site(rng, core, far - 15, mismatch=15 if side == 'r' else 16, span=(far - 420, cut))
    mut = copy_with(core, tr, rng, sub, clean=[(far - 420, cut)])
    ind = [(cut, 9), (far + 2 * rem // 3, -7)] if rem > 400 else []
    if far - 420 >= 60:
        ind += [(far - 420, 5), ((far - 420) // 2, -4)]
    other = with_indels(rng, mut, ind)
    # `core` is the scaffold that ends `rem` after the anchor; `other` goes on
    ends, goes = core, np.concatenate([other, rand(rng, 400)])
    ends = np.concatenate([rand(rng, 300), ends])
    goes = np.concatenate([rand(rng, 450), goes])
    if side == 'l':
        ends, goes = ends[::-1].copy(), goes[::-1].copy()
    return (goes.tobytes(), ends.tobytes()) if which == 'q' else (ends.tobytes(), goes.tobytes())


BEYOND_LEAN_Y = (1 << 28) + 1        # test_gpu_align.BEYOND_LEAN: every half starts at the 2048-column kernel
Q_SMALL = list(range(16, 48))        # every residue mod 14 and mod 32
Q_896 = list(range(880, 914))          # 880 and 881 stay with the lean kernel
Q_2048 = list(range(2014, 2050))


def family_q():
    """lenB of the half that ends at the query's end, 32 consecutive values (every residue mod 14 and mod 32) in three ranges:
    16 .. 47, and 15 and 63 .. 65, at the default y-drop (the lean kernel's EDGE rows); 880 .. 913 at y-drop 30 000, where min(lenB, 986) decides
    row 0 of the lean kernel and the 2048-column kernel takes the rest (`exists`); 2014 .. 2049 at 70 000, where min(lenB, 2320)
    decides row 0 of the 2048-column kernel and hx of k6_dp_any.  Every eighth pair also at the y-drops that send it to the
    other kernels, and with the half on the left; three with the target ending first; some on the minus strand"""
    out = []
    for k, rem in enumerate(Q_SMALL):
        T, Q = end_pair(2000 + k, rem, 'r', 'q', far=500)
        out.append(Case('Q-r%d' % rem, T, Q, minus=1 if k % 8 == 5 else 0))
        if k % 4 == 0:
            out.append(Case('Q-r%d-wide' % rem, T, Q, ydrop=BEYOND_LEAN_Y))
        if k % 8 == 2:
            T, Q = end_pair(2050 + k, rem - 1, 'l', 'q', far=500)
            out.append(Case('Q-l%d' % (rem - 1), T, Q))
            out.append(Case('Q-l%d-wide' % (rem - 1), T, Q, ydrop=BEYOND_LEAN_Y))
        if k % 12 == 0:
            T, Q = end_pair(2100 + k, rem, 'r', 't', far=500)
            out.append(Case('Q-t%d' % rem, T, Q))
    for k, (side, rem) in enumerate((('l', 15), ('r', 63), ('r', 64), ('l', 64), ('r', 65))):   # the smallest left half; two strips of 32
        T, Q = end_pair(2150 + k, rem, side, 'q', far=500)
        out.append(Case('Q-%s%d' % (side, rem), T, Q))
        out.append(Case('Q-%s%d-wide' % (side, rem), T, Q, ydrop=BEYOND_LEAN_Y))
    for k, rem in enumerate(Q_896):
        T, Q = end_pair(2200 + k, rem, 'r', 'q')
        out.append(Case('Q-r%d' % rem, T, Q, ydrop=30000))
        if k < 14:
            out.append(Case('Q-r%d-y9400' % rem, T, Q))
        if k % 8 == 2:
            T, Q = end_pair(2250 + k, rem, 'l', 'q')
            out.append(Case('Q-l%d' % rem, T, Q, ydrop=30000))
    for k, rem in enumerate(Q_2048):
        T, Q = end_pair(2300 + k, rem, 'r', 'q')
        out.append(Case('Q-r%d' % rem, T, Q, ydrop=70000, minus=1 if k % 8 == 5 else 0))
        if k % 8 == 2:
            out.append(Case('Q-r%d-y30000' % rem, T, Q, ydrop=30000))
            out.append(Case('Q-r%d-y9400' % rem, T, Q))
            T, Q = end_pair(2350 + k, rem, 'l', 'q')
            out.append(Case('Q-l%d' % rem, T, Q, ydrop=70000))
    return out


# ---------------------------------------------------------------------------------------------- family R: rows
R_LONG = (65533, 65534, 65535, 65536)
R_SHORT = (15, 16, 31, 32, 33, 63, 64, 65)


def long_pair(seed, rows, side, sub=0.03, insert=None):
    """a near-identical pair whose top anchor lies 600 bases from one end of the homology, the target cut so that the long half has
    `rows` target bases left and the query going on: the half is alive in its last row.  side: 'r' / 'l', the long half.
    insert: (distance from the anchor, n): n random bases inserted in the query there (family S)"""
    rng = np.random.default_rng(seed)
    n = 600 + 66500
    core = rand(rng, n)
    # the anchor's HSP: 4000 clean columns; every other HSP ends at one of the short indels, 2400 columns apart at the most
    tr = anchor_site(rng, core, 600 - 15, mismatch=15, span=(180, 4180))
    mut = copy_with(core, tr, rng, sub, clean=[(180, 4180)])
    ind = [(180, 3), (4180, -2)] + [(6500 + 2400 * k + int(rng.integers(0, 100)), int(rng.choice([-3, -2, -1, 1, 2, 3]))) for k in range(25)]
    if insert:
        ind.append((600 + insert[0], insert[1]))
    other = with_indels(rng, mut, ind)
    t = np.concatenate([rand(rng, 300), core[:600 + rows]])
    q = np.concatenate([rand(rng, 450), other, rand(rng, 300)])
    if side == 'l':
        t, q = t[::-1].copy(), q[::-1].copy()     # the reversed window's centre is the same column: the long half keeps `rows` - 1
    return t.tobytes(), q.tobytes()


def family_r():
    """the four row counts on either side, at the production cap and at the low one; the short target remainders"""
    out = []
    for side in ('r', 'l'):
        for rows in R_LONG:
            T, Q = long_pair(3000, rows + (1 if side == 'l' else 0), side)
            out.append(Case('R-%s%d' % (side, rows), T, Q))
            out.append(Case('R-%s%d-cap' % (side, rows), T, Q, cap=LOW_CAP))
    for k, rem in enumerate(R_SHORT):
        for side in ('l',) if rem < 16 else ('r', 'l') if rem in (32, 64) else ('rl'[k % 2],):
            T, Q = end_pair(3100 + k, rem, side, 't', far=500)
            out.append(Case('R-%s%d' % (side, rem), T, Q, minus=1 if k == 3 else 0))
    return out


# ---------------------------------------------------------------------------------------------- family I: the shortcut
I_N = (16, 31, 32, 33, 2047, 2048, 2049, 4095, 4096, 4097)
I_CHANGES = ('none', 'sub-last', 'sub-first', 'n-last', 'n-both', 'beyond')


def shortcut_pair(seed, n, side, ends, change):
    """two scaffolds identical over n bases from the anchor to the end of the shorter one (ends = 't' or 'q'), the other going on with
    other bases; on the far side of the anchor 500 bases of homology with substitutions.  change: 'sub-last' / 'n-last': a
    substitution / an N in base n - 1; 'sub-first': a substitution in base 0; 'n-both': an N in both at base n - 2 (n - 1 for
    n = 16 on the right would leave the window); 'beyond': a substitution in the longer scaffold just beyond the shorter one's end"""
    rng = np.random.default_rng(seed)
    far = 500
    m = n + (1 if side == 'l' else 0)          # bases of the core from the anchor's column on
    core = rand(rng, far + m)
    # 'sub-first': base 0 of the right half is the window's centre, of the left half (the sequences are reversed below) the column behind it
    tr = anchor_site(rng, core, far - 15, mismatch={'r': 15, 'l': 16}[side] if change == 'sub-first' else None, span=(far - 420, far + m))
    tr = [t for t in tr if t < far - 15 or far - 15 + 7 <= t <= far - 15 + 23]    # the identical run carries no designed transition
    if change == 'sub-first':
        # the window now holds a mismatch (2969); behind its border the run is A / T only, so that no window there reaches 2821
        core[far + 16 + 48:] = np.frombuffer(b'AT', np.uint8)[rng.integers(0, 2, max(0, core.size - far - 64))]
    mut = copy_with(core, tr, rng, 0.05, clean=[(far - 420, far + m)])
    mut = with_indels(rng, mut, [(far - 420, 4)])
    nxt = BASES[(int(CODE[core[-1]]) + 1) & 3]
    shorter = core.copy()
    longer = np.concatenate([mut, np.array([transition(nxt) if change == 'beyond' else nxt], np.uint8), rand(rng, 300)])
    last = far + m - 1
    if change == 'sub-last':
        longer[last + 4] = transition(longer[last + 4])          # `mut` is 4 bases longer than `core` before the clean stretch
    elif change == 'n-last':
        (shorter if seed % 2 else longer)[last + (0 if seed % 2 else 4)] = ord('N')
    elif change == 'n-both':
        shorter[last - 1] = ord('N')
        longer[last - 1 + 4] = ord('N')
    shorter = np.concatenate([rand(rng, 300), shorter])
    longer = np.concatenate([rand(rng, 450), longer])
    if side == 'l':
        shorter, longer = shorter[::-1].copy(), longer[::-1].copy()
    return (shorter.tobytes(), longer.tobytes()) if ends == 't' else (longer.tobytes(), shorter.tobytes())


def family_i():
    """every n with the shortcut taken on one side and, on the other side, one change that defeats it — the four kinds in turn;
    the control for every n whose last word holds 31 bases, and for 16 and 4096"""
    out = []
    for k, n in enumerate(I_N):
        a, b = ('r', 'l') if k % 2 == 0 else ('l', 'r')
        todo = [(a, 'none'), (b, I_CHANGES[1 + k % 4]), (a, I_CHANGES[1 + (k + 2) % 4])]
        if n % 32 == 31 or n in (16, 4096):
            todo.append((b, 'beyond'))
        for c, (side, change) in enumerate(todo):
            T, Q = shortcut_pair(4000 + 16 * k + c, n, side, 'tq'[(k // 2 + c) % 2], change)
            out.append(Case('I-%s%d-%s' % (side, n, change), T, Q, minus=1 if (k + c) % 7 == 3 else 0))
    return out


# ---------------------------------------------------------------------------------------------- family S: window slides
def _site_pair(rng, far, tail_t, tail_q, side):
    """scaffolds around an anchor site: `far` bases of homology (substitutions, one indel) before the site's clean stretch, then
    the given tails (arrays that start right behind the window's border), random flanks; side 'l' reverses both"""
    core = rand(rng, far + 110)
    tr = anchor_site(rng, core, far - 15, span=(far - 420, far + 95))      # the only window of 31 C / G columns: the tails hold none
    mut = copy_with(core, tr, rng, 0.05, clean=[(far - 420, far + 110)])
    if far - 420 >= 40:
        mut = with_indels(rng, mut, [(far - 420, 4)])
    t = np.concatenate([rand(rng, 300), core, tail_t, rand(rng, 300)])
    q = np.concatenate([rand(rng, 450), mut, tail_q, rand(rng, 350)])
    if side == 'l':
        t, q = t[::-1].copy(), q[::-1].copy()
    return t.tobytes(), q.tobytes()


def slide_pair(seed, n, k, side):
    """an insertion of n query bases whose first k repeat the k target bases that follow: the old diagonal goes on for k columns
    beside the new one, then runs into random bases and dies, and the first live column jumps to the new diagonal's fringe.
    Run at y-drop slide_ydrop(n): enough to cross the gap, little more."""
    rng = np.random.default_rng(seed)
    before, after = rand(rng, 150), rand(rng, 500)
    tail_t = np.concatenate([before, after])
    tail_q = np.concatenate([before, after[:k], rand(rng, n - k), after])
    return _site_pair(rng, 500, tail_t, tail_q, side)


def slide_ydrop(n, O=400, E=30):
    return O + n * E + 150


def family_s():
    """slides of two strips and more: insertions of 45 .. 60 bases in short pairs (the lean kernel), of 130 bases in the 66 kbp pair of
    family R, 3000 rows from the anchor, with more than 65 534 rows (the 2048-column kernel)"""
    out = []
    for k, n in enumerate((45, 52, 60)):
        for side in ('r', 'l'):
            T, Q = slide_pair(5000 + k, n, 20, side)
            out.append(Case('S-%s%d' % (side, n), T, Q, ydrop=slide_ydrop(n), minus=1 if (k, side) == (1, 'l') else 0))
    for side in ('r', 'l'):
        T, Q = long_pair(5100, 65600, side, sub=0.02, insert=(3000, 130))
        out.append(Case('S-%s130-rows' % side, T, Q, ydrop=slide_ydrop(130)))
    return out


# ---------------------------------------------------------------------------------------------- family T: ties
def _cg(rng, n):
    return np.frombuffer(b'CG', np.uint8)[rng.integers(0, 2, n)]


def return_pair(seed, side, n_in):
    """behind the last best cell an N column (-100), a C:C column (+100), twelve transversions: two rows on, the score is the best
    score again and no more.  n_in: 'q' / 't', the scaffold that holds the N"""
    rng = np.random.default_rng(seed)
    body = rand(rng, 80)
    body[-1] = ord('G')
    tv = rand(rng, 12)
    tq = np.array([{65: 67, 67: 65, 71: 84, 84: 71}[int(b)] for b in tv], np.uint8)
    x = np.array([ord('A')], np.uint8)
    nn = np.array([ord('N')], np.uint8)
    c = np.array([ord('C')], np.uint8)
    tail_t = np.concatenate([body, nn if n_in == 't' else x, c, tv])
    tail_q = np.concatenate([body, nn if n_in == 'q' else x, c, tq])
    return _site_pair(rng, 400, tail_t, tail_q, side)


T2_GAP, T2_NS, T2_LEN = 260, 41, 100        # 400 + 30 * 260 = 200 * 41: the gap costs what 41 C / G columns against N cost


def row_tie_pair(seed, side, long_query=False):
    """the target ends on a row with two best cells T2_GAP columns apart: the last T2_LEN target bases Z stand in the query
    twice — first with T2_NS of them, every other one from the first on, all C / G, as N, then, T2_GAP columns further on, exactly.  The diagonal through the
    Ns and the gap over them arrive with the same score; the cell in the smaller column is the result.
    long_query: 2300 random bases behind, for y-drop 70 000 to send the half to k6_dp_any"""
    rng = np.random.default_rng(seed)
    P, Z = rand(rng, 100), rand(rng, T2_LEN)
    Z[:2 * T2_NS:2] = _cg(rng, T2_NS)
    Zn = Z.copy()
    Zn[:2 * T2_NS:2] = ord('N')          # every other column: no stretch of them is worth two gaps around it
    tail_t = np.concatenate([P, Z])
    tail_q = np.concatenate([P, Zn, rand(rng, T2_GAP - T2_LEN), Z, rand(rng, 2300 if long_query else 0)])
    core = rand(rng, 400 + 110)
    tr = anchor_site(rng, core, 400 - 15, span=(0, 400 + 95))
    mut = copy_with(core, tr, rng, 0.0)
    t = np.concatenate([rand(rng, 300), core, tail_t])                      # the target ends with Z
    q = np.concatenate([rand(rng, 450), mut, tail_q, rand(rng, 350)])
    if side == 'l':
        t, q = t[::-1].copy(), q[::-1].copy()
    return t.tobytes(), q.tobytes()


def source_tie_pair(seed, side):
    """two sources of one column gap with the same arriving score and other counts: ten C of the target against N N C^10 of the query —
    the diagonal through the two Ns ends two columns left of the path that skips them, 60 = 2 E lower — then 12 query bases to
    skip, then 150 columns of homology that hold the best cell.  The left source (two mismatches more) is the rule's choice"""
    rng = np.random.default_rng(seed)
    P, R = rand(rng, 60), rand(rng, 150)
    P[-1] = ord('A')
    R[0] = ord('T')
    G = rand(rng, 12)
    G[0] = ord('A')
    cs = np.full(10, ord('C'), np.uint8)
    tail_t = np.concatenate([P, cs, R])
    tail_q = np.concatenate([P, np.array([78, 78], np.uint8), cs, G, R])
    return _site_pair(rng, 400, tail_t, tail_q, side)


def family_t():
    out = []
    for k, (side, n_in) in enumerate((('r', 'q'), ('l', 'q'), ('r', 't'), ('l', 't'))):
        T, Q = return_pair(6000 + k, side, n_in)
        out.append(Case('T-return-%s-%s' % (side, n_in), T, Q, minus=1 if k == 3 else 0))
    for k, side in enumerate(('r', 'l')):
        T, Q = row_tie_pair(6100 + k, side)
        out.append(Case('T-rowtie-%s' % side, T, Q))
        T, Q = row_tie_pair(6110 + k, side, long_query=True)
        out.append(Case('T-rowtie-%s-any' % side, T, Q, ydrop=70000))
        T, Q = source_tie_pair(6200 + k, side)
        out.append(Case('T-source-%s' % side, T, Q))
    return out


def dp_waves(w, i, j, threads, O=400, E=30, Y=9400):
    """the wavefront of band_dp (k6_band.h) that holds column j of row i when `threads` threads share the row"""
    ext = (Y + 200) // E + 2
    lo, hi = int(w.lo[i - 1]), int(w.hi[i - 1])
    ncols = min(w.lenB, hi + 1 + ext) - lo + 1
    chunk = (ncols + threads - 1) // threads
    return (j - lo) // chunk // 64


FAMILIES = {'W': family_w, 'Q': family_q, 'R': family_r, 'S': family_s, 'I': family_i, 'T': family_t}
