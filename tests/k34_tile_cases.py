"""Designed one-tile sequences for the seed scan (K34, mimeo_amd/csrc/k34_fused.hip) and a plain numpy model of its tiling.

The seed key is (pext12(lo window) << 12) | pext12(hi window) with lo = code & 1 (A, G = 0; C, T = 1) and hi = code >> 1 (A, C = 0;
G, T = 1) over the twelve care positions of the 12of19 seed.  So the TILE of a seed word is the purine / pyrimidine pattern of its
care positions and its key inside the tile is the A-vs-G / C-vs-T choice:

* every seed window inside a stretch of A and G lies in tile 0, every one inside a stretch of C and T in tile 4095;
* a window that straddles a purine stretch and a pyrimidine flank has a pyrimidine at care position 0 or 18: it leaves tile 0.  A purine
  stretch of L bases between pyrimidines puts exactly L - 18 entries into tile 0;
* window i of a stretch takes bit 11 of its key (the half of the key space) from base i + 18, the bases 0 .. 17 are free: the number of
  A among the bases behind the first 18 is the number of entries below key TILE_WORDS / 2 (`mid`);
* a planted 19-mer is one entry under a chosen key (`word_of_key`); poly-A puts all its windows under key 0.

The "quiet" flanks are poly-C on the target side and poly-T on the query side: both in tile 4095, twelve transitions apart, no seed hit
between them (that tile is a tile with thousands of entries on both sides and NOTHING to do); `flip` swaps purines and pyrimidines
(A <-> C, G <-> T: the lo bit), which moves a design from tile t to tile 4095 - t and keeps every in-tile key; `minus` stores the
reverse complement of the query, so that the minus strand of the stored query is the designed one.

`Model` restates, from the source and independent of the C oracle and of the HIP code: the seed-hit total under the 13-probe rule;
per tile nT, nQ, mid and the exact-key sum; and from those a tile's fate, its first-pass segments, its chunks and their kinds in an
aligned tile, the split-pass plan and the probe ranges that reach DENSE_MIN.  tests/test_host_k34_tiles.py holds the model to the
oracle's hit count and every case to the shape it was built for; tests/test_gpu_k34_tiles.py runs the cases on the device."""
import math
import zlib
from collections import namedtuple

import numpy as np

# ---- the constants, stated once (tests/test_host_k34_tiles.py compares them with common.h and k34_fused.hip) ----------------
SEED_LEN, SEED_WEIGHT = 19, 12
CARE = (0, 1, 2, 4, 7, 8, 11, 13, 15, 16, 17, 18)   # 1110100110010101111; care position j is key bit j (pext12)
TILE_WORDS = 4096
NTILE = (1 << 24) // TILE_WORDS
TCH = 64
QSEG_FIRST, QSEG_HEAVY = 1280, 1024
HEAVY_HITS, PART_HITS = 262144, 131072
DENSE_MIN = 48
RING = 128
WAVES = 8                                           # wavefronts of a workgroup of 512: chunk ch belongs to wavefront ch % 8
NOTHING, HERE, LISTED = 'NOTHING', 'HERE', 'LISTED'

_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b'ACGT'):
    _CODE[_c] = _CODE[_c | 0x20] = _i
_FLIP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b'ACGTacgt', b'CATGcatg'):
    _FLIP[_a] = _b
_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b'ACGTacgt', b'TGCAtgca'):
    _COMP[_a] = _b


def _arr(s):
    return np.frombuffer(s, np.uint8) if isinstance(s, (bytes, bytearray)) else np.asarray(s, np.uint8)


def seed_windows(seq, target, minus=0):
    """(positions, 24-bit keys) of the valid seed words of a strand: no base outside ACGT in the 19, and — target role — no lower case"""
    a = _arr(seq)
    code = _CODE[a]
    bad = code > 3
    if target:
        bad = bad | ((a >= 97) & (a <= 122))
    if minus:
        code, bad = np.where(code < 4, 3 - code, 4).astype(np.uint8)[::-1], bad[::-1]
    nw = a.size - SEED_LEN + 1
    if nw <= 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    cs = np.concatenate(([0], np.cumsum(bad)))
    ok = (cs[SEED_LEN:] - cs[:nw]) == 0
    lo, hi = (code & 1).astype(np.int64), (code >> 1).astype(np.int64)
    tile, w = np.zeros(nw, np.int64), np.zeros(nw, np.int64)
    for j, c in enumerate(CARE):
        tile |= lo[c:c + nw] << j
        w |= hi[c:c + nw] << j
    pos = np.flatnonzero(ok)
    return pos, ((tile << 12) | w)[pos]


def probe_key(w, j):
    """probe j of in-tile key w: the key itself, then its transition neighbour of bit j - 1"""
    return w if j == 0 else w ^ (1 << (j - 1))


Plan = namedtuple('Plan', 'est want groups pt need_q qlen pq parts')
Range = namedtuple('Range', 'clipped full own')   # a probe range inside one staged segment, its length in the whole tile, under the entry's own key?


class Model:
    """the seed scan of one (target, query, strand) restated in numpy"""

    def __init__(self, T, Q, strand=0, transitions=1):
        self.transitions = int(transitions)
        self.nn = SEED_WEIGHT + 1 if transitions else 1
        self.tpos, tk = seed_windows(T, True)
        self.qpos, qk = seed_windows(Q, False, strand)
        o = np.argsort(tk, kind='stable'); self.tpos, self.tkey = self.tpos[o], tk[o]      # index order: key, then position
        o = np.argsort(qk, kind='stable'); self.qpos, self.qkey = self.qpos[o], qk[o]
        self.nT = np.bincount(self.tkey >> 12, minlength=NTILE)
        self.nQ = np.bincount(self.qkey >> 12, minlength=NTILE)
        self.mid = np.bincount((self.qkey >> 12)[(self.qkey & 4095) < TILE_WORDS // 2], minlength=NTILE)
        ut, ct = np.unique(self.tkey, return_counts=True)
        uq, cq = np.unique(self.qkey, return_counts=True)

        def q_count(keys):
            if uq.size == 0:
                return np.zeros(keys.size, np.int64)
            i = np.minimum(np.searchsorted(uq, keys), uq.size - 1)
            return np.where(uq[i] == keys, cq[i], 0)

        def per_tile(pairs):
            out = np.zeros(NTILE, np.int64)
            np.add.at(out, ut >> 12, pairs)
            return out
        self.sigma = per_tile(ct * q_count(ut))                                            # exact-key sum of nT(w) nQ(w)
        self.neighbours = sum(per_tile(ct * q_count(ut ^ (1 << j))) for j in range(SEED_WEIGHT))
        self.tile_hits = self.sigma + (self.neighbours if transitions else 0)
        self.hits = int(self.tile_hits.sum())

    # -- one tile ---------------------------------------------------------------------------------------------------
    def tkeys(self, t):
        """the in-tile keys of the tile's target entries, in index order"""
        a, b = np.searchsorted(self.tkey, [t << 12, (t + 1) << 12])
        return self.tkey[a:b] & 4095

    def entries(self, t, side):
        """the scaffold positions of the tile's entries, in index order"""
        key, pos = (self.tkey, self.tpos) if side == 'T' else (self.qkey, self.qpos)
        a, b = np.searchsorted(key, [t << 12, (t + 1) << 12])
        return pos[a:b]

    def qoff(self, t):
        """the tile's TILE_WORDS + 1 query offsets relative to its first entry"""
        a, b = np.searchsorted(self.qkey, [t << 12, (t + 1) << 12])
        return np.concatenate(([0], np.cumsum(np.bincount(self.qkey[a:b] & 4095, minlength=TILE_WORDS))))

    def est(self, t):
        return int(self.sigma[t]) * (SEED_WEIGHT + 1 if self.transitions else 1)

    def fate(self, t):
        """count_prologue"""
        if not self.nT[t] or not self.nQ[t]:
            return NOTHING
        if not self.sigma[t] and not (self.transitions and self.neighbours[t]):
            return NOTHING
        return LISTED if self.est(t) > HEAVY_HITS or self.nQ[t] > 0xFFFF else HERE

    def segments(self, t):
        """first_pass_tile: (aligned, [(qs, qe)])"""
        nq, mid = int(self.nQ[t]), int(self.mid[t])
        if nq <= QSEG_FIRST:
            return False, [(0, nq)]
        if mid <= QSEG_FIRST and nq - mid <= QSEG_FIRST:
            return True, [(0, mid), (mid, nq)]
        return False, [(qs, min(qs + QSEG_FIRST, nq)) for qs in range(0, nq, QSEG_FIRST)]

    def nchunks(self, t):
        return -(-int(self.nT[t]) // TCH)

    def chunk_kinds(self, t):
        """an aligned tile: per segment (= half of the key space) the kind of every chunk — 'half': all its keys lie in the segment's
        half (probes 0 .. 11), 'other': none does (probe 12 alone), 'mixed' (all 13)"""
        k = self.tkeys(t) >> 11
        out = []
        for half in (0, 1):
            kinds = []
            for e0 in range(0, k.size, TCH):
                c = k[e0:e0 + TCH]
                kinds.append('half' if (c == half).all() else 'other' if (c != half).all() else 'mixed')
            out.append(kinds)
        return out

    def first_pass_pairs(self, t):
        """the pairs the first pass enumerates in the tile: every chunk against every segment, the probes jlo .. jhi - 1 in the offsets
        clamped to the segment"""
        keys, qoff = self.tkeys(t), self.qoff(t)
        aligned, segs = self.segments(t)
        n = 0
        for si, (qs, qe) in enumerate(segs):
            co = np.clip(qoff, qs, qe) - qs
            for e0 in range(0, keys.size, TCH):
                k = keys[e0:e0 + TCH]
                jlo, jhi = 0, self.nn
                if aligned:
                    in_half, in_other = ((k >> 11) == si).any(), ((k >> 11) != si).any()
                    if not in_other:
                        jhi = min(self.nn, SEED_WEIGHT)
                    elif not in_half:
                        jlo = SEED_WEIGHT
                for j in range(jlo, jhi):
                    w2 = probe_key(k, j)
                    n += int((co[w2 + 1] - co[w2]).sum())
        return n

    def plan(self, t):
        """k34_plan of a listed tile"""
        nt, nq, est = int(self.nT[t]), int(self.nQ[t]), self.est(t)
        want = min(1 << 20, -(-est // PART_HITS))
        groups = max(1, -(-nt // 512))
        pt = min(groups, max(1, want))
        need_q = max(1, -(-want // pt))
        qlen = max(64, (-(-nq // need_q) + 63) & ~63)
        pq = max(1, -(-nq // qlen))
        return Plan(est, want, groups, pt, need_q, qlen, pq, pt * pq)

    def split_segments(self, t):
        """split_part: the query ranges of the plan, each staged in segments of QSEG_HEAVY"""
        p, nq = self.plan(t), int(self.nQ[t])
        out = []
        for r in range(p.pq):
            qa, qb = r * p.qlen, min((r + 1) * p.qlen, nq)
            out.append([(qs, min(qs + QSEG_HEAVY, qb)) for qs in range(qa, qb, QSEG_HEAVY)])
        return out

    def split_pass_pairs(self, t):
        """(the pairs the split pass enumerates in the tile, the probe ranges of DENSE_MIN - 1 entries and more it meets: Range)"""
        keys, qoff = self.tkeys(t), self.qoff(t)
        uk = np.unique(keys)
        n, ranges = 0, []
        for part in self.split_segments(t):
            for qs, qe in part:
                co = np.clip(qoff, qs, qe) - qs
                for j in range(self.nn):
                    w2 = probe_key(keys, j)
                    n += int((co[w2 + 1] - co[w2]).sum())
                    u2 = probe_key(uk, j)
                    full, clip = qoff[u2 + 1] - qoff[u2], co[u2 + 1] - co[u2]
                    for f, c in zip(full[full >= DENSE_MIN - 1].tolist(), clip[full >= DENSE_MIN - 1].tolist()):
                        if c:
                            ranges.append(Range(c, f, j == 0))
        return n, ranges

    def listed(self):
        return [t for t in np.flatnonzero((self.nT > 0) & (self.nQ > 0)).tolist() if self.fate(t) == LISTED]

    def split_line(self):
        """(tiles listed, parts) as the `[k34] split pass` line states them"""
        ls = self.listed()
        return len(ls), sum(self.plan(t).parts for t in ls)

    def shape(self, t):
        aligned, segs = self.segments(t)
        f = self.fate(t)
        return 'tile %d nT %d nQ %d mid %d sigma %d hits %d %s segments %d%s chunks %d parts %d' % (
            t, self.nT[t], self.nQ[t], self.mid[t], self.sigma[t], self.tile_hits[t], f, len(segs), ' (aligned)' if aligned else '',
            self.nchunks(t), self.plan(t).parts if f == LISTED else 0)


# ---- the builder ------------------------------------------------------------------------------------------------------------
A, G = ord('A'), ord('G')


def rng_of(name):
    return np.random.default_rng(zlib.crc32(name.encode()))


def purines(rng, n):
    return np.where(rng.integers(0, 2, size=n) == 1, G, A).astype(np.uint8)


def block(rng, entries, low):
    """a purine stretch of `entries` seed windows, `low` of them in the lower half of the key space"""
    tail = np.full(entries, G, np.uint8)
    tail[rng.permutation(entries)[:low]] = A
    return np.concatenate((purines(rng, SEED_LEN - 1), tail))


def blocks(rng, entries, low, per=182):
    """purine stretches of up to `per` windows: `entries` windows in all, `low` of them in the lower half"""
    out, done = [], 0
    while done < entries:
        e = min(per, entries - done)
        out.append(block(rng, e, low * (done + e) // entries - low * done // entries))
        done += e
    return out


def poly(base, entries):
    return np.full(entries + SEED_LEN - 1, ord(base), np.uint8)


def word_of_key(k):
    """the purine 19-mer of in-tile key k (A at the seven positions the seed does not look at)"""
    w = np.full(SEED_LEN, A, np.uint8)
    for j, c in enumerate(CARE):
        if (k >> j) & 1:
            w[c] = G
    return w


def lay(items, side, rng=None, lead=40, gap=5, flank='quiet', flush=(False, False)):
    """the items one behind the other between flanks.  quiet: poly-C (target) or poly-T (query), `gap` bases between two items (any 5
    consecutive window positions hold two care positions: no window across a gap lies in a pure tile or meets the other side's);
    random: ACGT drawn from rng.  flush: no flank in front of the first / behind the last item"""
    def fill(n):
        if flank == 'random':
            return np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, size=n)]
        return np.full(n, ord('C' if side == 'T' else 'T'), np.uint8)
    out = [] if flush[0] else [fill(lead)]
    for i, it in enumerate(items):
        if i:
            out.append(fill(gap))
        out.append(_arr(it))
    if not flush[1]:
        out.append(fill(lead))
    return np.concatenate(out)


def flip(seq):
    """purines <-> pyrimidines (A <-> C, G <-> T): tile t -> tile 4095 - t, the in-tile keys stay"""
    return _FLIP[_arr(seq)]


def revcomp(seq):
    return _COMP[_arr(seq)][::-1].copy()


Case = namedtuple('Case', 'family name T Q strand transitions tiles want')
# tiles: the designed tiles (the first one is the one `want` speaks of); want: the shape the case was built for, asserted from the model
# by tests/test_host_k34_tiles.py (check): nT nQ mid sigma est hits fate segments nsegments aligned nchunks kinds plan ranges straddle tpos qpos ...


def _finish(family, name, T, Q, transitions, want, tiles=(0,)):
    """the variants a name's suffix asks for: @4095 = flipped into the last tile, -minus = on the minus strand"""
    strand = 0
    if '@4095' in name:
        T, Q, tiles = flip(T), flip(Q), tuple(NTILE - 1 - t for t in tiles)
    if name.endswith('-minus'):
        Q, strand = revcomp(Q), 1
    return Case(family, name, T, Q, strand, transitions, tiles, want)


def _target_like(rng, qblocks, nT, copy_entries):
    """target stretches with nT windows: the first are copies of the query's first stretches (seed hits and HSPs by construction),
    the rest is its own"""
    out, left = [], nT
    for b in qblocks:
        if left <= 0 or copy_entries <= 0:
            break
        e = min(b.size - (SEED_LEN - 1), left, copy_entries)
        out.append(b[:e + SEED_LEN - 1].copy())
        left -= e; copy_entries -= e
    if left:
        out += blocks(rng, left, left // 2)
    return out


# -- segments (first_pass_tile: the segment cut) ------------------------------------------------------------------------------
_SEGMENTS = {   # name: (nQ, mid, windows per stretch, segments, aligned)
    'q1279': (QSEG_FIRST - 1, 640, 182, [(0, 1279)], False),
    'q1280': (QSEG_FIRST, 640, 182, [(0, 1280)], False),
    'q1281': (QSEG_FIRST + 1, 640, 182, [(0, 640), (640, 1281)], True),
    'aligned-full': (2 * QSEG_FIRST, QSEG_FIRST, 182, [(0, 1280), (1280, 2560)], True),
    'count-cut': (2 * QSEG_FIRST, QSEG_FIRST + 1, 182, [(0, 1280), (1280, 2560)], False),
    'three': (2 * QSEG_FIRST + 1, QSEG_FIRST, 182, [(0, 1280), (1280, 2560), (2560, 2561)], False),
    'mid0': (QSEG_FIRST + 1, 0, 9, [(0, 1280), (1280, 1281)], False),
    'midall': (QSEG_FIRST + 1, QSEG_FIRST + 1, 9, [(0, 1280), (1280, 1281)], False),
    'mid1': (QSEG_FIRST + 1, 1, 9, [(0, 1), (1, 1281)], True),
    'six': (7000, 3500, 182, [(q, min(q + 1280, 7000)) for q in range(0, 7000, 1280)], False),
}


def _segments(name):
    nQ, mid, per, segs, aligned = _SEGMENTS[name.split('@')[0].replace('-minus', '')]
    rng = rng_of('segments/' + name.split('@')[0].replace('-minus', ''))
    qb = blocks(rng, nQ, mid, per)
    tb = _target_like(rng, qb, 700, 364 if per > 9 else 180)
    want = dict(nT=700, nQ=nQ, mid=mid, fate=HERE, segments=segs, aligned=aligned, nchunks=11)
    return _finish('segments', name, lay(tb, 'T'), lay(qb, 'Q'), 1, want)


def _six_random(name):
    """the design of the issue: 40 purine stretches of 200 bases on either side, set in random sequence: six segments by count"""
    rng = rng_of('segments/six-random')
    T = lay(blocks(rng, 40 * 182, 20 * 182), 'T', rng, flank='random', lead=150, gap=150)
    Q = lay(blocks(rng, 40 * 182, 20 * 182), 'Q', rng, flank='random', lead=150, gap=150)
    return _finish('segments', name, T, Q, 1, dict(fate=HERE, nsegments=6, aligned=False))


# -- chunks (chunk_first, chunk_ahead) ----------------------------------------------------------------------------------------
_CHUNK_Q = {'one': (600, 300, 1, False), 'two': (2000, 1000, 2, True), 'three': (2700, 1350, 3, False)}
_CHUNK_T = (1, 63, 64, 65, 512, 513, 576, 577)


def _chunks(name):
    base = name.replace('-minus', '')
    nT, seg = int(base.split('-')[0][1:]), base.split('-')[1]
    nQ, mid, nseg, aligned = _CHUNK_Q[seg]
    rng = rng_of('chunks/' + base)
    qb = blocks(rng, nQ, mid)
    if nT == 1:
        tb = [qb[0][40:40 + SEED_LEN].copy()]
    else:
        tb = _target_like(rng, qb, nT, 182)
    nch = -(-nT // TCH)
    want = dict(nT=nT, nQ=nQ, mid=mid, fate=HERE, nsegments=nseg, aligned=aligned, nchunks=nch,
                idle_waves=max(0, WAVES - nch),                                   # ch_first >= nchunks
                lone_chunk_waves=sum(1 for w in range(WAVES) if w < nch <= w + WAVES),   # nx == ch when further segments follow
                wrap_waves=sum(1 for w in range(WAVES) if w + WAVES < nch))       # the prefetch wraps from the last chunk to the first
    return _finish('chunks', name, lay(tb, 'T'), lay(qb, 'Q'), 1, want)


# -- halves (the jlo / jhi rule of an aligned tile) ---------------------------------------------------------------------------
_HALVES = {'lower': (128, 0), 'upper': (0, 128), 'on-boundary': (128, 100), 'in-chunk': (100, 100)}


def _halves(name):
    kind, tr = name.rsplit('-tr', 1)
    nlow, nup = _HALVES[kind]
    rng = rng_of('halves/' + kind)
    qb = blocks(rng, 2000, 1000)
    words = []
    for k in range(nlow + nup):   # a window of the query with its last base set: it meets that window, or its partner of bit 11
        b = qb[int(rng.integers(0, len(qb)))]
        at = int(rng.integers(0, b.size - SEED_LEN + 1))
        w = b[at:at + SEED_LEN].copy()
        w[SEED_LEN - 1] = A if k < nlow else G
        words.append(w)
    kinds = [[], []]    # the entries are in key order: the lower half's first
    for e0 in range(0, nlow + nup, TCH):
        low, up = e0 < nlow, min(e0 + TCH, nlow + nup) > nlow
        kinds[0].append('mixed' if low and up else 'half' if low else 'other')
        kinds[1].append('mixed' if low and up else 'half' if up else 'other')
    want = dict(nT=nlow + nup, nQ=2000, mid=1000, fate=HERE, aligned=True, segments=[(0, 1000), (1000, 2000)], kinds=kinds)
    return _finish('halves', name, lay(words, 'T'), lay(qb, 'Q'), int(tr), want)


# -- neighbour-only tiles (count_prologue: c2) --------------------------------------------------------------------------------
_NEIGHBOUR = {'one': (5,), 'some': (0, 6, 11), 'twelve': tuple(range(SEED_WEIGHT))}


def _neighbour(name):
    base = name.split('@')[0]
    kind, tr = base.rsplit('-tr', 1)
    rng = rng_of('neighbour/' + kind)
    u = purines(rng, SEED_LEN)
    qw = []
    for j in _NEIGHBOUR[kind]:
        w = u.copy()
        w[CARE[j]] ^= A ^ G
        w[3] ^= A ^ G     # a position the seed does not look at: the windows one base to either side differ in two care positions
        qw.append(w)
    hits = len(qw) if int(tr) else 0
    want = dict(nT=1, nQ=len(qw), sigma=0, hits=hits, fate=HERE if hits else NOTHING)
    return _finish('neighbour', name, lay([u], 'T'), lay(qw, 'Q'), int(tr), want)


# -- listing (count_prologue: the estimate and the 16-bit limit) --------------------------------------------------------------
def _listing_sigma(name):
    sigma, tr = int(name.split('-')[1]), int(name[-1])
    root = math.isqrt(sigma)
    extra = sigma - root * root            # 0 or 1: one more word under another key on both sides
    assert extra in (0, 1)
    t, q = [poly('A', root)], [poly('A', root)]
    if extra:
        t.append(word_of_key(4095)); q.append(word_of_key(4095))
    est = sigma * (13 if tr else 1)
    want = dict(nT=root + extra, nQ=root + extra, sigma=sigma, est=est, fate=LISTED if est > HEAVY_HITS else HERE, nsegments=1)
    return _finish('listing', name, lay(t, 'T'), lay(q, 'Q'), tr, want)


def _listing_nq(name):
    nQ = int(name.split('-')[1])
    rng = rng_of('listing/nq')
    qb = blocks(rng, nQ, nQ // 2, per=nQ)
    tb = [qb[0][1000:1000 + 182 + SEED_LEN - 1].copy()]
    want = dict(nT=182, nQ=nQ, fate=LISTED if nQ > 0xFFFF else HERE, aligned=False, est_below=HEAVY_HITS // 4)
    if nQ > 0xFFFF:
        want['plan'] = dict(want=1, groups=1, pt=1, need_q=1, qlen=65536, pq=1, parts=1)
    else:
        want['nsegments'] = 52
    return _finish('listing', name, lay(tb, 'T'), lay(qb, 'Q'), 1, want)


def _ry_block(rng, n):
    """purine at the even, pyrimidine at the odd positions: its windows lie in two tiles"""
    b = purines(rng, n)
    b[1::2] = np.where(b[1::2] == A, ord('C'), ord('T'))
    return b


RY_TILES = (sum(1 << j for j, c in enumerate(CARE) if c & 1), sum(1 << j for j, c in enumerate(CARE) if not c & 1))


def _listing_two(name):
    """tile 0 listed (poly-A on both sides), tile 4095 listed (a poly-C stretch of the query against the target's poly-C flanks), and a
    shared stretch of alternating purines and pyrimidines whose two tiles are worked in the first pass"""
    rng = rng_of('listing/two')
    ry = _ry_block(rng, 200)
    T = lay([poly('A', 300), ry], 'T', lead=600)
    Q = lay([poly('A', 300), poly('C', 150), ry], 'Q', gap=24)
    want = dict(nT=300, nQ=300, sigma=90000, fate=LISTED, fates={0: LISTED, NTILE - 1: LISTED, RY_TILES[0]: HERE, RY_TILES[1]: HERE}, nlisted=2)
    return _finish('listing', name, T, Q, 1, want, tiles=(0, NTILE - 1) + RY_TILES)


def _listing_blocks(name):
    """the design of the issue: 55 purine stretches of 200 bases on either side, set in random sequence: above HEAVY_HITS"""
    rng = rng_of('listing/blocks-55')
    T = lay(blocks(rng, 55 * 182, 55 * 91), 'T', rng, flank='random', lead=150, gap=150)
    Q = lay(blocks(rng, 55 * 182, 55 * 91), 'Q', rng, flank='random', lead=150, gap=150)
    return _finish('listing', name, T, Q, 1, dict(fate=LISTED))


# -- split pass (split_part, emit_lane_major, emit_dense, k34_plan) -----------------------------------------------------------
def _absent_keys(present, lo, hi, apart):
    """keys of lo .. hi that are not in `present` and more than two bits apart from each other and from those of `apart`"""
    out = []
    for k in range(lo, hi):
        if k not in present and all(bin(k ^ a).count('1') > 2 for a in apart + out):
            out.append(k)
    return out


def _split_dense(name):
    """A listed tile of three query ranges of 1088 (= 1024 + 64: two staged segments in the first two).  Behind the poly-A windows that make it
    heavy and 2800 windows of random purine stretches the query holds, under keys of their own: 47, 48 and 49 copies of three words
    (the target has each word once, and once its neighbour of bit 5: the range is met under the entry's own key and under a transition
    neighbour), and 60 copies of a word whose range lies across entry 1024 (the target has it once): 24 to 47 entries in either
    segment, dense in neither.  The keys are found by a short search over the keys the random stretches leave free."""
    rng = rng_of('split/dense')
    q0 = [poly('A', 150)] + blocks(rng, 2800, 1400)
    keys = np.sort(seed_windows(lay(q0, 'Q'), False)[1])
    keys = keys[keys < TILE_WORDS]                                       # tile 0
    present = set(keys.tolist())
    s_key = None
    for i in range(1024 - 47, 1024 - 13):                                # the 60 copies start at entry i: 13 .. 47 of them before 1024
        if keys[i] - keys[i - 1] > 1:
            s_key, s_at = int(keys[i - 1] + 1), i
            break
    assert s_key is not None
    # the three counted words: far behind the straddling one, each range inside one staged segment (asserted by the host test)
    d = _absent_keys(present, int(keys[2400]), TILE_WORDS, [s_key, 0])[:3]
    assert len(d) == 3
    q = q0 + [word_of_key(s_key)] * 60
    t = [poly('A', 150), word_of_key(s_key)]
    for k, n in zip(d, (DENSE_MIN - 1, DENSE_MIN, DENSE_MIN + 1)):
        q += [word_of_key(k)] * n
        t += [word_of_key(k), word_of_key(k ^ (1 << 5))]
    nQ = 150 + 2800 + 60 + 3 * DENSE_MIN
    want = dict(nT=150 + 1 + 6, nQ=nQ, fate=LISTED, plan=dict(want=3, groups=1, pt=1, need_q=3, qlen=1088, pq=3, parts=3),
                ranges=[(n, own) for n in (DENSE_MIN - 1, DENSE_MIN, DENSE_MIN + 1) for own in (True, False)],
                straddle=(60, 1024 - s_at, s_at + 60 - 1024), short_last_range=True)
    return _finish('split', name, lay(t, 'T'), lay(q, 'Q'), 1, want)


def _split_groups(name):
    nT = int(name.split('-')[1])
    groups = -(-nT // 512)
    want = dict(nT=nT, nQ=100, sigma=nT * 100, fate=LISTED,
                plan=dict(want=6, groups=groups, pt=groups, need_q=6 // groups, qlen=64, pq=2, parts=2 * groups))
    return _finish('split', name, lay([poly('A', nT)], 'T'), lay([poly('A', 100)], 'Q'), 1, want)


def _split_pt_pq(name):
    """two target shares and eleven query ranges of 64 (the floor), the last one of 60"""
    rng = rng_of('split/pt-pq')
    qb = [poly('A', 600)] + blocks(rng, 100, 50)
    tb = [poly('A', 600), qb[1][:60].copy()]
    want = dict(nT=600 + 42, nQ=700, fate=LISTED, plan=dict(want=36, groups=2, pt=2, need_q=18, qlen=64, pq=11, parts=22), short_last_range=True)
    return _finish('split', name, lay(tb, 'T'), lay(qb, 'Q'), 1, want)


# -- ends (stage_segment: bit 1 of sQN; pair_round_split: the target's ends) ---------------------------------------------------
def _ends(name):
    """stretches flush with both ends of both scaffolds: seed starts 0, 1, 2 and len - 20, len - 19.  listed: poly-A (the split pass's
    run test is what looks at the ends), here: copies of random purine stretches.  -n: an N inside the query's first stretch and one
    inside the target's middle stretch (no seed across it; the frames around it are flagged); -softmask: 40 lower-case bases inside
    the target's last stretch (the target loses those seeds, the query's lower case costs nothing)"""
    base = name.replace('-minus', '')
    rng = rng_of('ends/' + base)
    if base.startswith('listed'):
        first, last, midb = poly('A', 182), poly('A', 182), block(rng, 82, 41)
        tq = [[first.copy(), midb.copy(), last.copy()] for _ in range(2)]
    else:
        first, last = block(rng, 150, 75), block(rng, 150, 75)
        tq = [[first.copy(), block(rng, 82, 41), last.copy()] for _ in range(2)]
    t, q = tq
    nT = nQ = sum(b.size - 18 for b in t)
    if base.endswith('-n'):
        q[0][100] = ord('N'); t[1][50] = ord('N')
        nQ -= SEED_LEN; nT -= SEED_LEN
    if base.endswith('-softmask'):
        t[2][80:120] |= 0x20; q[0][30:90] |= 0x20
        nT -= 40 + SEED_LEN - 1
    T, Q = lay(t, 'T', gap=60, flush=(True, True)), lay(q, 'Q', gap=60, flush=(True, True))
    want = dict(nT=nT, nQ=nQ, fate=LISTED if base.startswith('listed') else HERE,
                tpos=[0, 1, 2, T.size - 20, T.size - 19], qpos=[0, 1, 2, Q.size - 20, Q.size - 19])
    return _finish('ends', name, T, Q, 1, want)


_BUILDERS = {}
FAMILIES = {}


def _family(family, fn, names):
    FAMILIES.setdefault(family, []).extend(names)
    for n in names:
        _BUILDERS[family, n] = fn


_family('segments', _segments, [n + s for n in _SEGMENTS for s in ('', '@4095')] + ['aligned-full-minus', 'three@4095-minus'])
_family('segments', _six_random, ['six-random'])
_family('chunks', _chunks, ['t%d-%s' % (n, s) for n in _CHUNK_T for s in _CHUNK_Q] + ['t65-two-minus', 't577-three-minus'])
_family('halves', _halves, ['%s-tr%d' % (k, tr) for k in _HALVES for tr in (1, 0)])
_family('neighbour', _neighbour, ['%s-tr%d' % (k, tr) for k in _NEIGHBOUR for tr in (1, 0)] + ['some-tr1@4095', 'some-tr0@4095'])
_family('listing', _listing_sigma, ['sigma-20164-tr1', 'sigma-20165-tr1', 'sigma-262144-tr0', 'sigma-262145-tr0'])
_family('listing', _listing_nq, ['nq-65535', 'nq-65536'])
_family('listing', _listing_two, ['two-listed-one-here'])
_family('listing', _listing_blocks, ['blocks-55'])
_family('split', _split_dense, ['dense'])
_family('split', _split_groups, ['groups-512', 'groups-513'])
_family('split', _split_pt_pq, ['pt-pq', 'pt-pq@4095'])
_family('ends', _ends, ['listed', 'listed-minus', 'listed-n', 'listed-softmask', 'here', 'here-n', 'here-softmask'])
CASES = [(f, n) for f in FAMILIES for n in FAMILIES[f]]

_cases, _models = {}, {}


def case(family, name):
    if (family, name) not in _cases:
        c = _BUILDERS[family, name](name)
        for a in (c.T, c.Q):
            a.setflags(write=False)
        _cases[family, name] = c
    return _cases[family, name]


def model(family, name):
    if (family, name) not in _models:
        c = case(family, name)
        _models[family, name] = Model(c.T, c.Q, c.strand, c.transitions)
    return _models[family, name]


# -- batches (split_pass: the flush when a part belongs to another unit) ------------------------------------------------------
def batch():
    """Three short scaffolds, all nine pairs and both strands in one call: 18 units.  Scaffolds 0 and 1 hold poly-A stretches and shared
    purine stretches: tile 0 of their four plus-strand units is listed, and pairs are staged in it (two of the four are self units,
    whose main diagonal is not K34's).  Scaffold 2 is random sequence around a stretch of alternating purines and pyrimidines: the
    units with it, and every minus-strand unit (the reverse complement of a purine stretch is a pyrimidine stretch), list nothing.

    The designed tiles are those of several units, and a self unit meets itself in every tile; the family's own figure (90 % of the
    call's hits in tile 0 of the units of scaffolds 0 and 1) is stated and asserted by tests/test_host_k34_tiles.py:
    test_the_batch_family."""
    rng = rng_of('batches')
    shared = blocks(rng, 2 * 182, 182)
    ry = _ry_block(rng, 300)
    rnd = lambda n: np.frombuffer(b'ACGT', np.uint8)[rng.integers(0, 4, size=n)]
    S = [lay([poly('A', 300)] + shared, 'T'), lay([shared[1], poly('A', 200), shared[0][:100]], 'T'), np.concatenate((rnd(1500), ry, rnd(1500)))]
    for a in S:
        a.setflags(write=False)
    return S


BATCH_LISTED_UNITS = [(0, 0, 0), (0, 1, 0), (1, 0, 0), (1, 1, 0)]   # (target, query, strand): tile 0 is listed
