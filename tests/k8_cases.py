"""The tandem scorer (K8) at its edges: a restatement that returns positions, and designed slices.

TEST INFRASTRUCTURE, beside tests/k5_wave_cases.py.  `mask_by_rule` is written from the DESIGN.md paragraph "Tandem scorer v2" alone:
for every period p = 1 .. maxperiod a local alignment of the slice with itself on the diagonals p - b .. p + b (b = 0 for p = 1, 1 for
p < 5, else 2; delta <= 0: b = 0),

    H[j][d] = max(0, H[j-1][d] + s(S[j], S[j-d]), H[j-1][d-1] - delta, H[j][d+1] - delta)      ties: diagonal, insertion, deletion

and "a path that reaches a new best >= minscore masks everything from the first base of its earlier copy to the base it has reached".
It shares nothing with `oracle.pipeline.tandem_masked` or the kernels: cells are kept per diagonal (a dict d -> cell), every period
begins at the first column that has a cell (j = p - b; there is no 32-aligned start), a cell carries (score, first base of the earlier
copy, best on the path; the end of the path's last marking rides along for the rewrite `mark_from_mend` alone), and the result is the
mask, not its sum.  `mutant=` turns ONE rule wrong (MUTANTS) or rewrites
one in an equivalent way (REWRITES); it exists for the host proof in tests/test_host_k8_edges.py that the designed slices tell the
rules apart, and no GPU test passes it.

A case is (scaffolds, slice list, (match, mismatch, minscore, maxperiod, delta)) at the smallest shape that still holds its edge; `hand`
gives, per slice, the answer worked out by hand where there is one ('none', 'all' or the positions).  tests/test_host_k8_edges.py
proves on the CPU that every case reaches its edge and that the hand answers are the restatement's; tests/test_gpu_k8_edges.py holds
`engine.tandem_mask` to the restatement bit for bit."""
import functools
from types import SimpleNamespace

import numpy as np

ACGT = np.frombuffer(b'ACGT', np.uint8)
DEFAULT = (2, 7, 50, 50, 7)       # match, mismatch, minscore, maxperiod, delta: TRF's `2 7 7 80 10 50 50`
OPEN_END = 0xFFFFFFFF
COST_CAP = 1.5e6                  # per test: sum over the slices of length * maxperiod (keeps the restatement cheap; no measurement)
BLOCK = 64                        # periods per wavefront of the wide kernel (host_plan::TANDEM_BLOCK)

# wrong rules: each must change the mask of a designed slice (KILLERS)
MUTANTS = ('ins_tie_ge', 'del_tie_ge', 'del_from_prev_column', 'best_on_ge', 'gt_minscore', 'mask_ends_at_j', 'band_p_le_5',
           'band_p_lt_4', 'non_acgt_match')
# rewrites that cannot change a mask (tests/test_host_k8_edges.py says why)
REWRITES = ('carry_best_across_reset', 'mark_from_mend')


# ---- the restatement ----------------------------------------------------------------------------------------------------------------
def half_band(p, delta, mutant=None):
    if delta <= 0 or p == 1:
        return 0
    lim = {'band_p_le_5': 6, 'band_p_lt_4': 4}.get(mutant, 5)
    return 1 if p < lim else 2


def _mask_by_rule(s, match, mismatch, minscore, maxperiod, delta, mutant):
    L = len(s)
    mask = np.zeros(L, dtype=bool)
    if mutant == 'non_acgt_match':
        code = list(s)
    else:
        code = [c if c in b'ACGT' else -1 - i for i, c in enumerate(s)]     # a letter outside ACGT equals nothing, itself included
    ins_ge, del_ge, del_prev = mutant == 'ins_tie_ge', mutant == 'del_tie_ge', mutant == 'del_from_prev_column'
    best_ge, gt_min, end_j = mutant == 'best_on_ge', mutant == 'gt_minscore', mutant == 'mask_ends_at_j'
    carry, from_mend = mutant == 'carry_best_across_reset', mutant == 'mark_from_mend'
    zero = (0, 0, 0, 0)                                                     # score, first base of the earlier copy, best, [mend]
    for p in range(1, maxperiod + 1):
        b = half_band(p, delta, mutant)
        lo, hi = p - b, p + b
        prev = {d: zero for d in range(lo, hi + 1)}
        for j in range(lo, L):                                              # a column j < lo has no cell: S[j - d] is not in the slice
            cur = {}
            cj = code[j]
            for d in range(hi, lo - 1, -1):
                if j < d:
                    cur[d] = zero
                    continue
                h, st, best, mend = prev[d]
                sc = match if cj == code[j - d] else -mismatch
                if h > 0:
                    h += sc
                else:                                                       # a fresh path: its earlier copy begins at j - d
                    h, st, best, mend = sc, j - d, (best if carry else 0), 0
                if d > lo:                                                  # insertion: from (j - 1, d - 1)
                    q = prev[d - 1]
                    if q[0] - delta > h or (ins_ge and q[0] - delta == h):
                        h, st, best, mend = q[0] - delta, q[1], q[2], q[3]
                if d < hi:                                                  # deletion: from (j, d + 1)
                    q = prev[d + 1] if del_prev else cur[d + 1]
                    if q[0] - delta > h or (del_ge and q[0] - delta == h):
                        h, st, best, mend = q[0] - delta, q[1], q[2], q[3]
                if h <= 0:
                    cur[d] = zero
                    continue
                if h > best or (best_ge and h == best):
                    best = h
                    if h > minscore or (h == minscore and not gt_min):
                        mask[(max(mend, st) if from_mend else st):(j if end_j else j + 1)] = True
                        mend = j + 1
                cur[d] = (h, st, best, mend)
            prev = cur
    return mask


_memo = {}


def mask_by_rule(seq, match=2, mismatch=7, minscore=50, maxperiod=50, delta=7, mutant=None):
    """The marked positions of the slice `seq` (bytes; lower case counts as upper case) as a bool array; memoised, read-only."""
    s = bytes(seq).upper()
    key = (s, match, mismatch, minscore, maxperiod, delta, mutant)
    if key not in _memo:
        m = _mask_by_rule(s, match, mismatch, minscore, maxperiod, delta, mutant)
        m.setflags(write=False)
        _memo[key] = m
    return _memo[key]


# ---- cases --------------------------------------------------------------------------------------------------------------------------
def rnd(rng, n):
    return ACGT[rng.integers(0, 4, n)].tobytes()


def tile(unit, n):
    return (unit * (n // len(unit) + 1))[:n]


def make(seqs, iv, params, hand=None, **info):
    hand = list(hand) if hand is not None else [None] * len(iv)
    assert len(hand) == len(iv)
    return SimpleNamespace(seqs=[bytes(s) for s in seqs], iv=[tuple(int(x) for x in v) for v in iv], params=tuple(params), hand=hand,
                           **info)


def clipped(c, k):
    """the bases of slice k, clipped to its scaffold; b'' for an empty or inverted slice"""
    ch, s, e = c.iv[k]
    e = min(e, len(c.seqs[ch]))
    return c.seqs[ch][s:e] if s < e else b''


def expected(c, mutant=None):
    return [mask_by_rule(clipped(c, k), *c.params, mutant=mutant) for k in range(len(c.iv))]


def cost(c):
    return sum(len(clipped(c, k)) for k in range(len(c.iv))) * c.params[3]


def hand_mask(c, k):
    """the hand-derived answer of slice k as a bool array, or None"""
    h, n = c.hand[k], len(clipped(c, k))
    if h is None:
        return None
    if isinstance(h, str):
        return np.full(n, h == 'all')
    m = np.zeros(n, dtype=bool)
    m[np.asarray(h, dtype=np.int64)] = True
    return m


def first_diagonal(block, delta):
    """host_plan::tandem_block_first_diagonal: a (slice, block) job is listed when this lies below the slice length"""
    return 1 if block == 0 else block * BLOCK + 1 - (2 if delta > 0 else 0)


# threshold: exact copies of a unit of p bases; p + 24 bases hold 24 matches at distance p (48 < 50), p + 25 hold 25 (50): the path
# begins at base 0 of the slice and has reached its last base
def _unit(rng, p):
    if p <= 5:
        return b'ACGTT'[:p] if p != 4 else b'ACGT'
    return rnd(rng, p)


def _threshold(periods, maxperiod, delta, seed):
    rng = np.random.default_rng(seed)
    seq, iv, hand, at = b'', [], [], {}
    for p in periods:
        seq += rnd(rng, 3)
        a = len(seq)
        seq += tile(_unit(rng, p), p + 25)
        iv += [(0, a, a + p + 24), (0, a, a + p + 25)]
        hand += ['none', 'all']
        at[p] = a
    return make([seq + rnd(rng, 3)], iv, (2, 7, 50, maxperiod, delta), hand, periods=tuple(periods), at=at)


def _threshold_cut(p, maxperiod, delta, full):
    """the p + 25 slice with maxperiod at the last value that still sees diagonal p (full) or one below it"""
    rng = np.random.default_rng(800 + p)
    seq = rnd(rng, 5) + tile(rnd(rng, p), p + 25)
    return make([seq], [(0, 5, 5 + p + 25)], (2, 7, 50, maxperiod, delta), ['all' if full else 'none'], periods=(p,))


def _threshold_family():
    f = {}
    for delta in (7, 0):
        f['to64_delta%d' % delta] = functools.partial(_threshold, (1, 2, 4, 5, 31, 32, 33, 50, 63, 64), 64, delta, 801)
        f['to130_delta%d' % delta] = functools.partial(_threshold, (65, 66, 127, 128, 129, 130), 130, delta, 802)
    f['homopolymer'] = lambda: make([b'C' + b'A' * 26 + b'C'], [(0, 1, 26), (0, 1, 27)], DEFAULT, ['none', 'all'], periods=(1,))
    for p in (20, 64, 66, 68):     # 68 at maxperiod 66: period 66 is lane 1 of the second block, diagonal 68 is lane 3's (beyond maxperiod)
        f['p%d_delta7_maxperiod_p-2' % p] = functools.partial(_threshold_cut, p, p - 2, 7, True)
        f['p%d_delta7_maxperiod_p-3' % p] = functools.partial(_threshold_cut, p, p - 3, 7, False)
        f['p%d_delta0_maxperiod_p' % p] = functools.partial(_threshold_cut, p, p, 0, True)
        f['p%d_delta0_maxperiod_p-1' % p] = functools.partial(_threshold_cut, p, p - 1, 0, False)
    return f


# placement: flank, G, (AC) array, G, flank: the mask is exactly the array, wherever it lies in the slice's words
def _placement(bit, length, seed, minscore=50, back=40):
    rng = np.random.default_rng(seed)
    left = rnd(rng, 70) + b'G'
    seq = left + tile(b'AC', length) + b'G' + rnd(rng, 70)
    a = len(left)
    iv = [(0, a - bit, a + length + back)]
    return make([seq], iv, (2, 7, minscore, 8, 7), [list(range(bit, bit + length))], bit=bit, length=length, array=(a, a + length))


def _placement_family():
    f = {}
    for bit, seed in ((31, 810), (32, 811), (33, 813), (63, 814), (64, 815)):
        f['starts_at_bit_%d' % bit] = functools.partial(_placement, bit, 80, seed)
    for i, length in enumerate((63, 64, 65)):
        f['ends_at_bit_%d' % (32 + length)] = functools.partial(_placement, 32, length, 820 + i)
    f['one_word_minscore_50'] = functools.partial(_placement, 32, 32, 830)
    f['one_word_minscore_30'] = functools.partial(_placement, 32, 32, 833, minscore=30)
    f['last_word_of_the_slice'] = functools.partial(_placement, 64, 32, 832, back=0)   # the slice ends with the array, on a word boundary
    return f


# neighbours: fully masked slices of 32, 64, 96 bases beside slices that must stay all zero, in lists that fill a workgroup of four
# wavefronts or leave it part-full
def _neighbour_scaffolds():
    rng = np.random.default_rng(840)
    s0 = rnd(rng, 64) + tile(b'AC', 128) + rnd(rng, 64)        # array at 64 .. 192
    s1 = rnd(rng, 70) + tile(b'AAG', 96)                       # array at 70 .. 166 = the scaffold's end
    return [s0, s1]


def _neighbours(n, maxperiod, delta=7):
    seqs = _neighbour_scaffolds()
    full = {32: (0, 64, 96), 64: (0, 96, 160), 96: (0, 64, 160)}
    zero = {1: (0, 10, 11), 31: (0, 200, 231), 32: (0, 20, 52), 33: (0, 222, 255)}
    lists = {1: [(full[32], 'all')],
             3: [(zero[1], 'none'), (full[64], 'all'), (zero[31], 'none')],
             4: [(full[32], 'all'), (zero[32], 'none'), (full[96], 'all'), (zero[33], 'none')],
             5: [(zero[33], 'none'), (full[96], 'all'), ((0, 100, 100), 'none'), (full[32], 'all'), ((0, 150, 90), 'none')],
             9: [(full[64], 'all'), (zero[1], 'none'), (full[64], 'all'), (zero[31], 'none'), ((1, 166 - 64, 166 + 100), 'all'),
                 ((1, 5, 37), 'none'), ((1, 166 - 32, OPEN_END), 'all'), (zero[33], 'none'), (full[32], 'all'),]}
    iv, hand = zip(*lists[n])
    return make(seqs, iv, (2, 7, 50, maxperiod, delta), hand)


def _neighbours_family():
    f = {}
    for n in (1, 3, 4, 5, 9):
        f['%d_slices' % n] = functools.partial(_neighbours, n, 8)
    for n in (5, 9):
        f['%d_slices_maxperiod_130' % n] = functools.partial(_neighbours, n, 130)
    f['9_slices_gap_free'] = functools.partial(_neighbours, 9, 8, 0)
    return f


# inside: a slice that begins inside an exact array of ACGTT; the copies in front of it do not count: 29 bases hold 24 matches, 30 hold 25
INSIDE_OFFSETS = (0, 1, 4, 5, 31, 32, 33)


def _inside(maxperiod, delta):
    rng = np.random.default_rng(850)
    s0 = tile(b'ACGTT', 100) + rnd(rng, 30) + tile(b'ACGTT', 40)
    s1 = tile(b'CGTTA', 50)
    iv = []
    for o in INSIDE_OFFSETS:
        iv += [(0, o, o + 29), (0, o, o + 30)]
    iv += [(1, 0, 29), (1, 0, 30), (1, 21, 50), (1, 20, 50), (0, 141, 170), (0, 140, 170), (0, 140, OPEN_END)]
    hand = ['none', 'all'] * (len(iv) // 2) + ['all']
    return make([s0, s1], iv, (2, 7, 50, maxperiod, delta), hand)


def _inside_family():
    return {'maxperiod_12': functools.partial(_inside, 12, 7), 'maxperiod_12_gap_free': functools.partial(_inside, 12, 0),
            'maxperiod_66': functools.partial(_inside, 66, 7)}


# letters: a letter outside ACGT matches nothing (a run of N is no homopolymer); lower case is the base
def _letters():
    rng = np.random.default_rng(860)
    arr = tile(b'AC', 120)
    with_n = arr[:30] + b'N' * 6 + arr[36:]
    flank = rnd(rng, 40)
    lower = flank[:30] + flank[30:].lower() + arr[:20].lower() + arr[20:] + rnd(rng, 20)
    parts = [b'N' * 40, b'R' * 40, b'a' * 26, b'aA' * 13, with_n, lower, lower.upper()]
    seq, iv = b'', []
    for x in parts:
        seq += b'G'
        iv.append((0, len(seq), len(seq) + len(x)))
        seq += x
    n_run = list(range(30)) + list(range(36, 120))     # 28 matches in front of the run; behind it a fresh path whose earlier copy begins at 36
    return make([seq + b'G'], iv, (2, 7, 50, 8, 7), ['none', 'none', 'all', 'all', n_run, None, None], lower=(5, 6))


# long: more than 64 mask words, so k8_tandem_count's lanes take a second trip
def _long(delta):
    seq = b'G' + b'T' * 2080 + b'G'
    return make([seq], [(0, 1, 1 + n) for n in (2048, 2049, 2080)], (2, 7, 50, 2, delta), ['all'] * 3)


# pairs: minscore 2, gap-free, periods 1 .. 3: every equal pair (j - d, j) marks [j - d, j], the densest marking a slice can get
def pair_union(s, maxd=3):
    m = np.zeros(len(s), dtype=bool)
    for d in range(1, maxd + 1):
        for j in range(d, len(s)):
            if s[j] == s[j - d]:
                m[j - d:j + 1] = True
    return m


def _pairs(seed):
    rng = np.random.default_rng(seed)
    seq = rnd(rng, 7) + rnd(rng, 40) + rnd(rng, 7)
    return make([seq], [(0, 7, 47)], (2, 7, 2, 3, 0), [np.flatnonzero(pair_union(seq[7:47])).tolist()])


# band and ties: arrays of about 180 bases with substitutions and indels, four parameter sets; chosen by search so that every wrong
# rule of MUTANTS changes a mask here (KILLERS)
TIE_PARAMS = ((2, 7, 50, 16, 7), (2, 5, 30, 12, 3), (2, 2, 12, 8, 2), (3, 7, 20, 10, 1))
TIE_UNITS = (2, 3, 4, 5, 6, 9, 20)


def noisy_array(seed, unit, n=180, sub=0.05, indel=0.08):
    rng = np.random.default_rng(seed)
    out = bytearray()
    for c in tile(rnd(rng, unit), n):
        r = rng.random()
        if r < indel / 2:
            continue
        if r < indel:
            out.append(int(ACGT[rng.integers(0, 4)]))
        if rng.random() < sub:
            c = int(ACGT[rng.integers(0, 4)])
        out.append(c)
    return bytes(out)


def placed_indel(seed, unit, g, n=180):
    """an exact array with one insertion (g > 0) or deletion (g < 0) of |g| bases in its middle"""
    rng = np.random.default_rng(seed)
    a = tile(rnd(rng, unit), n)
    return a[:n // 2] + (rnd(rng, g) if g > 0 else b'') + a[n // 2 + max(0, -g):]


def _ties(kind, seed, unit, arg, pset):
    rng = np.random.default_rng(seed + 7)
    arr = noisy_array(seed, unit) if kind == 'noisy' else placed_indel(seed, unit, arg)
    seq = rnd(rng, 10) + arr + rnd(rng, 10)
    return make([seq], [(0, 10, 10 + len(arr))], TIE_PARAMS[pset], unit=unit, kind=kind)


# noisy arrays (seed, unit, parameter set): four per unit, and those a search over the seeds 1000 .. 1011 found to tell the rare rules apart
TIE_NOISY = ((1000, 2, 0), (1001, 2, 1), (1002, 2, 2), (1003, 2, 3), (1008, 2, 0), (1000, 3, 1), (1001, 3, 2), (1002, 3, 3), (1003, 3, 0),
             (1004, 3, 0), (1009, 3, 2), (1000, 4, 1), (1000, 4, 2), (1001, 4, 3), (1002, 4, 0), (1003, 4, 0), (1003, 4, 1), (1007, 4, 1),
             (1011, 4, 0), (1000, 5, 3), (1001, 5, 0), (1002, 5, 1), (1003, 5, 2), (1009, 5, 2), (1000, 6, 0), (1001, 6, 1), (1002, 6, 2),
             (1003, 6, 3), (1006, 6, 2), (1000, 9, 1), (1001, 9, 2), (1002, 9, 3), (1003, 9, 0), (1008, 9, 0), (1000, 20, 2), (1001, 20, 2),
             (1001, 20, 3), (1002, 20, 0), (1002, 20, 2), (1003, 20, 1), (1004, 20, 2), (1005, 20, 2), (1006, 20, 2), (1008, 20, 2))
TIE_PLACED = (1, -2, 3, -1, 2, -3)     # every unit with each of these, the parameter sets in turn


def _ties_family():
    f = {}
    for seed, unit, pset in TIE_NOISY:
        f['noisy_unit%d_seed%d_params%d' % (unit, seed, pset)] = functools.partial(_ties, 'noisy', seed, unit, None, pset)
    for i, unit in enumerate(TIE_UNITS):
        for j, g in enumerate(TIE_PLACED):
            f['placed_unit%d_indel%+d_params%d' % (unit, g, (i + j) % 4)] = functools.partial(_ties, 'placed', 1100 + unit, unit, g, (i + j) % 4)
    return f


# wide: periods beyond 64.  One placed indel moves the path from diagonal u to u + g, and (maxperiod, u, g) are chosen so that only the
# top periods hold both diagonals and one of the two is fetched by the lanes 0 .. 3 for the whole block (63, 64, 129, 130 for the block
# 65 .. 128; 127, 128 for the block 129 .. 192)
WIDE_INDELS = ((65, 63, 4), (65, 67, -4), (65, 64, 3), (65, 66, -3), (65, 62, 3), (65, 65, 2),
               (66, 64, 4), (66, 67, -3), (66, 63, 3), (66, 62, 4), (66, 65, 3), (66, 66, 2),
               (67, 65, 4), (67, 67, 2), (67, 66, 3), (67, 64, 3), (67, 63, 4), (67, 62, 4),
               (127, 126, 3), (127, 129, -4), (127, 127, 2), (127, 128, -3), (127, 126, 2), (127, 129, -3),
               (130, 126, 4), (130, 127, 4), (130, 128, 4), (130, 131, -4), (130, 129, 3), (130, 130, 2))
FETCHED = {1: (63, 64, 129, 130), 2: (127, 128, 193, 194)}   # block -> the diagonals its lanes 0 .. 3 load for everyone


WIDE_HALF = 22   # matches on either side of the indel: 44 points each, so neither side reaches 50 alone and 88 - 7 |g| does


def wide_array(seed, u, g):
    """u + 22 bases of an exact array of unit u, the indel, 22 more: 22 matches on diagonal u, then 22 on u + g; only a path that
    takes the indel moves reaches minscore, and it marks the whole slice"""
    rng = np.random.default_rng(seed)
    a = tile(rnd(rng, u), u + 2 * WIDE_HALF + max(0, -g))
    x = u + WIDE_HALF
    return a[:x] + (rnd(rng, g) if g > 0 else b'') + a[x + max(0, -g):]


def _wide_indels(maxperiod, delta=7):
    seq, iv, info = b'', [], []
    for i, (mp, u, g) in enumerate(WIDE_INDELS):
        if mp != maxperiod:
            continue
        rng = np.random.default_rng(870 + i)
        seq += rnd(rng, 9)
        a = wide_array(900 + i, u, g)
        iv.append((0, len(seq), len(seq) + len(a)))
        info.append((u, g))
        seq += a
    return make([seq], iv, (2, 7, 50, maxperiod, delta), ['all'] * len(iv) if delta > 0 else None, indels=info)


def _wide_scaffold():
    rng = np.random.default_rng(880)
    return rnd(rng, 100) + tile(b'AC', 100) + rnd(rng, 100) + wide_array(881, 64, 3) + rnd(rng, 20)


def _wide_job_edge(delta):
    """slices of 63 .. 66 bases at maxperiod 130: first_diagonal(1, delta) = 63 (indel moves on) or 65 (off) lies below the length,
    or does not, so the second block's job is listed or left out"""
    seq = _wide_scaffold()
    iv, hand = [], []
    for n in (63, 64, 65, 66):
        iv += [(0, 100, 100 + n), (0, 10, 10 + n), (0, 300, 300 + n)]     # inside the AC array; random; the start of the 64-base unit's array
        hand += ['all', None, None]
    return make([seq], iv, (2, 7, 50, 130, delta), hand)


def _wide_shuffled():
    seq = _wide_scaffold()
    base = _wide_job_edge(7).iv
    rng = np.random.default_rng(882)
    short = [(0, int(a), int(a) + int(n)) for a, n in zip(rng.integers(0, 280, 12), rng.integers(1, 40, 12))]
    iv = base + short + [(0, 300, 300 + 64 + 3 + 2 * WIDE_HALF), (0, 300, OPEN_END), (0, 50, 50)]
    iv = [iv[i] for i in rng.permutation(len(iv))]
    return make([seq, seq[300:]], iv + [(1, 0, 127), (1, 0, 66)], (2, 7, 50, 130, 7))


def _wide_family():
    f = {'indels_maxperiod_%d' % mp: functools.partial(_wide_indels, mp) for mp in (65, 66, 67, 127, 130)}
    f['indels_maxperiod_65_gap_free'] = functools.partial(_wide_indels, 65, 0)
    f['job_edge_delta7'] = functools.partial(_wide_job_edge, 7)
    f['job_edge_delta0'] = functools.partial(_wide_job_edge, 0)
    f['shuffled'] = _wide_shuffled
    return f


def _families():
    return {
        'threshold': _threshold_family(),
        'placement': _placement_family(),
        'neighbours': _neighbours_family(),
        'inside': _inside_family(),
        'letters': {'letters': _letters},
        'long': {'delta7': functools.partial(_long, 7), 'gap_free': functools.partial(_long, 0)},
        'pairs': {'seed%d' % s: functools.partial(_pairs, s) for s in (890, 891, 892)},
        'band_and_ties': _ties_family(),
        'wide': _wide_family(),
    }


FAMILIES = _families()


@functools.lru_cache(maxsize=None)
def case(family, name):
    return FAMILIES[family][name]()


# the kill table: wrong rule -> designed slices (family, case, slice) whose mask it changes (tests/test_host_k8_edges.py asserts each)
KILLERS = {
    'ins_tie_ge': [('band_and_ties', 'noisy_unit3_seed1009_params2', 0), ('band_and_ties', 'noisy_unit4_seed1007_params1', 0)],
    'del_tie_ge': [('band_and_ties', 'noisy_unit2_seed1000_params0', 0), ('band_and_ties', 'noisy_unit3_seed1003_params0', 0)],
    'del_from_prev_column': [('band_and_ties', 'noisy_unit2_seed1008_params0', 0), ('band_and_ties', 'noisy_unit3_seed1004_params0', 0)],
    'best_on_ge': [('band_and_ties', 'noisy_unit4_seed1000_params1', 0), ('band_and_ties', 'noisy_unit6_seed1000_params0', 0)],
    'gt_minscore': [('threshold', 'to64_delta7', 1), ('threshold', 'homopolymer', 1), ('band_and_ties', 'noisy_unit2_seed1008_params0', 0)],
    'mask_ends_at_j': [('threshold', 'to64_delta7', 1), ('placement', 'starts_at_bit_32', 0)],
    'band_p_le_5': [('band_and_ties', 'noisy_unit4_seed1003_params0', 0), ('band_and_ties', 'noisy_unit20_seed1001_params2', 0)],
    'band_p_lt_4': [('band_and_ties', 'noisy_unit5_seed1009_params2', 0), ('band_and_ties', 'noisy_unit20_seed1001_params2', 0)],
    'non_acgt_match': [('letters', 'letters', 0), ('letters', 'letters', 1)],
}
