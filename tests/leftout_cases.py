"""A designed genome for the "left out" contract (include/mimeo_hip.h, mimeo_get_failed_pairs): which scaffold pairs hit
the engine's trace-pool limit under MIMEO_K6_TRACE_POOL_MB=1, and on which strand, follows from the design — nothing is
drawn so that "something" fails.

Scaffolds: `nscaf` (6: below PACK_MIN, the per-pair path and dist.deal_units; 9: a full cross product is packed) scaffolds
of SCAF_BP + 97 i bases of random ACGT, each drawn from its own generator (seed, i), so that the six-scaffold genome is the
first six scaffolds of the nine-scaffold one and the two share their oracle rows.

Background: two families of 250-500 bp; every scaffold carries one forward and one reverse-complemented copy of each, up
to 10 % substitutions and synth's indels, in four slots of 2000 bp in permuted order (BG0 ..): at least 1100 random bases
lie between two copies, more than a gapped extension crosses at y-drop 9400 (280 do not stop it), so no alignment joins two
copies.  Every pair of scaffolds then has rows on both strands, and a half extension of a background copy has at most about
520 rows.

Long regions L1, L2, L3 of LONG_BP = 12 000 bp; every placed copy carries 3 % substitutions and six indels of 1-3 bases of
its own, so no copy equals its partner (an identical half takes the identical-suffix shortcut, needs no pool and cannot
fail).  L1: forward in scaffold 0, reverse-complemented in scaffold 3 -> (0, 3) and (3, 0) fail on the minus strand only.
L2: forward in scaffolds 1 and 4 -> (1, 4) and (4, 1) fail on the plus strand only.  L3: twice in scaffold 5, 8 kbp of
background slots between the copies, the second copy reverse-complemented -> the self pair (5, 5) fails on the minus strand.
(Two forward copies would not do: lastz --chain keeps one collinear chain per strand, on the plus strand of a self pair that
is the main diagonal alone, so the HSPs between two forward copies are never extended — the oracle returns one plus-strand
row for every (t, t).)  Scaffolds 2, 6, 7 and 8 carry only
background.  Two copies of 12 kbp and 8 kbp between them need 32 kbp, hence SCAF_BP = 34 000 rather than 30 000.

Sizes (k6_trace.hip, trace_round): a half of r rows needs about r (W + 16) bytes with W = max(maxcols, (ydrop - open) /
extend + 1) + (ydrop + 200) / extend + 4 >= 625 at the default penalties: a background half about 0.35 MB at the narrowest W (W grows
with the band), the larger half of a 12 kbp copy (at least 6000 rows) at least 3.8 MB, against a pool of 1 MB.
Readings of the engine's own MIMEO_K6_STATS line (`largest half … MB`) on the MI355X, pool uncapped, paths asked for:
  nscaf = 9 built without the long regions, all 81 pairs:   0.458 MB   (must be below 0.5; 754 halves traced)
  each designed pair alone:                                 (0, 3) 5.718, (3, 0) 6.054, (1, 4) 9.732, (4, 1) 9.602,
                                                            (5, 5) 8.086 MB   (must be above 2)
These readings size the inputs; no assertion about results uses them."""
import numpy as np

from mimeo_amd.synth import _ACGT, _COMP, _mutate

SCAF_BP = 34_000
LONG_BP = 12_000
LONG_AT = 1_000                  # the long region of scaffolds 0, 1, 3, 4 and the first copy of L3 in scaffold 5
LONG_AT2 = LONG_AT + LONG_BP + 8_000   # the second copy of L3
BG0, BG_STEP = LONG_AT + LONG_BP + 400, 2_000   # four background slots between the two long positions
PLUS, MINUS = 0, 1               # qstrand of a record
# the designed pairs and the strand on which each hits the limit
F = {(0, 3): MINUS, (3, 0): MINUS, (1, 4): PLUS, (4, 1): PLUS, (5, 5): MINUS}
# (scaffold, long region, position, reverse-complemented)
PLACED = [(0, 0, LONG_AT, False), (3, 0, LONG_AT, True), (1, 1, LONG_AT, False), (4, 1, LONG_AT, False),
          (5, 2, LONG_AT, False), (5, 2, LONG_AT2, True)]


def _rng(seed, *key):
    return np.random.Generator(np.random.PCG64([seed, *key]))


def _long_copy(rng, region):
    """3 % substitutions and six indels of 1-3 bases, exactly LONG_BP bases (cut or padded at the end)"""
    c = region.copy()
    m = rng.random(c.size) < 0.03
    c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
    for p in sorted(rng.integers(500, c.size - 500, size=6).tolist(), reverse=True):
        ln = int(rng.integers(1, 4))
        c = np.delete(c, slice(p, p + ln)) if rng.random() < 0.5 else np.insert(c, p, rng.integers(0, 4, size=ln, dtype=np.uint8))
    if c.size < LONG_BP:
        c = np.concatenate([c, rng.integers(0, 4, size=LONG_BP - c.size, dtype=np.uint8)])
    return c[:LONG_BP]


def genome(nscaf, seed=20, long_regions=True):
    """(names, list of uint8 ASCII arrays); genome(6) is the first six scaffolds of genome(9)"""
    assert nscaf >= 6
    fr = _rng(seed, 1000)
    fams = [fr.integers(0, 4, size=int(fr.integers(250, 501)), dtype=np.uint8) for _ in range(2)]
    regions = [fr.integers(0, 4, size=LONG_BP, dtype=np.uint8) for _ in range(3)]
    seqs = []
    for i in range(nscaf):
        rng = _rng(seed, i)
        c = rng.integers(0, 4, size=SCAF_BP + 97 * i, dtype=np.uint8)
        slots = rng.permutation(4)
        for k, slot in enumerate(slots.tolist()):
            cp = _mutate(rng, fams[k // 2], float(rng.random()) * 0.10, 0.005)[:520]
            if k % 2:
                cp = _COMP[cp[::-1]]
            at = BG0 + BG_STEP * slot + int(rng.integers(0, 300))
            c[at:at + cp.size] = cp
        if long_regions:
            for n, (s, reg, at, rc) in enumerate(PLACED):
                if s == i:
                    cp = _long_copy(_rng(seed, 2000 + n), regions[reg])
                    c[at:at + LONG_BP] = _COMP[cp[::-1]] if rc else cp
        seqs.append(_ACGT[c])
    return ['lo%02d' % i for i in range(nscaf)], seqs


def shares_a_scaffold_with_F(t, q):
    used = {s for pr in F for s in pr}
    return (t, q) not in F and (t in used or q in used)


def oracle_pair(T, Q):
    """An oracle job (tests/oracle_pool.py): lastz(target T, query Q), both strands, uncapped"""
    from oracle import oracle as O
    return O.align_pair(bytes(T), bytes(Q))


_oracle = {}


def oracle_rows(seqs, pairs, seed=20, cap=16):
    """{(t, q): the oracle's records}, computed once per pair and process (the two genomes share their first six scaffolds)"""
    from tests import oracle_pool
    from oracle import oracle as O
    O.lib()
    todo = [pr for pr in dict.fromkeys(pairs) if (seed, pr) not in _oracle]
    for pr, recs in zip(todo, oracle_pool.run([(oracle_pair, seqs[t], seqs[q]) for t, q in todo], cap)):
        _oracle[(seed, pr)] = recs
    return {pr: _oracle[(seed, pr)] for pr in pairs}
