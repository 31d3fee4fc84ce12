"""One chromosome-scale scaffold: `big`, 268 500 000 bases (just above 2^28 - 19), against 40 scaffolds of 20-60 kbp that
share its repeat families, through one mimeo_align_pairs call: (big, s) and (s, big) for every small s and a few (s, s').

Three code paths switch on only at this scale.  The follower key of a batch holding big in both roles takes 29 end bits and
30 diagonal bits (ExtBatch::run), which leaves 5 unit bits: the pipeline cuts batches at 32 units (ext_batch_max_units), not
at MAX_GROUPS.  And a K34 query tile of big holds about 65 550 entries, so its tiles fall on both sides of the 65 535 entries
a first-pass tile may hold: those above go to the heavy / split pass in the same launch.  Copies of two repeat families lie
flush with big's first and last base, so records and keys reach the top of their fields.

The records are checked against the round-1 decomposition (MIMEO_HEAVY=v1, MIMEO_MIRROR=0, MIMEO_BATCH_UNITS=1: a batch of
one unit takes the key widths of that unit alone) byte for byte, and against the C oracle on eight units: both orders of
the two pairs that carry the flush copies, on the strand that aligns them, and four units picked by a fixed seed.  The
(big, big) pair is left out: the oracle cannot afford it."""
import numpy as np
import pytest

from mimeo_amd.synth import make_families, synth_genome
from tests import oracle_pool as OP

pytestmark = pytest.mark.gpu

BIG = 268_500_000
NSMALL = 40
SEED_LEN = 19
CARE = np.array([0, 1, 2, 4, 7, 8, 11, 13, 15, 16, 17, 18])   # the 12of19 seed 1110100110010101111 (device_util.h: pext12)
ENV = ('MIMEO_HEAVY', 'MIMEO_MIRROR', 'MIMEO_BATCH_UNITS', 'MIMEO_PACK', 'MIMEO_K4_VARIANT', 'MIMEO_INDEX_BUDGET_MB')
_ACGT = np.frombuffer(b'ACGT', np.uint8)


def bits_for(v):
    """bits that hold the values 0 .. v (k4_extend.hip)"""
    return max(1, int(v).bit_length())


def ext_batch_max_units(max_t, max_q):
    """k4_extend.hip: the follower key is unit << (dbits + ebits) | (diagonal + Lq) << ebits | seed end, 64 bits"""
    ebits, dbits = bits_for(max_t + SEED_LEN), bits_for(max_t + max_q + SEED_LEN)
    ubits = 64 - min(63, ebits + dbits)
    return 1 << min(ubits, 20)


def chromosome_genome(seed=2031):
    """names, ASCII arrays, and {small scaffold: the strand (0 plus, 1 minus) on which it aligns with big's ends}: big is
    scaffold 0"""
    rng = np.random.default_rng(seed)
    fams = make_families(seed, 14, (500, 3000))
    shared, flush = fams[:12], fams[12:]
    _, (big,) = synth_genome(seed + 1, BIG, 1, repeat_frac=0.02, shared_families=shared)
    smalls = [synth_genome(seed + 2 + i, int(rng.integers(20_000, 60_001)), 1, repeat_frac=0.08, shared_families=shared)[1][0]
              for i in range(NSMALL)]
    # family 12 ends at big's first base and family 13 at its last; both are copied (3 % substitutions) forward into one
    # small scaffold and reverse-complemented into another, so that records on both strands reach big's ends.  The two
    # copies of a small scaffold are collinear with big's on their strand, so that one chain (--chain) takes both
    head, tail = flush
    big[:head.size] = _ACGT[head]
    big[BIG - tail.size:] = _ACGT[tail]
    carriers = {}
    for s, minus in ((3, 0), (17, 1)):
        for fam, p in ((head, 12_000 if minus else 1000), (tail, 1000 if minus else 12_000)):
            c = fam.copy()
            m = rng.random(c.size) < 0.03
            c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
            smalls[s][p:p + c.size] = _ACGT[(3 - c)[::-1] if minus else c]
        carriers[s + 1] = minus
    names = ['big'] + ['s%02d' % i for i in range(NSMALL)]
    return names, [big] + smalls, carriers


def tile_counts(seq, minus):
    """query entries of every K34 tile of one strand of `seq`: a tile is the 12 low-plane bits (bit 0 of the 2-bit code
    A0 C1 G2 T3) at the care positions of the 19-base window (common.h: key = pext12(lo) << 12 | pext12(hi)); counted in
    chunks.  The synthetic bases are all ACGT, so every window that fits is a seed word."""
    code = np.searchsorted(_ACGT, seq).astype(np.uint8)
    if minus:
        code = (3 - code)[::-1]
    lo = code & 1
    n = lo.size - SEED_LEN + 1
    counts = np.zeros(4096, dtype=np.int64)
    step = 1 << 24
    for p0 in range(0, n, step):
        p1 = min(n, p0 + step)
        tile = np.zeros(p1 - p0, dtype=np.uint16)
        for j, c in enumerate(CARE):
            tile |= lo[p0 + c:p1 + c].astype(np.uint16) << j
        counts += np.bincount(tile, minlength=4096)
    assert counts.sum() == n
    return counts


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def _clear(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def test_chromosome_scale_scaffold_matches_the_oracle_and_the_round1_decomposition(eng, monkeypatch):
    _clear(monkeypatch)
    names, seqs, carriers = chromosome_genome()
    assert len(seqs[0]) == BIG > 2 ** 28 - SEED_LEN
    smalls = range(1, NSMALL + 1)
    pairs = [(0, s) for s in smalls] + [(s, 0) for s in smalls] + [(s, s + 1) for s in range(1, 12, 2)]
    # the oracle's sample: both orders of the two pairs that carry the flush copies, on the strand that aligns them, and four
    # more units picked by a fixed seed — a unit per job, at most four at a time: a call with big in it takes the oracle
    # about two minutes of a core and holds up to 2.7 GB
    flush = [(0, s, m) for s, m in sorted(carriers.items())] + [(s, 0, m) for s, m in sorted(carriers.items())]
    rest = [(t, q, m) for t, q in pairs for m in (0, 1) if (t, q, m) not in flush]
    rng = np.random.default_rng(5)
    units = flush + [rest[int(k)] for k in rng.choice(len(rest), 4, replace=False)]
    pending = OP.start([(OP.align_unit, seqs[t], seqs[q], minus) for t, q, minus in units], 4)
    G = eng.Genome(names, seqs)
    got = eng.align_pairs(G, None, pairs)
    st = eng.stats()
    assert not eng.failed_pairs()
    # shape: no super-scaffolds (not a cross product), every pair on both strands, batches cut by the width of the key
    strands = 2 * len(pairs)
    cap = ext_batch_max_units(BIG, BIG)
    assert cap == 32 and bits_for(BIG + SEED_LEN) == 29 and bits_for(2 * BIG + SEED_LEN) == 30
    assert st['super_units'] == 0 and st['pair_strands'] == strands, st
    assert st['batches'] >= -(-strands // cap) and st['batches'] > 1, (st['batches'], strands)
    # records reach the top of the 29-bit coordinate fields, on both strands, in both roles of big
    for minus in (0, 1):
        on = got[got['qstrand'] == minus]
        assert (on['tend'][on['tid'] == 0] > 2 ** 28).any(), minus
        assert (on['qend'][on['qid'] == 0] > 2 ** 28).any(), minus
        assert (on['tstart'][on['tid'] == 0] < 64).any() and (on['qstart'][on['qid'] == 0] < 64).any(), minus
    # tiles of big's query strands on both sides of the 65 535 entries of a first-pass tile (the minus strand is scanned
    # as query by (s, big, -); the plus strand too once the shared plus strand is off)
    for minus in (1, 0):
        cnt = tile_counts(seqs[0], minus)
        assert (cnt > 0xFFFF).sum() > 100 and (cnt <= 0xFFFF).sum() > 100, (minus, int(cnt.min()), int(cnt.max()))
    # the round-1 decomposition, a batch per unit, every unit scanned
    for k, v in (('MIMEO_HEAVY', 'v1'), ('MIMEO_MIRROR', '0'), ('MIMEO_BATCH_UNITS', '1')):
        monkeypatch.setenv(k, v)
    alt = eng.align_pairs(G, None, pairs)
    st1 = eng.stats()
    _clear(monkeypatch)
    G.close()
    assert not eng.failed_pairs()
    assert st1['batches'] == st1['scan_launches'] == strands, st1
    assert alt.tobytes() == got.tobytes(), (alt.size, got.size)
    # the oracle, unit by unit
    rows = [OP.assert_unit_matches(got, exp, t, q, minus, 'chromosome') for (t, q, minus), exp in zip(units, pending.results())]
    assert all(rows[:len(flush)]), list(zip(units, rows))
