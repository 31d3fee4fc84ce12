"""The step bench.py times (workload c4): one target row of the 1 Gbp self job, 100 scaffolds of 10 Mbp, through
mimeo_align_units with every seed index resident but the row's own — the row's minus-strand units, its self unit, and the
plus-strand unit of every pair it owns in both orders (dist.units_of_row), each owned pair scanned once and emitted
transposed for the other order.  One batch and one K34 launch over every scanned unit: 24 end bits, 25 diagonal bits and
8 unit bits in the follower key, two LDS segments per query tile.

The records are checked (a) against the C oracle on a fixed sample of the row's units, (b) against the round-1
decomposition of the same stages — MIMEO_HEAVY=v1 (stand-alone seed scan K3 + hit array), MIMEO_MIRROR=0 (every unit
scanned, no shared plus strand), MIMEO_BATCH_UNITS=1 (a batch per unit: key widths of that unit alone) — byte for byte,
and (c) the seed-hit count against MIMEO_HEAVY=v1 with the shared plus strand kept.  Rows 0 and 57 have the two ownership
parities of circulant dealing (dist.plus_owner)."""
import numpy as np
import pytest

from mimeo_amd import dist
from tests import oracle_pool as OP

pytestmark = pytest.mark.gpu

ROWS = (0, 57)
ENV = ('MIMEO_HEAVY', 'MIMEO_MIRROR', 'MIMEO_BATCH_UNITS', 'MIMEO_PACK', 'MIMEO_K4_VARIANT', 'MIMEO_INDEX_BUDGET_MB')


def row_plan(t, nscaf):
    """What the engine must make of units_of_row(t): the (target, query, minus) units it scans, in launch order (target-major,
    stable in the list's order; plus before minus; a mirror unit rides with its source), the mirror units, and the number of
    (target, query, strand) units in all."""
    units = dist.units_of_row(t, nscaf)
    # every pair {t, q} the row owns is named in both orders on the plus strand: (min, max, +) is scanned and
    # (max, min, +) receives its HSPs transposed
    owned = [b for a, b, m in units if a == t and b != t and m == dist.BOTH]
    assert sorted(a for a, b, m in units if a != t) == owned and all(m == dist.PLUS for a, b, m in units if a != t)
    mirrors = [(max(t, q), min(t, q), 0) for q in owned]
    scanned = []
    for a, b, m in sorted(units, key=lambda u: u[0]):
        for minus in (0, 1):
            if m & (2 if minus else 1) and (a, b, minus) not in mirrors:
                scanned.append((a, b, minus))
    total = sum(bin(m).count('1') for _, _, m in units)
    assert len(scanned) + len(mirrors) == total
    return units, scanned, mirrors, total


def oracle_sample(t, nscaf, seed=57):
    """Row t's units put under the oracle: the self unit on both strands, the first and last pair the row owns with their
    mirror units, two minus-only units (one picked by a fixed seed; the other is the last unit the launch scans), and the
    first scanned unit (the self unit's plus strand)."""
    units, scanned, mirrors, _ = row_plan(t, nscaf)
    owned = [b for a, b, m in units if a == t and b != t and m == dist.BOTH]
    minus_only = [b for a, b, m in units if a == t and m == dist.MINUS]
    last = scanned[-1]
    assert last[2] == 1 and last[1] in minus_only
    rng = np.random.default_rng(seed)
    pick = int(rng.choice([q for q in minus_only if q != last[1]]))
    sample = [(t, t, 0), (t, t, 1)]
    for q in (owned[0], owned[-1]):
        sample += [(t, q, 0), (q, t, 0)]
    sample += [(t, pick, 1), last]
    assert scanned[0] == (t, t, 0) and sum(u in mirrors for u in sample) == 2
    return sample


@pytest.fixture(scope='module')
def c4():
    import bench
    from mimeo_amd import engine
    from mimeo_amd.synth import synth_genome
    mode, seed, _, total_bp, nscaf, _, _, kind = bench.WORKLOADS['c4']
    assert mode == 'self' and kind == 'row'
    engine.init(0)
    names, seqs = synth_genome(seed, total_bp, nscaf)
    A = engine.Genome(names, seqs)
    yield engine, A, seqs, nscaf
    A.close()


def _clear(monkeypatch):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)


def test_c4_rows_match_the_oracle_and_the_round1_decomposition(c4, monkeypatch):
    eng, A, seqs, S = c4
    _clear(monkeypatch)
    sample = oracle_sample(ROWS[0], S)
    # the oracle works through its sample on the host while the GPU runs the rows
    pending = OP.start([(OP.align_unit, seqs[a], seqs[b], minus) for a, b, minus in sample], 8)
    params = eng.default_params()
    # (1) the bench's step: indexes of every scaffold resident, then per row the row's own dropped and its units aligned
    A.build_indexes()
    fused, hits = {}, {}
    for t in ROWS:
        units, scanned, mirrors, total = row_plan(t, S)
        A.drop_indexes([t])
        fused[t] = eng.align_units(A, None, units, params)
        st = eng.stats()
        assert not eng.failed_pairs()
        # the launch shape the bench times: one batch, one K34 launch over every scanned unit, the mirror units riding along
        assert st['batches'] == 1, (t, st['batches'])
        assert st['scan_kernel_launches'] == 1, (t, st['scan_kernel_launches'])
        assert st['pair_strands'] == total, (t, st['pair_strands'], total)
        assert st['scan_launches'] == len(scanned) == total - len(mirrors), (t, st['scan_launches'], len(scanned))
        assert st['super_units'] == 0 and st['alignments'] == fused[t].size > 1000
        hits[t] = st['seed_hits']
        assert hits[t] > 13.0 * len(scanned) * float(A.lengths[0]) ** 2 / 4 ** 12
        assert {(int(a), int(b)) for a, b in zip(fused[t]['tid'], fused[t]['qid'])} <= {(a, b) for a, b, _ in units}
    # (2) the same rows through the round-1 decomposition, indexes built per call
    A.drop_indexes()
    A.keep_indexes(False)
    for tag, env in (('v1', {'MIMEO_HEAVY': 'v1'}), ('v1_unit_batches', {'MIMEO_HEAVY': 'v1', 'MIMEO_MIRROR': '0', 'MIMEO_BATCH_UNITS': '1'})):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        for t in ROWS:
            units, scanned, mirrors, total = row_plan(t, S)
            alt = eng.align_units(A, None, units, params)
            st = eng.stats()
            assert not eng.failed_pairs()
            assert st['pair_strands'] == total
            if tag == 'v1':   # the same units scanned, by another seed scan: the same seed hits
                assert st['scan_launches'] == len(scanned) and st['seed_hits'] == hits[t], (tag, t, st['seed_hits'], hits[t])
            else:             # every unit scanned, each in a batch of its own
                assert st['scan_launches'] == st['batches'] == total, (tag, t, st['scan_launches'], st['batches'])
            assert alt.tobytes() == fused[t].tobytes(), (tag, t, alt.size, fused[t].size)
        _clear(monkeypatch)
    # (3) the oracle's sample of row 0, unit by unit
    rows = [OP.assert_unit_matches(fused[ROWS[0]], exp, a, b, minus, 'c4 row %d' % ROWS[0])
            for (a, b, minus), exp in zip(sample, pending.results())]
    assert sum(rows) > 100 and sum(1 for n in rows if n) >= 6, list(zip(sample, rows))


def test_queue_sizing_starts_afresh_in_every_call(monkeypatch):
    """Regression: the extension queues' learned sizing outlived the call that learned it.  One repeat-rich call (the genome
    of test_gpu_align.test_wave_chain_on_every_group_size: its batch overflows and the boosts rose to ~100-300) sized the
    queues of every later call on any input; in the whole suite the C4 row above ran as 125 batches instead of one, and a C2
    call after it failed to allocate 190 GiB.  Here a random pair under a fixed 3 GiB queue budget: one batch before the
    repeat-rich call and one after it (several before the fix), and the same records (none: random bases align nowhere)."""
    from mimeo_amd import engine as eng
    from mimeo_amd.synth import synth_genome
    eng.init(0)
    _clear(monkeypatch)
    names, seqs = synth_genome(5, 8_000_000, 2, repeat_frac=0.0)
    g = eng.Genome(names, seqs)
    rn, rs = synth_genome(93, 900_000, 3, repeat_frac=0.3, families=3, cons_len=(200, 2500), max_div=0.2, indel_rate=0.02, microsat_frac=0.02)
    r = eng.Genome(rn, rs)
    monkeypatch.setenv('MIMEO_QUEUE_BUDGET_MB', '3072')
    pairs = [(0, 1), (1, 0)]
    before = eng.align_pairs(g, None, pairs)
    st = eng.stats()
    assert st['batches'] == 1 and st['queue_reruns'] == 0, st
    eng.align_pairs(r, None, [(t, q) for t in range(3) for q in range(3)])
    assert eng.stats()['queue_reruns'] >= 1   # its queues overflowed: what the sizing learned from
    after = eng.align_pairs(g, None, pairs)
    st = eng.stats()
    monkeypatch.delenv('MIMEO_QUEUE_BUDGET_MB')
    assert st['batches'] == 1 and st['queue_reruns'] == 0, st
    assert after.tobytes() == before.tobytes()
    g.close()
    r.close()
