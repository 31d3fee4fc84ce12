"""K8 tandem scorer beyond 64 periods (`--tmaxperiod` up to 2000, TRF's own range; k8_tandem_mask_wide: one wavefront per
(slice, block of 64 periods), the job list of host_plan::tandem_jobs): exact agreement with the CPU restatement
`oracle.pipeline.tandem_masked` at the block edges, over a reordered job list and at the top of the range, the
behaviour the filter needs on satellite-sized units (100 - 200 bases), and the two commands.  As for the periods up to 64
(test_gpu_tandem.py), agreement with TRF itself cannot be measured here: PARITY UNPINNED."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b'ACGT', np.uint8)


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def _random(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def _array(rng, unit, copies=5, sub=0.03, indel=0.0):
    """`copies` copies of a random unit of `unit` bases: `sub` substitutions, `indel` single-base insertions or deletions"""
    rep = np.tile(_random(rng, unit), copies)
    out = bytearray()
    for c in rep.tolist():
        r = rng.random()
        if r < indel / 2:
            continue                                    # deletion
        if r < indel:
            out.append(int(ACGT[rng.integers(0, 4)]))   # insertion in front
        if rng.random() < sub:
            c = int(ACGT[rng.integers(0, 4)])
        out.append(c)
    return np.frombuffer(bytes(out), np.uint8).copy()


def _scaffold(seed, units, spacer=(300, 420)):
    """Arrays of the given unit lengths (every second one with 2 % indels) between random spacers; the first array starts at
    base 0 and the last one ends at the scaffold's last base.  Returns (bases, spans of the arrays)."""
    rng = np.random.default_rng(seed)
    parts, spans, pos = [], [], 0
    for i, u in enumerate(units):
        if i:
            sp = _random(rng, int(rng.integers(*spacer)))
            parts.append(sp)
            pos += sp.size
        a = _array(rng, u, indel=0.02 if i % 2 else 0.0)
        parts.append(a)
        spans.append((pos, pos + a.size))
        pos += a.size
    return np.concatenate(parts), spans


EDGE_UNITS = (64, 65, 66, 127, 128, 129, 130)


@pytest.fixture(scope='module')
def edge_scaffold():
    s, spans = _scaffold(21, EDGE_UNITS)
    a, b = spans[3]
    s[a + 150:a + 170] = ord('N')                 # an N run inside the 127-base array
    a, b = spans[4]
    s[a - 100:a + 300] |= 0x20                    # a lower-case stretch over the start of the 128-base array
    return s, spans


def _oracle(seqs, iv, params, memo=None, return_mask=False):
    from oracle import pipeline as P
    memo = {} if memo is None else memo
    out = []
    for c, s, e in iv:
        if (c, s, e) not in memo:
            memo[(c, s, e)] = np.array(P.tandem_masked(seqs[c].tobytes(), s, min(e, len(seqs[c])), *params, return_mask=True), dtype=bool)
        out.append(memo[(c, s, e)] if return_mask else int(memo[(c, s, e)].sum()))
    return out


# (match, mismatch, minscore, maxperiod, delta): two blocks with the last lanes off, one period into the second block, two
# full blocks (other weights), one period into the third block without the indel moves
@pytest.mark.parametrize('params', [(2, 7, 50, 130, 7), (2, 7, 50, 65, 7), (3, 7, 80, 128, 9), (2, 7, 50, 129, 0)])
def test_block_edges_equal_cpu_restatement(eng, edge_scaffold, params):
    seq, spans = edge_scaffold
    n = len(seq)
    assert 5500 < n < 6500 and spans[0][0] == 0 and spans[-1][1] == n
    rng = np.random.default_rng(22)
    iv = [(0, max(0, a - int(rng.integers(0, 81))), min(n, b + int(rng.integers(0, 81)))) for a, b in spans]
    iv += [(0, 0, 150), (0, n - 150, n + 40)]                                   # from base 0; to the scaffold end (and clipped there)
    starts = (0, spans[1][0] + 3, spans[2][0], n - 66, spans[4][0] + 1, spans[0][0] + 5)
    iv += [(0, a, a + ln) for a, ln in zip(starts, (1, 63, 64, 66, 129, 131))]
    iv += [(0, 10, 10)]
    assert sum(min(e, n) - s for _, s, e in iv) * params[3] < 1.5e6             # the restatement's work, kept small
    g = eng.Genome(['edge'], [seq])
    got = eng.tandem_masked(g, np.array(iv, dtype=np.uint32), *params)
    masks = eng.tandem_mask(g, np.array(iv, dtype=np.uint32), *params)
    g.close()
    memo = {}
    exp = _oracle([seq], iv, params, memo)
    assert got.tolist() == exp, params
    for k, (m, x) in enumerate(zip(masks, _oracle([seq], iv, params, memo, return_mask=True))):   # the positions, not only how many
        assert m.shape == x.shape and np.array_equal(m, x), (params, iv[k], np.flatnonzero(m != x)[:8].tolist())
    if params[3] >= 128 and params[4] > 0:
        assert sum(exp[:7]) > 0.85 * sum(b - a for a, b in spans)               # the arrays are what is being masked


def test_reordered_job_list_equals_cpu_restatement(eng, edge_scaffold):
    """~120 slices of 1 .. 140 bases on two scaffolds, shuffled, some twice: the jobs are sorted by slice length and the
    blocks without work left out, and every result must still land on its own slice."""
    params = (2, 7, 50, 130, 7)
    seq0 = edge_scaffold[0]
    seq1, _ = _scaffold(23, (3, 10, 33, 40, 50, 66, 70, 96), spacer=(40, 90))
    seqs = [seq0, seq1]
    rng = np.random.default_rng(24)
    iv = []
    for i in range(100):
        c = int(rng.integers(0, 2))
        ln = int(rng.integers(1 if i % 2 else 90, 141))   # every second one long enough for a unit of 64 and 25 matches
        a = int(rng.integers(0, len(seqs[c]) - ln + 1))
        iv.append((c, a, a + ln))
    iv += [(0, 0, 140), (1, len(seq1) - 140, len(seq1)), (1, 0, 1), (0, 64, 128), (0, 0, 63), (1, 5, 5)]
    iv += [iv[i] for i in rng.integers(0, len(iv), 14)]
    order = rng.permutation(len(iv))
    iv = [iv[i] for i in order]
    assert len(iv) == 120 and sum(e - s for _, s, e in iv) * params[3] < 1.5e6
    g = eng.Genome(['edge', 'short'], seqs)
    got = eng.tandem_masked(g, np.array(iv, dtype=np.uint32), *params)
    g.close()
    exp = _oracle(seqs, iv, params, {})
    assert got.tolist() == exp
    assert sum(1 for x in exp if x) >= 20 and sum(1 for x in exp if not x) >= 20   # both kinds of slice are there


def test_top_of_range_gap_free(eng):
    """u + u[:60], u = 1990 random bases, as one slice without the indel moves: only period 1990 sees the copy, so the
    whole slice is masked at maxperiod 2000 and nothing at 1989."""
    from oracle import pipeline as P
    rng = np.random.default_rng(25)
    u = _random(rng, 1990)
    s = np.concatenate([u, u[:60]])
    g = eng.Genome(['top'], [s])
    iv = np.array([(0, 0, 2050)], dtype=np.uint32)
    got = [int(eng.tandem_masked(g, iv, 2, 7, 50, mp, 0)[0]) for mp in (2000, 1989)]
    g.close()
    exp = [P.tandem_masked(s.tobytes(), 0, 2050, 2, 7, 50, mp, 0) for mp in (2000, 1989)]
    assert exp == [2050, 0]
    assert got == exp


def test_unit_of_500_at_maxperiod_2000(eng):
    from oracle import pipeline as P
    rng = np.random.default_rng(26)
    s = np.tile(_random(rng, 500), 3)[:1200]
    g = eng.Genome(['u500'], [s])
    got = int(eng.tandem_masked(g, np.array([(0, 0, 1200)], dtype=np.uint32), 2, 7, 50, 2000, 7)[0])
    g.close()
    exp = P.tandem_masked(s.tobytes(), 0, 1200, 2, 7, 50, 2000, 7)
    assert exp == 1200
    assert got == exp


def test_maxperiod_outside_1_to_2000_raises_and_the_engine_goes_on(eng):
    rng = np.random.default_rng(27)
    s = np.concatenate([_random(rng, 300), np.frombuffer(b'CA' * 100, np.uint8)])
    g = eng.Genome(['s'], [s])
    iv = np.array([(0, 0, 500)], dtype=np.uint32)
    for bad in (2001, 0, -1):
        with pytest.raises(RuntimeError, match='2000'):
            eng.tandem_masked(g, iv, 2, 7, 50, bad, 7)
    assert 190 <= int(eng.tandem_masked(g, iv, 2, 7, 50, 2000, 7)[0]) <= 260   # the CA run, and the engine still works
    assert int(eng.tandem_masked(g, iv)[0]) >= 190
    g.close()


def test_satellite_units_masked_random_not(eng):
    """What the range is for: five-copy arrays of 100-, 171- and 200-base units (3 % substitutions, without and with 2 %
    indels) are masked at maxperiod = unit + 8 and not at all at 50; random sequence stays unmasked at 400.  (The
    restatement gives >= 0.995, 0 and 0 on such inputs; 0.85 and 0.08 are the thresholds of test_gpu_tandem.py.)"""
    rng = np.random.default_rng(28)
    parts, spans, units, pos = [], [], [], 0
    for unit in (100, 171, 200):
        for indel in (0.0, 0.02):
            a = _array(rng, unit, indel=indel)
            sp = _random(rng, 200)
            parts += [a, sp]
            spans.append((pos, pos + a.size))
            units.append(unit)
            pos += a.size + sp.size
    parts.append(_random(rng, 2000))
    g = eng.Genome(['sat'], [np.concatenate(parts)])
    for (a, b), unit in zip(spans, units):
        iv = np.array([(0, a, b)], dtype=np.uint32)
        assert int(eng.tandem_masked(g, iv, 2, 7, 50, unit + 8, 7)[0]) / (b - a) > 0.85, unit
        assert int(eng.tandem_masked(g, iv, 2, 7, 50, 50, 7)[0]) == 0, unit
    rnd = np.array([(0, pos, pos + 2000)], dtype=np.uint32)
    assert int(eng.tandem_masked(g, rnd, 2, 7, 50, 400, 7)[0]) / 2000.0 < 0.08
    g.close()


def test_filter_command_drops_a_171_base_satellite(eng, tmp_path):
    from mimeo_amd import formats, run_filter
    rng = np.random.default_rng(29)
    recs = [('te1', _random(rng, 900).tobytes()), ('sat171', _array(rng, 171, copies=6).tobytes())]
    lib = tmp_path / 'lib.fa'
    lib.write_bytes(b''.join(b'>' + n.encode() + b'\n' + s + b'\n' for n, s in recs))
    run_filter.main(['--infile', str(lib), '-d', str(tmp_path / 'default')])
    assert formats.read_fasta(str(tmp_path / 'default' / 'lib_filtered.fa'))[0] == ['te1', 'sat171']
    run_filter.main(['--infile', str(lib), '-d', str(tmp_path / 'wide'), '--tmaxperiod', '200'])
    names, seqs = formats.read_fasta(str(tmp_path / 'wide' / 'lib_filtered.fa'))
    assert names == ['te1'] and seqs[0].tobytes() == recs[0][1]


def test_trf_filter_at_tmaxperiod_200_equals_restatement(eng):
    from mimeo_amd import workflow
    from oracle import pipeline as P
    rng = np.random.default_rng(30)
    sat = _array(rng, 171, indel=0.02)
    seq = np.concatenate([_random(rng, 500), sat, _random(rng, 1500)])
    a = 500
    names = ['chrA', 'chrB']
    g = eng.Genome(names, [seq, _random(rng, 400)])
    rows = [[names[0], '+', str(a + 10), str(a + sat.size - 10), names[1], '+', '1', '300', '9999', '99.0'],
            [names[0], '+', str(a + sat.size + 300), str(a + sat.size + 1000), names[1], '-', '7', '307', '8888', '98.5']]
    got = workflow.trf_filter(rows, g, tmaxperiod=200, maxtandem=40)
    exp = P.trf_filter(rows, {names[0]: seq.tobytes()}, tmaxperiod=200, maxtandem=40)
    assert got == exp and [r[2] for r in got] == [rows[1][2]]
    assert len(workflow.trf_filter(rows, g, maxtandem=40)) == 2    # at the default of 50 the satellite passes as if it were a transposon
    g.close()
