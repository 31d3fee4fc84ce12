"""The gap-free stage on DESIGNED diagonals (tests/gapfree_cases.py): walks that stop on the pre-filter's block edges and on the
window hand-overs, dips that cost exactly the x-drop, scores exactly at the threshold, seeds that end exactly at a dismissed head's
reach — the cases the random pairs of test_gpu_hsp.py / test_gpu_runs.py / test_gpu_segments.py leave to chance.  That the
families reach those edges is asserted on the CPU (tests/test_host_gapfree_edges.py), where the oracle is also held to the
second restatement on them.  Here the engine must equal the oracle, exactly, under K34 and under the three round-1 variants."""
import numpy as np
import pytest

from tests import gapfree_cases as G
from tests import oracle_pool

pytestmark = pytest.mark.gpu

COLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
ACOLS = oracle_pool.ACOLS
ENV = ('MIMEO_HEAVY', 'MIMEO_K4_VARIANT', 'MIMEO_QUEUE_SHRINK', 'MIMEO_PACK')
BUILDS = (('k34', {}), ('v1', {'MIMEO_HEAVY': 'v1'}), ('v1_full_planes', {'MIMEO_HEAVY': 'v1', 'MIMEO_K4_VARIANT': '5'}),
          ('v1_walk_all', {'MIMEO_HEAVY': 'v1', 'MIMEO_K4_VARIANT': '1'}))
_cache = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def suites():
    """the families, family C's thresholds resolved from its own HSPs — built once for the module"""
    if 'suites' not in _cache:
        from oracle import oracle as O
        s = G.suites()
        pair = s['C'][0]
        s['C'] = (pair, [{}] + G.c_runs(O.ungapped_hsps(pair.T, pair.Q, 0, O.default_params(chain=0, hspthresh=1500)))[2])
        _cache['suites'] = s
    return _cache['suites']


def expected(name, k):
    """the oracle's HSPs of parameter set k of a family, computed once and shared by the tests"""
    if (name, k) not in _cache:
        from oracle import oracle as O
        pair, runs = suites()[name]
        q, strand = G.query(pair, runs[k])
        _cache[name, k] = O.ungapped_hsps(pair.T, q, strand, O.default_params(chain=0, **G.engine_kw(runs[k])))
    return _cache[name, k]


def _set(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _cmp(got, exp, tag):
    a = np.sort(got[COLS], order=COLS)
    b = np.sort(exp[COLS], order=COLS)
    assert a.size == b.size, (tag, a.size, b.size, _first_difference(a, b))
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (tag, a[bad[:5]], b[bad[:5]])


def _first_difference(a, b):
    sa, sb = set(map(tuple, a.tolist())), set(map(tuple, b.tolist()))
    return 'engine only', sorted(sa - sb)[:3], 'oracle only', sorted(sb - sa)[:3]


def _genomes(eng, pair, runs):
    """one Genome per strand variant of the pair: (target, query) and (target, reverse-complemented query)"""
    return {m: eng.Genome(['t', 'q'], [pair.T, G.revcomp(pair.Q) if m else pair.Q]) for m in {r.get('minus', 0) for r in runs}}


@pytest.mark.parametrize('name', ['A', 'AX', 'B6', 'B6N', 'B6M', 'B78', 'C', 'D', 'E'])
def test_designed_family_equals_the_oracle_under_every_decomposition(eng, monkeypatch, name):
    """every parameter set of the family: K34 (default) and MIMEO_HEAVY=v1 with MIMEO_K4_VARIANT unset / 5 / 1 each equal the
    oracle's HSPs, and give the same bytes and the same number of seed hits as one another"""
    pair, runs = suites()[name]
    gs = _genomes(eng, pair, runs)
    total = 0
    for k, run in enumerate(runs):
        exp = expected(name, k)
        total += exp.size
        strand = 1 if run.get('minus') else 0
        res = {}
        for tag, env in BUILDS:
            _set(monkeypatch, env)
            got = eng.ungapped_hsps(gs[strand], 0, gs[strand], 1, strand, eng.default_params(chain=0, **G.engine_kw(run)))
            res[tag] = (got.tobytes(), eng.stats()['seed_hits'])
            _cmp(got, exp, (name, run, tag))
        _set(monkeypatch, {})
        for tag in res:
            assert res[tag] == res['k34'], (name, run, tag, res[tag][1], res['k34'][1])
    assert total > 0
    for g in gs.values():
        g.close()


def test_family_a_survives_a_repeated_batch(eng, monkeypatch):
    """MIMEO_QUEUE_SHRINK=4000: the queues overflow, the batch is repeated with larger ones, and the HSPs are the same bytes"""
    for name in ('A', 'AX'):
        pair, runs = suites()[name]
        g = eng.Genome(['t', 'q'], [pair.T, pair.Q])
        _set(monkeypatch, {})
        first = eng.ungapped_hsps(g, 0, g, 1, 0, eng.default_params(chain=0))
        assert eng.stats()['queue_reruns'] == 0
        _set(monkeypatch, {'MIMEO_QUEUE_SHRINK': '4000'})
        again = eng.ungapped_hsps(g, 0, g, 1, 0, eng.default_params(chain=0))
        reruns = eng.stats()['queue_reruns']
        _set(monkeypatch, {})
        assert reruns > 0, (name, reruns)
        assert first.tobytes() == again.tobytes(), name
        _cmp(again, expected(name, 0), (name, 'rerun'))
        g.close()


def test_the_pre_filter_was_really_on(eng, monkeypatch):
    """family C at the default parameters: the filter dismisses most seed hits (those of the random flanks) — so the equalities
    above were reached WITH it, not by walking everything — and the decomposition without a filter sees the same hits"""
    pair, runs = suites()['C']
    g = eng.Genome(['t', 'q'], [pair.T, pair.Q])
    counts = {}
    for tag, env in (BUILDS[0], BUILDS[3]):
        _set(monkeypatch, env)
        got = eng.ungapped_hsps(g, 0, g, 1, 0, eng.default_params(chain=0))
        st = eng.stats()
        counts[tag] = (st['seed_hits'], st['walked_hits'], got.size)
    _set(monkeypatch, {})
    g.close()
    assert 0 < counts['k34'][1] < counts['k34'][0], counts
    assert counts['k34'][0] == counts['v1_walk_all'][0] and counts['k34'][2] == counts['v1_walk_all'][2] == expected('C', 0).size, counts


def _cut_genome(eng, cuts):
    n = len(cuts)
    return eng.Genome(['t%d' % i for i in range(n)] + ['q%d' % i for i in range(n)], [t for t, _ in cuts] + [q for _, q in cuts])


def _oracle_pairs(cuts, idx, **params):
    from oracle import oracle as O
    O.lib()
    return oracle_pool.run([(lambda t, q: O.align_pair(t, q, O.default_params(**params)), cuts[i][0].tobytes(), cuts[i][1].tobytes())
                            for i in idx], cap=16)


def _cmp_pair(got, exp, t, q, tag):
    a = np.sort(got[(got['tid'] == t) & (got['qid'] == q)][ACOLS], order=ACOLS)
    b = np.sort(exp[ACOLS], order=ACOLS)
    assert a.size == b.size and (a == b).all(), (tag, t, q, a, b)
    return a.size


def test_one_batched_call_over_the_cut_out_cases(eng, monkeypatch):
    """cases of families A, AX and B6 as scaffold pairs of their own (gapfree_cases.batched_cutouts: every fifth and all of
    family_ends; all 1628 took 27 s), the copy flush with both ends — every walk ends at a sequence end, many frames hang over
    it — all in one Genome and one align_pairs call without the gapped stage.  The oracle sees all of family_ends — the walks
    that run out of sequence after 20..26 steps to the left and 1..7 to the right exist only there — and every fifth of the
    other pairs (on threads, while the device works; all 342 pairs of the call cost it 20 s).  (case, case) pairs are no cross product, so the call runs one unit per pair with or without MIMEO_PACK=0 —
    asserted, and the bytes must be the same; packed against unpacked is the next test."""
    from oracle import oracle as O
    O.lib()
    cuts, checked = G.batched_cutouts(suites())
    n = len(cuts)
    prm = dict(gapped=0, hspthresh=1500)
    pending = oracle_pool.start([(lambda t, q: O.align_pair(t, q, O.default_params(**prm)), cuts[i][0].tobytes(), cuts[i][1].tobytes())
                                 for i in checked], cap=16)
    g = _cut_genome(eng, cuts)
    pairs = [(i, n + i) for i in range(n)]
    _set(monkeypatch, {})
    got = eng.align_pairs(g, None, pairs, eng.default_params(**prm))
    assert eng.stats()['super_units'] == 0
    _set(monkeypatch, {'MIMEO_PACK': '0'})
    unpacked = eng.align_pairs(g, None, pairs, eng.default_params(**prm))
    _set(monkeypatch, {})
    exp = pending.results()
    assert got.tobytes() == unpacked.tobytes()
    rows = sum(_cmp_pair(got, e, i, n + i, 'cut-out') for i, e in zip(checked, exp))
    assert rows >= len(checked) and got.size >= n, (rows, len(checked), got.size, n)
    g.close()


def test_cut_out_cases_through_super_scaffolds_and_spacers(eng, monkeypatch):
    """a full cross product — what the packed path takes: 40 cut-out targets x 40 cut-out queries run as super-scaffolds with
    spacers between the members, whose ends the designed copies touch.  The pairs (case, case) equal the oracle; every pair
    equals the unit-per-pair path (MIMEO_PACK=0) byte for byte."""
    cuts = G.batched_cutouts(suites())[0]
    cuts = cuts[5::len(cuts) // 40][:40]
    n = len(cuts)
    g = _cut_genome(eng, cuts)
    pairs = [(i, n + j) for i in range(n) for j in range(n)]
    _set(monkeypatch, {})
    got = eng.align_pairs(g, None, pairs, eng.default_params(gapped=0, hspthresh=1500))
    assert eng.stats()['super_units'] > 0
    _set(monkeypatch, {'MIMEO_PACK': '0'})
    unpacked = eng.align_pairs(g, None, pairs, eng.default_params(gapped=0, hspthresh=1500))
    assert eng.stats()['super_units'] == 0
    _set(monkeypatch, {})
    assert got.tobytes() == unpacked.tobytes()
    rows = sum(_cmp_pair(got, e, i, n + i, 'packed') for i, e in enumerate(_oracle_pairs(cuts, range(n), gapped=0, hspthresh=1500)))
    assert rows >= n, rows
    g.close()
