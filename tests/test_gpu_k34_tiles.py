"""The seed scan (K34, k34_fused.hip) on the designed one-tile sequences of tests/k34_tile_cases.py: every edge of the segment cut, the
chunk prefetch, the probes an aligned tile skips, the neighbour-only count, the listing threshold, the split pass's plan and its two
emitters, the flush between units and the scaffold ends (tests/test_host_k34_tiles.py proves on the CPU that the cases hold them and
that the model's hit total is the oracle's).  Through the C ABI, one unit per case:

* the HSPs (chain = 0), sorted, are the oracle's over tstart, qstart, length, score, raw_score;
* the `seed_hits` statistic — the sum of the pairs the chunk visits enumerate — is the model's total: a pair dropped or doubled at a
  segment, half or part boundary shows even when its diagonal still yields the same HSP;
* `mimeo_seed_hits` (K2 + K3) gives the oracle's hits: an index fault is told from an enumeration fault;
* the `[k34] split pass` line of MIMEO_K4_STATS names the model's number of listed tiles and of parts;
* under MIMEO_HEAVY=v1 (hit array + K4, the other decomposition) the HSP bytes and `seed_hits` are the same.
The batch family goes through `align_pairs(gapped=0)`, 18 units in one call.  Everything is integer: no tolerance."""
import re

import numpy as np
import pytest

from tests import k34_tile_cases as W

pytestmark = pytest.mark.gpu

HCOLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
ACOLS = ['tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand']
ENV = ('MIMEO_HEAVY', 'MIMEO_K4_VARIANT', 'MIMEO_QUEUE_SHRINK', 'MIMEO_PACK', 'MIMEO_K34_DEBUG', 'MIMEO_K4_STATS', 'MIMEO_BATCH_UNITS', 'MIMEO_MIRROR')


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def _set(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _split_lines(err):
    """(tiles listed, parts) of every `[k34] split pass` line"""
    return [(int(a), int(b)) for a, b in re.findall(r'\[k34\] split pass: (\d+) tiles listed of \d+, (\d+) parts', err)]


def _hit_keys(h):
    return np.sort(h['tpos'].astype(np.uint64) << np.uint64(32) | h['qpos'].astype(np.uint64))


@pytest.mark.parametrize('family', list(W.FAMILIES))
def test_designed_tiles(eng, monkeypatch, capfd, family):
    from oracle import oracle as O
    names = W.FAMILIES[family]
    cases = [W.case(family, n) for n in names]
    g = eng.Genome(['%s.%s' % (n, s) for n in names for s in 'tq'], [a for c in cases for a in (c.T, c.Q)])
    try:
        for k, c in enumerate(cases):
            m, tag = W.model(family, c.name), (family, c.name)
            t, q = 2 * k, 2 * k + 1
            prm = eng.default_params(chain=0, transitions=c.transitions)
            oprm = O.default_params(chain=0, transitions=c.transitions)
            _set(monkeypatch, {'MIMEO_K4_STATS': '1'})
            capfd.readouterr()
            got = eng.ungapped_hsps(g, t, g, q, c.strand, prm)
            hits = eng.stats()['seed_hits']
            lines = _split_lines(capfd.readouterr().err)
            exp = O.ungapped_hsps(c.T.tobytes(), c.Q.tobytes(), c.strand, oprm)
            print(family, c.name, 'seed hits', hits, 'model', m.hits, 'hsps', got.size, 'oracle', exp.size, 'split pass', lines, 'model', m.split_line())
            assert hits == m.hits, (tag, 'seed hits', hits, m.hits)
            a, b = np.sort(got[HCOLS], order=HCOLS), np.sort(exp[HCOLS], order=HCOLS)
            assert a.size == b.size and (a == b).all(), (tag, 'hsps', a.size, b.size)
            nlisted, nparts = m.split_line()
            if nlisted:
                assert lines and all(l == (nlisted, nparts) for l in lines), (tag, lines, (nlisted, nparts))
            else:
                assert all(l == (0, 0) for l in lines), (tag, lines)
            # the index and the join alone
            _set(monkeypatch, {})
            sh = eng.seed_hits(g, t, g, q, c.strand, prm)
            oh = O.seed_hits(c.T.tobytes(), c.Q.tobytes(), c.strand, oprm)
            assert sh.size == oh.size and np.array_equal(_hit_keys(sh), _hit_keys(oh)), (tag, 'mimeo_seed_hits', sh.size, oh.size)
            # the other decomposition
            _set(monkeypatch, {'MIMEO_HEAVY': 'v1'})
            v1 = eng.ungapped_hsps(g, t, g, q, c.strand, prm)
            v1_hits = eng.stats()['seed_hits']
            _set(monkeypatch, {})
            assert v1.tobytes() == got.tobytes(), (tag, 'MIMEO_HEAVY=v1', v1.size, got.size)
            assert v1_hits == hits, (tag, 'MIMEO_HEAVY=v1 seed hits', v1_hits, hits)
    finally:
        _set(monkeypatch, {})
        g.close()


def test_batch_of_eighteen_units(eng, monkeypatch, capfd):
    """all nine pairs of three short scaffolds, both strands, in one call.  With MIMEO_MIRROR=0 every pair and strand is a unit that runs
    the seed scan: the parts of the four listed tiles belong to four units, the persistent workgroups of the split pass pass from one
    unit to the next with pairs staged; the records pair by pair are the oracle's, `seed_hits` is the sum of the 18 models, the split
    pass line the sum of their plans.  The default (a plus-strand unit also serves its transpose, which has as many hits: of the units
    (t, q, +) and (q, t, +) one runs no scan) and MIMEO_HEAVY=v1 return the same records."""
    from oracle import oracle as O
    S = W.batch()
    g = eng.Genome(['s0', 's1', 's2'], S)
    pairs = [(t, q) for t in range(3) for q in range(3)]
    models = {(t, q, s): W.Model(S[t], S[q], s, 1) for t, q in pairs for s in (0, 1)}
    try:
        res = {}
        for tag, env in (('no_mirror', {'MIMEO_MIRROR': '0', 'MIMEO_K4_STATS': '1'}), ('default', {}), ('v1', {'MIMEO_MIRROR': '0', 'MIMEO_HEAVY': 'v1'})):
            _set(monkeypatch, env)
            capfd.readouterr()
            al = eng.align_pairs(g, None, pairs, eng.default_params(gapped=0))
            res[tag] = (al, eng.stats()['seed_hits'], _split_lines(capfd.readouterr().err))
        _set(monkeypatch, {})
        got, hits, lines = res['no_mirror']
        want_hits = sum(m.hits for m in models.values())
        want_line = (sum(m.split_line()[0] for m in models.values()), sum(m.split_line()[1] for m in models.values()))
        print('batch: seed hits', hits, 'model', want_hits, 'split pass', lines, 'model', want_line, 'records', got.size, 'default seed hits', res['default'][1])
        assert hits == want_hits
        assert want_line[0] == len(W.BATCH_LISTED_UNITS) and (sum(a for a, _ in lines), sum(b for _, b in lines)) == want_line, (lines, want_line)
        rows = 0
        for t, q in pairs:
            exp = O.align_pair(S[t].tobytes(), S[q].tobytes(), O.default_params(gapped=0))
            a = np.sort(got[(got['tid'] == t) & (got['qid'] == q)][ACOLS], order=ACOLS)
            b = np.sort(exp[ACOLS], order=ACOLS)
            assert a.size == b.size and (a == b).all(), (t, q, a.size, b.size)
            rows += b.size
        assert rows == got.size > 0
        for tag in ('default', 'v1'):
            assert res[tag][0].tobytes() == got.tobytes(), (tag, res[tag][0].size, got.size)
        assert res['v1'][1] == hits
        assert res['default'][1] == want_hits - sum(models[t, q, 0].hits for t, q in pairs if t < q)
    finally:
        _set(monkeypatch, {})
        g.close()
