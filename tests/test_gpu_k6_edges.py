"""The DP cascade of K6 on DESIGNED pairs (tests/k6_cases.py): halves that a register kernel keeps or loses by one strip, query
and target ends at every residue of the strip widths, 65 534 and 65 535 rows, window slides of several strips, shortcuts whose
last word is partial, later cells that return to the best score — what the random pairs of test_gpu_align.py leave to chance.
That the families reach those edges is asserted on the CPU (tests/test_host_k6_edges.py), where the oracle is also held to a band
walk of its own.  Here the engine must equal the oracle on every case, give the same records under every layout, and go the way
through the cascade that the walk predicts (MIMEO_K6_STATS)."""
import collections

import numpy as np
import pytest

from tests import k6_cases as K
from tests import oracle_pool

pytestmark = pytest.mark.gpu

COLS = oracle_pool.ACOLS
ENV = ('MIMEO_K6_SCORE_CAP', 'MIMEO_K6_BMAX', 'MIMEO_K6_STATS')
_cache = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def _okey(c):
    return c.T, c.Q, tuple(sorted(c.oracle_kw().items()))


def oracle_start(cases):
    """the oracle's records of the cases that have none yet, on threads while the device works: call the result to wait"""
    from oracle import oracle as O
    O.lib()
    res = _cache.setdefault('oracle', {})
    todo = {}
    for c in cases:
        if _okey(c) not in res:
            todo.setdefault(_okey(c), c)
    pending = oracle_pool.start([(lambda c: O.align_pair(c.T, c.Q, O.default_params(**c.oracle_kw())), c) for c in todo.values()], cap=16)
    return lambda: res.update(zip(todo, pending.results()))


def family(name):
    if name not in _cache:
        _cache[name] = K.FAMILIES[name]()
    return _cache[name]


# tests per family, case k of a family in part k mod n: the oracle takes 0.2 s of a CPU per case, however small, and 0.6 s for a
# 66 kbp pair of family R, whose sixteen long cases come first — one to a part
NPARTS = {'W': 4, 'Q': 12, 'R': 16}
PARTS = [(n, k) for n in sorted(K.FAMILIES) for k in range(NPARTS.get(n, 1))]
_ids = ['%s%d' % p for p in PARTS]


def part_of(name, part):
    return family(name)[part::NPARTS.get(name, 1)]


def _chunks():
    """the cases of the layout tests, a few per test: a fixed fifth of W, Q, S and I in three parts, all of R in the parts above"""
    fifth = [c for n in 'WQSI' for c in family(n)[::5]]
    out = {'fifth%d' % k: fifth[k::3] for k in range(3)}
    out.update({'R%02d' % k: part_of('R', k) for k in range(NPARTS['R'])})
    return out


CHUNKS = sorted(_chunks())


def _set(monkeypatch, case, **env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if case.cap:
        monkeypatch.setenv('MIMEO_K6_SCORE_CAP', str(case.cap))
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _params(eng, c):
    return eng.default_params(strand=2 if c.minus else 1, **c.params)


def _genome(eng, c, genomes):
    key = (c.T, c.Q)
    if key not in genomes:
        genomes[key] = eng.Genome(['t', 'q'], [c.T, c.Q])
    return genomes[key]


def _cmp(got, exp, tag):
    a, b = got[COLS], exp[COLS]
    assert a.size == b.size, (tag, a.size, b.size, a[:3], b[:3])
    bad = np.flatnonzero(a != b)
    assert bad.size == 0, (tag, a[bad[:3]], b[bad[:3]])


def first_run(eng, monkeypatch, cases):
    """the records of every case from a plain align_pair call, kept for the layout tests"""
    runs = _cache.setdefault('runs', {})
    genomes = {}
    for c in cases:
        if c.name not in runs:
            _set(monkeypatch, c)
            runs[c.name] = eng.align_pair(_genome(eng, c, genomes), 0, _genome(eng, c, genomes), 1, _params(eng, c))
            assert not eng.failed_pairs(), c.name
    for g in genomes.values():
        g.close()
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    return runs


@pytest.mark.parametrize('name,part', PARTS, ids=_ids)
def test_designed_family_equals_the_oracle(eng, monkeypatch, name, part):
    """every case through engine.align_pair: the oracle's records, in the oracle's order, on every column"""
    cases = part_of(name, part)
    wait = oracle_start(cases)
    runs = first_run(eng, monkeypatch, cases)
    wait()
    for c in cases:
        exp = _cache['oracle'][_okey(c)]
        assert exp.size >= 1, c.name
        _cmp(runs[c.name], exp, c.name)


@pytest.mark.parametrize('chunk', CHUNKS)
def test_layouts_one_call_over_all_scaffolds(eng, monkeypatch, chunk):
    """the chunk's few cases as scaffolds of one Genome, through align_pairs instead of align_pair: one call for every set of
    parameters among them, so most calls carry one or two pairs (the W cases all differ in y-drop).  The records of each pair are
    those of its own call.  Rounds shared by many long halves: test_layouts_the_long_halves_of_r_in_one_call"""
    cases = _chunks()[chunk]
    runs = first_run(eng, monkeypatch, cases)
    seqs, index = [], {}
    for c in cases:
        for s in (c.T, c.Q):
            if s not in index:
                index[s] = len(seqs)
                seqs.append(s)
    g = eng.Genome(['s%d' % i for i in range(len(seqs))], seqs)
    groups = collections.defaultdict(list)
    for c in cases:
        groups[(c.minus, c.cap, tuple(sorted(c.params.items())))].append(c)
    for members in groups.values():
        _set(monkeypatch, members[0])
        pairs = [(index[c.T], index[c.Q]) for c in members]
        got = eng.align_pairs(g, None, pairs, _params(eng, members[0]))
        assert not eng.failed_pairs(), members[0].name
        for c, (t, q) in zip(members, pairs):
            mine = got[(got['tid'] == t) & (got['qid'] == q)]
            _cmp(mine, runs[c.name], c.name)
    _set(monkeypatch, K.Case('none', b'A', b'A'))
    g.close()


@pytest.mark.parametrize('cap', [None, K.LOW_CAP], ids=['production-cap', 'low-cap'])
def test_layouts_the_long_halves_of_r_in_one_call(eng, monkeypatch, cap):
    """the eight 66 kbp pairs of family R in one Genome and one align_pairs call: their long halves share the rounds — four of
    them leave the lean kernel at row 65 535 together, and under the low cap leave the 2048-column kernel for k6_dp_any together"""
    cases = [c for c in family('R') if c.cap == cap and int(c.name.split('-')[1][1:]) in K.R_LONG]
    assert len(cases) == 8
    runs = first_run(eng, monkeypatch, cases)
    g = eng.Genome(['s%d' % i for i in range(16)], [s for c in cases for s in (c.T, c.Q)])
    _set(monkeypatch, cases[0])
    got = eng.align_pairs(g, None, [(2 * k, 2 * k + 1) for k in range(8)], _params(eng, cases[0]))
    assert not eng.failed_pairs()
    for k, c in enumerate(cases):
        _cmp(got[(got['tid'] == 2 * k) & (got['qid'] == 2 * k + 1)], runs[c.name], c.name)
    _set(monkeypatch, K.Case('none', b'A', b'A'))
    g.close()


@pytest.mark.parametrize('chunk', CHUNKS)
def test_layouts_one_anchor_per_round(eng, monkeypatch, chunk):
    """MIMEO_K6_BMAX=1: the same records"""
    cases = _chunks()[chunk]
    runs = first_run(eng, monkeypatch, cases)
    genomes = {}
    for c in cases:
        _set(monkeypatch, c, MIMEO_K6_BMAX='1')
        g = _genome(eng, c, genomes)
        got = eng.align_pair(g, 0, g, 1, _params(eng, c))
        assert not eng.failed_pairs(), c.name
        assert got.tobytes() == runs[c.name].tobytes(), c.name
    _set(monkeypatch, K.Case('none', b'A', b'A'))
    for g in genomes.values():
        g.close()


@pytest.mark.parametrize('chunk', CHUNKS + ['T'])
def test_layouts_with_paths(eng, monkeypatch, chunk):
    """paths=True: k6_trace runs every half again through the band DP it shares with k6_dp_any and treats a half that ends
    elsewhere as an engine error — no failed pair, the same records; the blocks of the W and Q cases are the path oracle's.
    Family T rides along whole: its ties are what two runs of one DP could settle differently"""
    from tests import paths_oracle as PO
    from tests.test_gpu_paths import check_against_oracle
    PO.lib()
    cases = family('T') if chunk == 'T' else _chunks()[chunk]
    checked = [c for c in cases if c.name[0] in 'WQT']
    pending = oracle_pool.start([(lambda c: PO.align_paths(c.T, c.Q, 0, **c.oracle_kw()), c) for c in checked], cap=16)
    runs = first_run(eng, monkeypatch, cases)
    genomes, out = {}, {}
    for c in cases:
        _set(monkeypatch, c)
        g = _genome(eng, c, genomes)
        out[c.name] = eng.align_pairs(g, None, [(0, 1)], _params(eng, c), paths=True)
        assert not eng.failed_pairs(), (c.name, eng.last_error())
        _cmp(out[c.name][0], runs[c.name], c.name)
    _set(monkeypatch, K.Case('none', b'A', b'A'))
    for g in genomes.values():
        g.close()
    for c, (orecs, ext) in zip(checked, pending.results()):
        check_against_oracle(*out[c.name], orecs, ext, c.name)


def _stats(err):
    """the first `[k6] jobs` line of a call's MIMEO_K6_STATS output and its per-job lines"""
    lines = err.splitlines()
    k = next(i for i, l in enumerate(lines) if l.startswith('[k6] jobs'))
    head = lines[k]
    d = dict(jobs=int(head.split('jobs ')[1].split()[0]), shortcut=int(head.split('shortcut ')[1].split()[0]),
             rebased=int(head.split('k6_dp_any: ')[1].split(')')[0]), rows_max=int(head.split(' max ')[1].split()[0]),
             hist=[int(x) for x in head.split('>=1024:')[1].split()],
             fine=[int(x) for x in lines[k + 1].split('from 448:')[1].split()], job={})
    for l in lines[k + 2:k + 2 + d['jobs']]:
        assert l.startswith('  [k6] job '), l
        f = l.split(':')[1].split()
        d['job'][int(f[1])] = {f[i]: int(f[i + 1]) for i in range(2, len(f), 2)}
    return d, head


@pytest.mark.parametrize('name,part', PARTS, ids=_ids)
def test_every_half_goes_the_way_the_walk_predicts(eng, monkeypatch, capfd, name, part):
    """one anchor per round with statistics: the first round's two jobs are the halves of the top anchor.  The shortcut count, the
    longest half, the rebased count and the band buckets are the walk's; and each half came back with the walk's rows, best
    cell and band as the predicted kernel reports it — a multiple of 14 up to 882 from the lean kernel, of 32 up to 2016 from
    the 2048-column kernel, the exact width from k6_dp_any — which tells the three apart"""
    cases = part_of(name, part)
    K.prepare(cases, threads=16)
    genomes = {}
    for c in cases:
        _, hs = c.analyse()
        _set(monkeypatch, c, MIMEO_K6_BMAX='1', MIMEO_K6_STATS='1')
        g = _genome(eng, c, genomes)
        capfd.readouterr()
        eng.align_pair(g, 0, g, 1, _params(eng, c))
        d, head = _stats(capfd.readouterr().err)
        routes = [r for _, r in hs]
        live = [r for r in routes if r['kernel'] != 'shortcut']
        assert d['jobs'] == 2, (c.name, head)
        assert d['shortcut'] == 2 - len(live), (c.name, head)
        assert d['rows_max'] == max([r['rows'] for r in live] + [0]), (c.name, head)
        assert d['rebased'] == sum(r['rebases'] > 0 for r in routes), (c.name, head)
        hist, fine = [0] * 9, [0] * 34
        for r in live:
            hist[min(8, r['maxcols'] // 128)] += 1
            fine[min(33, r['maxcols'] // 32)] += 1
        assert d['hist'] == hist and d['fine'] == fine[14:], (c.name, head, hist, fine[14:])
        for (w, r), direction in zip(hs, (-1, 1)):
            j = d['job'][direction]
            want = dict(rows=r['rows'], maxcols=r['maxcols'], i=w.best[1], j=w.best[2], rebased=int(r['rebases'] > 0))
            assert j == want, (c.name, direction, r['kernel'], j, want)
            m = r['maxcols']
            assert {'lean': m % 14 == 0 and m <= 882, 'wide': m % 32 == 0 and m <= 2016}.get(r['kernel'], True), (c.name, r)
    _set(monkeypatch, K.Case('none', b'A', b'A'))
    for g in genomes.values():
        g.close()
