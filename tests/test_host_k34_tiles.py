"""The designed one-tile sequences of tests/k34_tile_cases.py on the CPU: the constants the model states equal those of the sources, the
model's seed-hit total equals the C oracle's on every case (which pins the model, so that the GPU test can trust its per-tile
statements), every case is what it claims to be (the shape it was built for is asserted from the model, not assumed), and the families
hold the edge values they exist for.  No GPU."""
import os
import re
import time

import pytest

from tests import k34_tile_cases as W

_T0 = time.perf_counter()
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mimeo_amd', 'csrc')


def _constant(text, name):
    m = re.search(r'\b%s = (\d+)' % name, text)
    assert m, 'no `%s = <number>` in the source: the model of tests/k34_tile_cases.py states it and must be told where it went' % name
    return int(m.group(1))


def test_the_constants_of_the_model_are_those_of_the_sources():
    """a retune fails here, with the name of the constant, and does not silently move every case off its edge"""
    common = open(os.path.join(CSRC, 'common.h')).read()
    k34 = open(os.path.join(CSRC, 'k34_fused.hip')).read()
    util = open(os.path.join(CSRC, 'device_util.h')).read()
    for name in ('SEED_LEN', 'SEED_WEIGHT', 'TILE_WORDS'):
        assert _constant(common, name) == getattr(W, name), name
    assert re.search(r'NBUCKET = 1u << 24;', common) and re.search(r'NTILE = NBUCKET / TILE_WORDS;', common) and W.NTILE == (1 << 24) // W.TILE_WORDS
    for name in ('TCH', 'HEAVY_HITS', 'PART_HITS', 'DENSE_MIN', 'RING', 'QSEG_FIRST', 'QSEG_HEAVY'):
        assert _constant(k34, name) == getattr(W, name), name
    assert 'k34_scan_extend<512, QSEG_FIRST, false>' in k34 and 'k34_scan_extend<512, QSEG_HEAVY, true>' in k34 and W.WAVES == 512 // 64
    assert '(nT + 511u) / 512u' in k34 and '1u << 20' in k34 and '& ~63u' in k34          # k34_plan's own numbers, restated in Model.plan
    # pext12 takes the care positions of 1110100110010101111 in order: (mask, shift) pairs of device_util.h
    body = util[util.index('uint32_t pext12('):]
    body = body[:body.index('}')]
    bits = []
    for sh, mask in [(0, int(re.search(r'\(x & (0x[0-9A-Fa-f]+)u\)', body).group(1), 16))] + \
            [(int(s), int(m, 16)) for s, m in re.findall(r'\(\(x >> (\d+)\) & (0x[0-9A-Fa-f]+)u\)', body)]:
        bits += [(b, b + sh) for b in range(12) if mask >> b & 1]
    assert [src for _, src in sorted(bits)] == list(W.CARE)


def _oracle_hits(c):
    from oracle import oracle as O
    return O.seed_hits(c.T.tobytes(), c.Q.tobytes(), c.strand, O.default_params(transitions=c.transitions))


@pytest.mark.parametrize('family', list(W.FAMILIES))
def test_model_hit_total_is_the_oracles(family):
    for name in W.FAMILIES[family]:
        c, m = W.case(family, name), W.model(family, name)
        h = _oracle_hits(c)
        assert m.hits == h.size, (family, name, m.hits, h.size)
        if h.size < 50000:   # and the hits themselves: positions by tile, from the model's entries
            got = set(zip(h['tpos'].tolist(), h['qpos'].tolist()))
            t = c.tiles[0]
            tp, qp = set(m.entries(t, 'T').tolist()), set(m.entries(t, 'Q').tolist())
            assert sum(1 for a, b in got if a in tp and b in qp) == m.tile_hits[t], (family, name)


def check(c, m):
    """the shape `want` states, from the model; returns the line the summary quotes"""
    t, w = c.tiles[0], c.want
    aligned, segs = m.segments(t)
    have = dict(nT=int(m.nT[t]), nQ=int(m.nQ[t]), mid=int(m.mid[t]), sigma=int(m.sigma[t]), est=m.est(t), hits=int(m.tile_hits[t]), fate=m.fate(t),
                nchunks=m.nchunks(t), aligned=aligned, segments=segs, nsegments=len(segs))
    for k, v in have.items():
        if k in w:
            assert v == w[k], (c.family, c.name, k, v, w[k])
    known = set(have)
    if 'kinds' in w:
        assert aligned and m.chunk_kinds(t) == w['kinds'], (c.name, m.chunk_kinds(t))
    if 'idle_waves' in w:   # chunk ch is wavefront ch % WAVES's
        n = m.nchunks(t)
        mine = [len(range(wv, n, W.WAVES)) for wv in range(W.WAVES)]
        assert (mine.count(0), mine.count(1), sum(1 for k in mine if k > 1)) == (w['idle_waves'], w['lone_chunk_waves'], w['wrap_waves']), (c.name, mine)
    if 'plan' in w:
        p = m.plan(t)._asdict()
        assert {k: p[k] for k in w['plan']} == w['plan'], (c.name, p)
    if 'short_last_range' in w:
        p = m.plan(t)
        assert p.pq * p.qlen > m.nQ[t] > (p.pq - 1) * p.qlen, (c.name, p)
    if 'ranges' in w or 'straddle' in w:
        ranges = m.split_pass_pairs(t)[1]
        for n, own in w.get('ranges', ()):
            assert W.Range(n, n, own) in ranges, (c.name, n, own)
        if 'straddle' in w:
            full, before, after = w['straddle']
            assert before + after == full >= W.DENSE_MIN > max(before, after) and min(before, after) > 0
            assert sorted(r.clipped for r in ranges if r.full == full) == sorted((before, after)), (c.name, [r for r in ranges if r.full == full])
    for side in ('T', 'Q'):
        if side.lower() + 'pos' in w:
            assert set(w[side.lower() + 'pos']) <= set(m.entries(t, side).tolist()), (c.name, side)
    if 'fates' in w:
        assert {k: m.fate(k) for k in w['fates']} == w['fates'], c.name
    if 'nlisted' in w:
        assert len(m.listed()) == w['nlisted'], (c.name, m.listed())
    if 'est_below' in w:
        assert m.est(t) < w['est_below']
    assert set(w) <= known | {'kinds', 'idle_waves', 'lone_chunk_waves', 'wrap_waves', 'plan', 'short_last_range', 'ranges', 'straddle', 'tpos', 'qpos', 'fates',
                              'nlisted', 'est_below'}, (c.name, set(w))
    return '%s/%s: %s' % (c.family, c.name, m.shape(t))


@pytest.mark.parametrize('family,name', W.CASES, ids=['%s/%s' % c for c in W.CASES])
def test_the_case_is_what_it_was_built_for(family, name):
    c, m = W.case(family, name), W.model(family, name)
    print(check(c, m))
    assert max(c.T.size, c.Q.size) <= 70000 and (max(c.T.size, c.Q.size) <= 25000 or name.startswith('nq-'))
    # the model's own statements agree with each other: the pairs the segment, half and part rules enumerate are the tile's hits
    for t in c.tiles:
        f = m.fate(t)
        if f == W.HERE:
            assert m.first_pass_pairs(t) == m.tile_hits[t], (name, t)
        if f == W.LISTED:
            assert m.split_pass_pairs(t)[0] == m.tile_hits[t], (name, t)
    # not vacuous: hits in the designed tile (none where the case says NOTHING), and the designed tiles hold the case's hits
    t = c.tiles[0]
    if c.want.get('fate') == W.NOTHING:
        assert m.tile_hits[t] == 0 and m.nT[t] and m.nQ[t]
    else:
        assert m.tile_hits[t] >= 1
        assert 10 * sum(int(m.tile_hits[k]) for k in c.tiles) >= 9 * m.hits, (name, [int(m.tile_hits[k]) for k in c.tiles], m.hits)


def _all(family):
    return [(W.case(family, n), W.model(family, n)) for n in W.FAMILIES[family]]


def test_every_family_holds_its_edge_values():
    Q1 = W.QSEG_FIRST
    seg = {}
    for c, m in _all('segments'):
        t = c.tiles[0]
        aligned, segs = m.segments(t)
        seg.setdefault(t, set()).add((int(m.nQ[t]), int(m.mid[t]), aligned, len(segs)))
        assert m.fate(t) == W.HERE
    for t in (0, W.NTILE - 1):
        s = seg[t]
        assert {n for n, _, _, _ in s} >= {Q1 - 1, Q1, Q1 + 1, 2 * Q1, 2 * Q1 + 1}
        assert {(2 * Q1, Q1, True, 2), (2 * Q1, Q1 + 1, False, 2), (2 * Q1 + 1, Q1, False, 3), (Q1 + 1, 0, False, 2), (Q1 + 1, Q1 + 1, False, 2), (Q1 + 1, 1, True, 2)} <= s
        assert any(k >= 6 for _, _, _, k in s)
    assert {c.strand for c, _ in _all('segments')} == {0, 1}

    ch = {}
    for c, m in _all('chunks'):
        t = c.tiles[0]
        ch.setdefault(len(m.segments(t)[1]), {})[int(m.nT[t])] = (c.want['idle_waves'], c.want['lone_chunk_waves'], c.want['wrap_waves'], m.segments(t)[0])
    assert set(ch) == {1, 2, 3}
    for nseg, by_nt in ch.items():
        assert set(by_nt) == {1, 63, 64, 65, 512, 513, 576, 577}
        assert by_nt[1][0] == 7 and by_nt[512][:3] == (0, 8, 0) and by_nt[513][:3] == (0, 7, 1) and by_nt[577][:3] == (0, 6, 2)
        assert all(v[3] == (nseg == 2) for v in by_nt.values())

    hv = {(c.name.rsplit('-tr', 1)[0], c.transitions): m.chunk_kinds(c.tiles[0]) for c, m in _all('halves')}
    for tr in (0, 1):
        assert hv['lower', tr] == [['half'] * 2, ['other'] * 2] and hv['upper', tr] == [['other'] * 2, ['half'] * 2]
        assert hv['on-boundary', tr] == [['half', 'half', 'other', 'other'], ['other', 'other', 'half', 'half']]
        assert hv['in-chunk', tr] == [['half', 'mixed', 'other', 'other'], ['other', 'mixed', 'half', 'half']]

    nb = {(c.name, int(m.tile_hits[c.tiles[0]]), m.fate(c.tiles[0])) for c, m in _all('neighbour')}
    assert {('one-tr1', 1, W.HERE), ('some-tr1', 3, W.HERE), ('twelve-tr1', 12, W.HERE), ('one-tr0', 0, W.NOTHING), ('some-tr0', 0, W.NOTHING),
            ('twelve-tr0', 0, W.NOTHING), ('some-tr1@4095', 3, W.HERE)} <= nb
    assert all(m.sigma[c.tiles[0]] == 0 for c, m in _all('neighbour'))

    ls = {(c.transitions, m.est(c.tiles[0]), int(m.nQ[c.tiles[0]]) > 0xFFFF, m.fate(c.tiles[0])) for c, m in _all('listing')}
    assert {(1, 262132, False, W.HERE), (1, 262145, False, W.LISTED), (0, 262144, False, W.HERE), (0, 262145, False, W.LISTED)} <= ls
    nq = {int(m.nQ[c.tiles[0]]): m.fate(c.tiles[0]) for c, m in _all('listing')}
    assert nq[65535] == W.HERE and nq[65536] == W.LISTED
    assert any(len(m.listed()) == 2 and W.HERE in [m.fate(t) for t in c.tiles] for c, m in _all('listing'))

    plans = {c.name: m.plan(c.tiles[0]) for c, m in _all('split')}
    assert (plans['groups-512'].groups, plans['groups-513'].groups) == (1, 2)
    assert any(p.pt > 1 and p.pq > 1 for p in plans.values()) and any(p.qlen == 64 for p in plans.values()) and any(p.qlen > W.QSEG_HEAVY for p in plans.values())
    c, m = W.case('split', 'dense'), W.model('split', 'dense')
    ranges = m.split_pass_pairs(0)[1]
    for n in (W.DENSE_MIN - 1, W.DENSE_MIN, W.DENSE_MIN + 1):
        assert W.Range(n, n, True) in ranges and W.Range(n, n, False) in ranges
    assert any(r.full >= W.DENSE_MIN > r.clipped for r in ranges)

    for c, m in _all('ends'):
        for side, seq in (('T', c.T), ('Q', c.Q)):
            assert {0, 1, 2, seq.size - 20, seq.size - 19} <= set(m.entries(0, side).tolist()), c.name
    assert {m.fate(0) for _, m in _all('ends')} == {W.HERE, W.LISTED}
    assert any(b'N' in c.Q.tobytes() and b'N' in c.T.tobytes() for c, _ in _all('ends')) and any(c.T.tobytes() != c.T.tobytes().upper() for c, _ in _all('ends'))


def test_the_batch_family():
    """18 units: the model's total of each is the oracle's; tile 0 of the four plus-strand units of scaffolds 0 and 1 is listed and
    nothing else is; a plus-strand unit and its transpose hold the same number of hits (what the shared plus strand relies on).
    Tile 0 of those four units holds 90 % of the call's hits and more: the rest is every window of a self unit meeting itself, the
    flanks' tile 4095 and what random sequence meets by chance"""
    from oracle import oracle as O
    S = W.batch()
    total = designed = 0
    listed, hits = [], {}
    for t, T in enumerate(S):
        for q, Q in enumerate(S):
            for strand in (0, 1):
                m = W.Model(T, Q, strand, 1)
                assert m.hits == O.seed_hits(T.tobytes(), Q.tobytes(), strand).size, (t, q, strand)
                hits[t, q, strand] = m.hits
                total += m.hits
                listed += [(t, q, strand)] * len(m.listed())
                if (t, q, strand) in W.BATCH_LISTED_UNITS:
                    assert m.listed() == [0] and m.split_pass_pairs(0)[0] == m.tile_hits[0]
                    designed += int(m.tile_hits[0])
                if t == q == 2 and strand == 0:
                    assert m.tile_hits[list(W.RY_TILES)].min() > 50 and W.LISTED not in (m.fate(k) for k in W.RY_TILES)
    assert listed == W.BATCH_LISTED_UNITS and len(S) == 3 and max(a.size for a in S) < 5000
    assert all(hits[t, q, 0] == hits[q, t, 0] for t in range(3) for q in range(3))
    print('batch: hits %d, in the designed tiles %d' % (total, designed))
    assert 10 * designed >= 9 * total


def test_zz_the_time_of_this_file():
    print('tests/test_host_k34_tiles.py: %.1f s for %d cases' % (time.perf_counter() - _T0, len(W.CASES)))
    assert len(W.CASES) < 120
