"""The care-position count of the seed filters on the device (mimeo_amd/csrc/seed_window.h: one carry-save network of three-input
boolean functions behind K34's pre-filter, the sharp filter at its walk-queue flush, and the walk kernel's left_masks / filter_left).

tests/test_gpu_flush_filter.py holds the records to the oracle's under the four decompositions of the stage and the counts to
inequalities (a filter that passes too much on would go unseen there).  Here the COUNTS are pinned: on two 100 kbp scaffolds
with planted repeat copies at 85 - 95 % identity (about 8 000 seed hits per unit, windows at every offset to the word
boundaries, heads and followers) the `walk queue` and `walked` figures of the MIMEO_K4_STATS line equal the number of seed hits
that the numpy restatement of the filters (tests/flush_filter_spec.py) passes, for the plus and the minus strand and the self
unit, with and without the transition rule:
  default             walk queue = walked = hits the cheap and then the sharp filter pass;
  MIMEO_K34_DEBUG=32  walk queue = hits the cheap filter passes; walked = those the walk kernel's own filter passes too;
  MIMEO_HEAVY=v1      walked = hits the walk kernel's filter passes (no walk queue: it looks at every seed hit).
The walk kernel's filter (k4_device.h: hit_needs_walk<16>) is the sharp filter but for the left steps 64 .. 79: their windows
are tested at the eight care positions nearest the frame, and a column in front of the frame's first word (which depends on the
target position's offset in its word) counts as identical.  The records equal the oracle's under every build."""
import re

import numpy as np
import pytest

from tests import flush_filter_spec as F

pytestmark = pytest.mark.gpu

HCOLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
ENV = ('MIMEO_HEAVY', 'MIMEO_K4_VARIANT', 'MIMEO_QUEUE_SHRINK', 'MIMEO_PACK', 'MIMEO_K34_DEBUG', 'MIMEO_K4_STATS')
BUILDS = (('default', {}), ('no_flush_filter', {'MIMEO_K34_DEBUG': '32'}), ('v1', {'MIMEO_HEAVY': 'v1'}))
UNITS = ((0, 1, 0), (0, 1, 1), (0, 0, 0))      # plus strand, minus strand, a scaffold against itself
ACGT = np.frombuffer(b'ACGT', np.uint8)
COMP = np.zeros(256, np.uint8)
COMP[list(b'ACGT')] = list(b'TGCA')
CARE8_HIGH = np.array([7, 8, 11, 13, 15, 16, 17, 18])


def _scaffolds():
    """two scaffolds of 100 kbp: in each, three copies of four families of 300 - 900 bases, one of the three reverse-complemented (so
    that either strand meets copies), 5 - 15 % of a copy's bases substituted: about 8 000 seed hits between unrelated bases
    and some 4 000 inside copies"""
    rng = np.random.default_rng(2310)
    fams = [rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in (300, 500, 700, 900)]
    seqs = []
    for _ in range(2):
        s = ACGT[rng.integers(0, 4, size=100_000, dtype=np.uint8)].copy()
        for k in range(12):
            c = fams[k % 4].copy()
            at = int(rng.integers(0, s.size - c.size))
            m = rng.random(c.size) < rng.uniform(0.05, 0.15)
            c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
            s[at:at + c.size] = COMP[ACGT[c][::-1]] if 4 <= k < 8 else ACGT[c]
        seqs.append(s)
    return seqs


def _walk_kernel_needs_walk(a, b, nflag, tpos, transitions):
    """hit_needs_walk<16>: flush_filter_spec.sharp_needs_walk with the late boundaries as the walk kernel tests them"""
    x = a ^ b
    cg = (a == 1) | (a == 2)
    lstops, lub = F._sharp_side(x, cg, F.LEFT_BLOCKS, 910)
    rstops, rub = F._sharp_side(x, cg, F.RIGHT_BLOCKS, 910)
    veto = np.zeros(a.shape[0], dtype=bool)
    for s in range(64):
        veto |= F._possible(x, 108 - s, F.CARE, transitions, True)
    # the frame's first word starts 64 + (tpos mod 32) bases in front of the seed start (column 109)
    xm = np.where(np.arange(F.FRAME)[None, :] < (45 - (tpos & 31))[:, None], 0, x)
    late = np.zeros(a.shape[0], dtype=bool)
    for s in range(64, 80):
        late |= F._possible(xm, 108 - s, CARE8_HIGH, transitions, True)
    veto |= late & ~lstops[3]
    return nflag | ~(lstops[4] & rstops[3] & (lub + rub < 3000) & ~veto)


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


@pytest.fixture(scope='module')
def expected():
    """(unit, transitions) -> the oracle's HSPs and the counts the three builds must report; computed once"""
    from oracle import oracle as O
    seqs = _scaffolds()
    out = {}
    for t, q, strand in UNITS:
        T = seqs[t].tobytes()
        Q = COMP[seqs[q][::-1]].tobytes() if strand else seqs[q].tobytes()
        for tr in (1, 0):
            prm = O.default_params(chain=0, transitions=tr)
            h = O.seed_hits(seqs[t].tobytes(), seqs[q].tobytes(), strand, prm)
            tp, qp = h['tpos'].astype(np.int64), h['qpos'].astype(np.int64)
            if t == q and not strand:               # the main diagonal of a self unit never enters the filters
                keep = tp != qp
                tp, qp = tp[keep], qp[keep]
            a, b, nflag = F.frames(T, Q, list(zip(tp.tolist(), qp.tolist())))
            cheap = F.cheap_needs_walk(a, b, nflag, transitions=bool(tr))
            sharp = F.sharp_needs_walk(a, b, nflag, transitions=bool(tr))
            walk = _walk_kernel_needs_walk(a, b, nflag, tp, bool(tr))
            out[(t, q, strand, tr)] = {
                'hsps': np.sort(O.ungapped_hsps(seqs[t].tobytes(), seqs[q].tobytes(), strand, prm)[HCOLS], order=HCOLS),
                'hits': int(tp.size),
                'default': (int((cheap & sharp).sum()), int((cheap & sharp).sum())),
                'no_flush_filter': (int(cheap.sum()), int((cheap & walk).sum())),
                'v1': (0, int(walk.sum())),
            }
    return seqs, out


def _set(monkeypatch, env):
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize('transitions', [1, 0])
@pytest.mark.parametrize('unit', UNITS, ids=['plus', 'minus', 'self'])
def test_counts_and_records_of_the_three_builds(eng, expected, monkeypatch, capfd, unit, transitions):
    seqs, exp = expected
    t, q, strand = unit
    e = exp[(t, q, strand, transitions)]
    assert 300 < e['hits'] < 40000 and 0 < e['default'][0] < e['no_flush_filter'][0] < e['hits'], e
    g = eng.Genome(['a', 'b'], seqs)
    try:
        for tag, env in BUILDS:
            _set(monkeypatch, dict(env, MIMEO_K4_STATS='1'))
            capfd.readouterr()
            h = eng.ungapped_hsps(g, t, g, q, strand, eng.default_params(chain=0, transitions=transitions))
            st = eng.stats()
            err = capfd.readouterr().err
            queue = sum(int(x) for x in re.findall(r'walk queue (\d+)', err))
            walked = sum(int(x) for x in re.findall(r'walk queue \d+ walked (\d+)', err))
            listed = sum(int(x) for x in re.findall(r'split pass: (\d+) tiles listed', err))
            print(unit, transitions, tag, 'hits', e['hits'], 'walk queue', queue, 'walked', walked, 'expected', e[tag], 'listed', listed)
            got = np.sort(h[HCOLS], order=HCOLS)
            assert got.size == e['hsps'].size and (got == e['hsps']).all(), (tag, got.size, e['hsps'].size)
            assert st['queue_reruns'] == 0 and listed == 0, (tag, st['queue_reruns'], listed)
            assert (queue, walked) == e[tag], (tag, 'walk queue, walked', (queue, walked), 'expected', e[tag])
            assert st['walked_hits'] == e[tag][1], (tag, st['walked_hits'], e[tag][1])
    finally:
        _set(monkeypatch, {})
        g.close()
    assert e['hsps'].size >= 4
