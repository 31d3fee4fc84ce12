"""The sharp filter at the walk-queue flush of K34's first pass (k34_fused.hip: walk_flush; k34_filter.h: pair_needs_walk_sharp).

A pair the first pass stages is looked at once more where the wavefront flushes its staging area — both frames fetched by entry
number, the walk kernel's three proofs in frame coordinates — and only the survivors reach the walk queue, marked so that
k4_walk_batch does not filter them again; the split pass and MIMEO_K34_DEBUG=32 write unmarked entries, which it filters as
before.  Whatever is dismissed where, the HSPs must be the same bytes under four decompositions of the stage: the default,
MIMEO_K34_DEBUG=32 (no flush filter), MIMEO_HEAVY=v1 (stand-alone seed scan + the walk kernel's own filter) and MIMEO_HEAVY=v1
MIMEO_K4_VARIANT=1 (no filter at all: every seed hit is walked) — and the oracle's.  The rule itself is held to the exact walk on
the CPU (tests/test_host_flush_filter.py)."""
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HCOLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
ENV = ('MIMEO_HEAVY', 'MIMEO_K4_VARIANT', 'MIMEO_QUEUE_SHRINK', 'MIMEO_PACK', 'MIMEO_K34_DEBUG', 'MIMEO_K4_STATS')
BUILDS = (('default', {}), ('no_flush_filter', {'MIMEO_K34_DEBUG': '32'}), ('v1', {'MIMEO_HEAVY': 'v1'}),
          ('v1_walk_all', {'MIMEO_HEAVY': 'v1', 'MIMEO_K4_VARIANT': '1'}))
ACGT = np.frombuffer(b'ACGT', np.uint8)


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


def _k4_stats(err):
    """what MIMEO_K4_STATS=1 wrote: (walk-queue entries, tiles the first pass listed for the split pass), summed over the batches"""
    return (sum(int(x) for x in re.findall(r'walk queue (\d+)', err)), sum(int(x) for x in re.findall(r'split pass: (\d+) tiles listed', err)))


def _four_builds(eng, monkeypatch, capfd, g, t, q, strand, extra=None, **kw):
    """one unit under the four builds: tag -> (HSPs, seed hits, walked hits, walk-queue entries, listed tiles, reruns)"""
    out = {}
    for tag, env in BUILDS:
        _set(monkeypatch, dict(env, MIMEO_K4_STATS='1', **(extra or {})))
        capfd.readouterr()
        h = eng.ungapped_hsps(g, t, g, q, strand, eng.default_params(chain=0, **kw))
        st = eng.stats()
        out[tag] = (h, st['seed_hits'], st['walked_hits']) + _k4_stats(capfd.readouterr().err) + (st['queue_reruns'],)
    _set(monkeypatch, {})
    return out


def _same(res, where):
    for tag in res:
        assert res[tag][0].tobytes() == res['default'][0].tobytes(), (where, tag, res[tag][0].size, res['default'][0].size)
        assert res[tag][1] == res['default'][1], (where, tag, 'seed hits', res[tag][1], res['default'][1])


def _oracle(res, T, Q, strand, where, **kw):
    from oracle import oracle as O
    exp = O.ungapped_hsps(T.tobytes(), Q.tobytes(), strand, O.default_params(chain=0, **kw))
    a, b = np.sort(res['default'][0][HCOLS], order=HCOLS), np.sort(exp[HCOLS], order=HCOLS)
    assert a.size == b.size and (a == b).all(), (where, a.size, b.size)
    return b.size


def test_two_scaffolds_with_diverged_repeats_both_strands_and_self(eng, monkeypatch, capfd):
    """two 300 kbp scaffolds, a tenth of them diverged copies (up to 30 %) of six families: the pairs the cheap filter passes are
    mostly copies too far apart to leave an HSP — what the flush filter is there to dismiss.  The default walks no more than the
    build without the flush filter does, and its walk queue is shorter."""
    from mimeo_amd.synth import synth_genome
    names, seqs = synth_genome(31, 600_000, 2, repeat_frac=0.1, families=6, cons_len=(300, 3000), max_div=0.3)
    g = eng.Genome(names, seqs)
    nh = 0
    for t, q, strand in ((0, 1, 0), (0, 1, 1), (0, 0, 0), (0, 0, 1)):
        res = _four_builds(eng, monkeypatch, capfd, g, t, q, strand)
        _same(res, (t, q, strand))
        nh += _oracle(res, seqs[t], seqs[q], strand, (t, q, strand))
        d, n = res['default'], res['no_flush_filter']
        assert 0 < d[2] <= n[2] < d[1], ((t, q, strand), 'walked hits', d[2], n[2], d[1])
        assert 0 < d[3] < n[3], ((t, q, strand), 'walk-queue entries', d[3], n[3])
        assert res['v1_walk_all'][2] == 0 or res['v1_walk_all'][2] >= n[2]
    assert nh > 100
    g.close()


def _plant(rng, dst, at, copy, div):
    c = copy.copy()
    m = rng.random(c.size) < div
    c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
    dst[at:at + c.size] = ACGT[c]


def _edge_pair(seed):
    """a 45 kbp and a 22 kbp scaffold: diverged copies of four families flush with the first and the last base of both, N runs
    inside a copy, touching one and 100 bases from one, a soft-masked stretch of the longer scaffold with two copies planted in it"""
    rng = np.random.default_rng(seed)
    fams = [rng.integers(0, 4, size=int(n), dtype=np.uint8) for n in (240, 400, 700, 1100)]
    seqs = []
    for n, ncopies in ((45_000, 40), (22_000, 24)):
        s = ACGT[rng.integers(0, 4, size=n, dtype=np.uint8)].copy()
        where = []
        for k in range(ncopies):
            f = fams[k % 4]
            at = int(rng.integers(1500, n - 1500 - f.size))
            _plant(rng, s, at, f, rng.uniform(0.02, 0.3))
            where.append((at, f.size))
        _plant(rng, s, 0, fams[1], 0.1)                                      # flush with the first base ...
        _plant(rng, s, n - fams[2].size, fams[2], 0.1)                       # ... and with the last one
        for k, (at, ln) in enumerate(where[:9]):
            if k % 3 == 0: s[at + ln // 2:at + ln // 2 + 7] = ord('N')       # inside a copy
            if k % 3 == 1: s[at + ln:at + ln + 30] = ord('N')                # touching one
            if k % 3 == 2: s[at - 100 - 12:at - 100] = ord('N')              # 100 bases from one
        seqs.append(s)
    # soft-masked: the target role loses the seeds of this stretch (svt plane), which holds two copies of its own
    _plant(rng, seqs[0], 20_500, fams[2], 0.05)
    _plant(rng, seqs[0], 22_000, fams[3], 0.12)
    seqs[0][20_000:24_000] |= 0x20
    return seqs


def test_frames_that_reach_padding_n_and_soft_masked_bases(eng, monkeypatch, capfd):
    """short scaffolds with copies flush with both ends, so that frames hang over the padding on either side; the shorter one as
    target and as query; N inside, beside and near copies (a flagged frame is kept unseen); a soft-masked target"""
    seqs = _edge_pair(77)
    g = eng.Genome(['long', 'short'], seqs)
    nh = 0
    for t, q in ((0, 1), (1, 0), (1, 1)):
        for strand in (0, 1):
            for kw in ({}, {'hspthresh': 1500, 'xdrop': 500}):
                res = _four_builds(eng, monkeypatch, capfd, g, t, q, strand, **kw)
                _same(res, (t, q, strand, kw))
                nh += _oracle(res, seqs[t], seqs[q], strand, (t, q, strand, kw), **kw)
                assert 0 < res['default'][2] < res['default'][1]
    assert nh > 100
    g.close()


def _both_passes_pair(seed):
    """two 200 kbp scaffolds with ordinary diverged repeats and, in both, arrays of 1500 bases of three motifs and of their reverse
    complements — so that either strand of the query meets arrays of its own motifs in the target: a motif's seed words fill
    one tile with 10^6 and more seed hits, far beyond what the first pass keeps to itself (262 144 estimated)"""
    from mimeo_amd.synth import synth_genome
    names, seqs = synth_genome(seed, 400_000, 2, repeat_frac=0.1, families=5, cons_len=(300, 2000), max_div=0.3)
    rng = np.random.default_rng(seed)
    seqs = [s.copy() for s in seqs]
    for s in seqs:
        for motif in ([0], [3], [1, 0], [2, 3], [2, 3, 3], [0, 0, 1]):      # A, T; AC, GT; GTT, AAC
            at = int(rng.integers(1000, s.size - 3000))
            a = np.resize(np.array(motif, dtype=np.uint8), 1500)
            k = rng.random(1500) < 0.02
            a[k] = (a[k] + rng.integers(1, 4, size=int(k.sum()), dtype=np.uint8)) & 3
            s[at:at + 1500] = ACGT[a]
    return names, seqs


@pytest.mark.parametrize('shrink', [None, '4000'])
def test_a_unit_that_uses_both_passes(eng, monkeypatch, capfd, shrink):
    """microsatellite arrays beside ordinary repeats: the split pass's unmarked entries and the first pass's marked ones meet in one
    walk queue; with MIMEO_QUEUE_SHRINK the queues overflow and the batch is repeated"""
    names, seqs = _both_passes_pair(5)
    g = eng.Genome(names, seqs)
    extra = {'MIMEO_QUEUE_SHRINK': shrink} if shrink else None
    for strand in (0, 1):
        res = _four_builds(eng, monkeypatch, capfd, g, 0, 1, strand, extra=extra)
        _same(res, (strand, shrink))
        assert _oracle(res, seqs[0], seqs[1], strand, (strand, shrink)) > 20
        d, n = res['default'], res['no_flush_filter']
        assert d[4] > 0 and n[4] > 0, ('no tile went to the split pass', d[4], n[4])
        assert 0 < d[2] <= n[2] < d[1], ('walked hits', d[2], n[2], d[1])
        if shrink:                  # (the arrays' followers may overflow the queues of the first attempt on their own)
            assert d[5] > 0 and n[5] > 0, ('reruns', d[5], n[5])
    g.close()


def test_the_switch_word_keeps_two_bits_and_refuses_the_rest(eng, monkeypatch):
    """MIMEO_K34_DEBUG: 16 and 32 (and their sum) are the switches that remain, and change no record; any other bit — the timing
    experiments that used to sit in the kernel's loops, or one that never existed — is an error that names the variable, not a
    switch that is silently ignored."""
    rng = np.random.default_rng(34)
    seqs = [ACGT[rng.integers(0, 4, size=2000, dtype=np.uint8)] for _ in range(2)]
    g = eng.Genome(['a', 'b'], seqs)
    prm = eng.default_params(chain=0)
    _set(monkeypatch, {})
    ref = eng.ungapped_hsps(g, 0, g, 1, 0, prm)
    for v in ('16', '32', '48'):
        _set(monkeypatch, {'MIMEO_K34_DEBUG': v})
        assert eng.ungapped_hsps(g, 0, g, 1, 0, prm).tobytes() == ref.tobytes(), v
    for v in ('4', '64'):
        _set(monkeypatch, {'MIMEO_K34_DEBUG': v})
        with pytest.raises(RuntimeError, match='MIMEO_K34_DEBUG'):
            eng.ungapped_hsps(g, 0, g, 1, 0, prm)
    _set(monkeypatch, {})
    assert eng.ungapped_hsps(g, 0, g, 1, 0, prm).tobytes() == ref.tobytes()
    g.close()


def test_the_packed_path(eng, monkeypatch):
    """twelve scaffolds of 30 kbp against themselves: the default runs them as super-scaffolds (frames across spacers of N are
    flagged), and the records equal those of the unit-per-pair path under the round-1 decompositions, and the oracle's for
    three of the pairs.

    Two deliberate departures from what the other tests of this file require.  (1) `seed_hits` is compared among the builds
    that count alike, not among all: a super-scaffold unit also counts the hits between members that are no pair of the call,
    so the packed builds (default, MIMEO_K34_DEBUG=32) agree with each other, and the unit-per-pair builds (the default under
    MIMEO_PACK=0, MIMEO_HEAVY=v1, v1 walking everything) with each other.  (2) `walked_hits(default) <= walked_hits(DEBUG=32)`
    is not required here: a frame with an N in its 192 bases — the spacers — is kept unseen at the flush, while the walk kernel's
    filter looks for N in the 192 bases of its own word-aligned frame, so beside a spacer either build may walk a few hits the
    other does not (127 437 against 127 133 on this genome)."""
    from mimeo_amd.synth import synth_genome
    from oracle import oracle as O
    from tests.oracle_pool import ACOLS
    names, seqs = synth_genome(19, 360_000, 12, repeat_frac=0.15, families=5, cons_len=(300, 1500), max_div=0.25)
    g = eng.Genome(names, seqs)
    pairs = [(t, q) for t in range(12) for q in range(12)]
    prm = dict(gapped=0, hspthresh=2200)
    res = {}
    for tag, env in BUILDS + (('unit_per_pair', {'MIMEO_PACK': '0'}),):
        _set(monkeypatch, dict(env, **({'MIMEO_PACK': '0'} if 'MIMEO_HEAVY' in env else {})))
        al = eng.align_pairs(g, None, pairs, eng.default_params(**prm))
        st = eng.stats()
        res[tag] = (al, st['seed_hits'], st['walked_hits'], st['super_units'])
    _set(monkeypatch, {})
    g.close()
    got = res['default'][0]
    assert got.size > 0
    for tag in res:
        assert res[tag][0].tobytes() == got.tobytes(), tag
    rows = 0
    for t, q in ((0, 1), (5, 5), (11, 2)):
        exp = O.align_pair(seqs[t].tobytes(), seqs[q].tobytes(), O.default_params(**prm))
        a = np.sort(got[(got['tid'] == t) & (got['qid'] == q)][ACOLS], order=ACOLS)
        b = np.sort(exp[ACOLS], order=ACOLS)
        assert a.size == b.size and (a == b).all(), (t, q, a.size, b.size)
        rows += b.size
    assert rows > 0
    assert res['default'][3] > 0 and res['no_flush_filter'][3] > 0 and res['v1'][3] == 0 and res['unit_per_pair'][3] == 0
    assert res['default'][1] == res['no_flush_filter'][1]
    assert res['unit_per_pair'][1] == res['v1'][1] == res['v1_walk_all'][1]
    for tag in ('default', 'no_flush_filter', 'unit_per_pair'):
        assert 0 < res[tag][2] < res[tag][1], (tag, res[tag][1:])
