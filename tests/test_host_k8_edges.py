"""The designed slices of tests/k8_cases.py, proved on the CPU (no GPU): `mask_by_rule` gives the answers worked out by hand, its sums
are those of the other restatement (`oracle.pipeline.tandem_masked`), every wrong rule of the kill table changes the mask of a named
designed slice, the two equivalent rewrites change none, and every family reaches the edge it exists for.  tests/test_gpu_k8_edges.py
then holds the engine's masks to `mask_by_rule` bit for bit.  Integer work throughout: no tolerance."""
import numpy as np
import pytest

from tests import k8_cases as K

FAMILY_NAMES = list(K.FAMILIES)


def cases(family):
    return [(name, K.case(family, name)) for name in K.FAMILIES[family]]


def words(c):
    """mask words per slice, as tandem_masked_device lays them out"""
    return [(len(K.clipped(c, k)) + 31) // 32 for k in range(len(c.iv))]


def test_families_are_the_nine_and_stay_under_the_cost_cap():
    assert FAMILY_NAMES == ['threshold', 'placement', 'neighbours', 'inside', 'letters', 'long', 'pairs', 'band_and_ties', 'wide']
    for f in FAMILY_NAMES:
        assert sum(K.cost(c) for _, c in cases(f)) < K.COST_CAP, f


@pytest.mark.parametrize('family', FAMILY_NAMES)
def test_hand_answers_and_the_other_restatement(family):
    from oracle import pipeline as P
    hands = 0
    for name, c in cases(family):
        exp = K.expected(c)
        for k, m in enumerate(exp):
            s = K.clipped(c, k)
            assert m.dtype == bool and m.size == len(s)
            h = K.hand_mask(c, k)
            if h is not None:
                hands += 1
                assert np.array_equal(m, h), (family, name, k, np.flatnonzero(m != h)[:8].tolist())
            # the other restatement works on seq[start:end] of the whole scaffold, so this also says that the slice alone decides
            ch, a, e = c.iv[k]
            e = min(e, len(c.seqs[ch]))
            other = P.tandem_masked(c.seqs[ch], a, e, *c.params) if a < e else 0
            assert other == int(m.sum()), (family, name, k)
    assert hands or family in ('band_and_ties',), family


def test_kill_table_has_no_survivor():
    """Each wrong rule changes the mask of the designed slices named for it: an engine that had the rule wrong would differ from
    `mask_by_rule` there."""
    assert set(K.KILLERS) == set(K.MUTANTS)
    for mutant in K.MUTANTS:
        assert K.KILLERS[mutant], mutant
        for family, name, k in K.KILLERS[mutant]:
            c = K.case(family, name)
            s = K.clipped(c, k)
            assert not np.array_equal(K.mask_by_rule(s, *c.params), K.mask_by_rule(s, *c.params, mutant=mutant)), (mutant, family, name, k)
    # the runs of N and R are masked nowhere by the rule and everywhere if letters outside ACGT matched each other
    c = K.case('letters', 'letters')
    for k in (0, 1):
        assert K.mask_by_rule(K.clipped(c, k), *c.params, mutant='non_acgt_match').all()


@pytest.mark.parametrize('family', ['placement', 'inside', 'letters', 'pairs', 'band_and_ties'])
def test_two_rewrites_cannot_change_a_mask(family):
    """carry_best_across_reset: a fresh path takes `best` from the cell it restarts in instead of 0 -- but a cell that was reset is
    (0, 0, 0), its best is 0 already.  mark_from_mend: a new best marks [max(mend, start), j] instead of [start, j], mend = the end of
    the path's last marking -- but start never changes along a path and every earlier marking of the path began at start, so
    [start, mend) is marked already and the union is the same.  Checked where paths restart and mark again most often."""
    for name, c in cases(family):
        exp = K.expected(c)
        for rewrite in K.REWRITES:
            for k, m in enumerate(K.expected(c, rewrite)):
                assert np.array_equal(m, exp[k]), (rewrite, family, name, k)


# ---- one predicate per family: the edge is reached ---------------------------------------------------------------------------------
def test_threshold_edges():
    for delta in (7, 0):
        for name, periods, mp in (('to64', (1, 2, 4, 5, 31, 32, 33, 50, 63, 64), 64), ('to130', (65, 66, 127, 128, 129, 130), 130)):
            c = K.case('threshold', '%s_delta%d' % (name, delta))
            assert c.periods == periods and c.params == (2, 7, 50, mp, delta)
            for i, p in enumerate(periods):
                short, full = K.clipped(c, 2 * i), K.clipped(c, 2 * i + 1)
                assert (len(short), len(full)) == (p + 24, p + 25) and full[:-1] == short
                assert all(full[j] == full[j - p] for j in range(p, p + 25))       # exact copies: 25 matches at distance p, 24 in the short one
                assert c.hand[2 * i:2 * i + 2] == ['none', 'all']
    c = K.case('threshold', 'homopolymer')
    assert [K.clipped(c, k) for k in (0, 1)] == [b'A' * 25, b'A' * 26] and c.hand == ['none', 'all']
    for p in (20, 64, 66, 68):
        for tag, mp, delta, full in (('delta7_maxperiod_p-2', p - 2, 7, True), ('delta7_maxperiod_p-3', p - 3, 7, False),
                                     ('delta0_maxperiod_p', p, 0, True), ('delta0_maxperiod_p-1', p - 1, 0, False)):
            c = K.case('threshold', 'p%d_%s' % (p, tag))
            assert c.params == (2, 7, 50, mp, delta) and len(K.clipped(c, 0)) == p + 25 and c.hand == ['all' if full else 'none']
    # the deciding lane in the second block, with lanes beyond maxperiod in it: period 66 gap-free; period 66 walking diagonal 68, which is
    # the own diagonal of lane 3 = period 68 > maxperiod
    for name in ('p66_delta0_maxperiod_p', 'p68_delta7_maxperiod_p-2'):
        mp = K.case('threshold', name).params[3]
        assert (mp - 1) // K.BLOCK == 1 and mp % K.BLOCK not in (0, 63)
    assert K.case('threshold', 'p68_delta7_maxperiod_p-2').params[3] == 66


def test_placement_edges():
    starts, ends = set(), set()
    for name, c in cases('placement'):
        (ch, s, e), (a, b) = c.iv[0], c.array
        seq = c.seqs[0]
        assert a - s == c.bit and b - a == c.length and seq[a - 1:a] == b'G' and seq[b:b + 1] == b'G'
        assert seq[a:b] == K.tile(b'AC', c.length)
        m = K.expected(c)[0]
        assert m.sum() == c.length and m[c.bit:c.bit + c.length].all()              # exactly the array, for every seed used
        starts.add(c.bit)
        ends.add(c.bit + c.length)
    assert {31, 32, 33, 63, 64} <= starts and {95, 96, 97} <= ends
    for name in ('one_word_minscore_50', 'one_word_minscore_30'):
        c = K.case('placement', name)
        assert c.bit % 32 == 0 and c.length == 32
    assert K.case('placement', 'one_word_minscore_30').params[2] == 30
    c = K.case('placement', 'last_word_of_the_slice')
    assert len(K.clipped(c, 0)) == c.bit + c.length == 96                          # the array is the slice's last word, all of it


def test_neighbours_edges():
    sizes, kinds = set(), set()
    full_len, zero_len = set(), set()
    for name, c in cases('neighbours'):
        n = len(c.iv)
        sizes.add(n)
        exp = K.expected(c)
        w = words(c)
        for k, (ch, s, e) in enumerate(c.iv):
            ln = len(K.clipped(c, k))
            kinds.add('empty' if s == e else 'inverted' if s > e else 'open' if e == K.OPEN_END else 'clipped' if e > len(c.seqs[ch]) else 'plain')
            kinds.add('scaffold%d' % ch)
            assert c.hand[k] in ('all', 'none') and exp[k].all() == (c.hand[k] == 'all') or ln == 0
            if c.hand[k] == 'all':
                assert ln % 32 == 0 and ln > 0                                      # its last word is full: the next slice's word follows a word of ones
                full_len.add(ln)
            elif ln:
                zero_len.add(ln)
                assert not exp[k].any()
        if len(set(c.iv)) < n:
            kinds.add('twice')
        # every zero slice with a word has a fully masked slice right before or behind it in the word array
        order = [k for k in range(n) if w[k]]
        for i, k in enumerate(order):
            if c.hand[k] == 'none' and n > 1:
                near = [order[x] for x in (i - 1, i + 1) if 0 <= x < len(order)]
                assert any(c.hand[x] == 'all' for x in near), (name, k)
    assert sizes == {1, 3, 4, 5, 9}                                                 # 4: a full workgroup of four wavefronts; the others leave one part-full
    assert {'empty', 'inverted', 'open', 'clipped', 'twice', 'scaffold0', 'scaffold1'} <= kinds
    assert full_len == {32, 64, 96} and zero_len == {1, 31, 32, 33}


def test_inside_edges():
    for name, c in cases('inside'):
        exp = K.expected(c)
        inside = 0
        for k, (ch, s, e) in enumerate(c.iv):
            seq = c.seqs[ch]
            ln = len(K.clipped(c, k))
            assert ln in (29, 30) and exp[k].all() == (ln == 30) and exp[k].any() == (ln == 30)
            if s >= 5 and seq[s - 5:s] == seq[s:s + 5]:
                # a copy lies right in front: a scorer that looked there would mask the 29-base slice too
                inside += 1
                if ln == 29:
                    assert K.mask_by_rule(seq[s - 5:s + ln], *c.params)[5:].all()
        assert inside >= 8
        assert {s for ch, s, e in c.iv if ch == 0} >= set(K.INSIDE_OFFSETS)
        assert (1, 0, 29) in c.iv and (1, 20, 50) in c.iv and len(c.seqs[1]) == 50 and (0, 140, 170) in c.iv and len(c.seqs[0]) == 170


def test_letters_edges():
    c = K.case('letters', 'letters')
    s = [K.clipped(c, k) for k in range(len(c.iv))]
    assert s[:4] == [b'N' * 40, b'R' * 40, b'a' * 26, b'aA' * 13]
    assert s[4].count(b'N') == 6 and s[4][30:36] == b'N' * 6
    assert s[5] != s[6] and s[5].upper() == s[6] and s[5][30:60].islower() and s[6][40:60] == K.tile(b'AC', 20)
    exp = K.expected(c)
    assert np.array_equal(exp[5], exp[6]) and exp[5][40:].sum() >= 120 and not exp[5][:30].any()


def test_long_edges():
    for name, c in cases('long'):
        assert [len(K.clipped(c, k)) for k in range(3)] == [2048, 2049, 2080] and c.params[3] == 2
        assert words(c) == [64, 65, 65]            # 64 words are one trip of k8_tandem_count's 64 lanes; 65 need a second
        assert all(m.all() for m in K.expected(c))


def test_pairs_edges():
    for name, c in cases('pairs'):
        s = K.clipped(c, 0)
        assert len(s) == 40 and c.params == (2, 7, 2, 3, 0)
        m = K.expected(c)[0]
        assert np.array_equal(m, K.pair_union(s)) and 20 <= m.sum() < 40 and (np.diff(m.astype(int)) != 0).sum() >= 2


def test_band_and_ties_edges():
    seen, masked = set(), 0
    for name, c in cases('band_and_ties'):
        ln = len(K.clipped(c, 0))
        assert 150 <= ln <= 200 and c.params in K.TIE_PARAMS
        seen.add((c.kind, c.unit, K.TIE_PARAMS.index(c.params)))
        masked += bool(K.expected(c)[0].any())
    for unit in K.TIE_UNITS:
        assert {p for kind, u, p in seen if u == unit and kind == 'noisy'} == {0, 1, 2, 3}
        assert {p for kind, u, p in seen if u == unit and kind == 'placed'} == {0, 1, 2, 3}
    assert sorted(abs(g) for g in K.TIE_PLACED) == [1, 1, 2, 2, 3, 3] and masked >= 0.75 * len(K.FAMILIES['band_and_ties'])


def test_wide_edges():
    fetched = set()
    for mp in (65, 66, 67, 127, 130):
        c = K.case('wide', 'indels_maxperiod_%d' % mp)
        assert c.params == (2, 7, 50, mp, 7) and len(c.indels) == 6
        exp = K.expected(c)
        for k, (u, g) in enumerate(c.indels):
            assert (62 <= u <= 67 or 126 <= u <= 131) and g and exp[k].all()
            s = K.clipped(c, k)
            assert not K.mask_by_rule(s, 2, 7, 50, mp, 0).any()                     # neither side of the indel reaches minscore alone
            # the periods that hold both diagonals u and u + g, and what their block's lanes 0 .. 3 fetch of the two
            holders = [q for q in range(1, mp + 1) if abs(q - u) <= 2 and abs(q - u - g) <= 2]
            assert holders, (mp, u, g)
            if min(holders) > K.BLOCK:                                              # only the wide kernel's shared masks can cover it
                for q in holders:
                    fetched |= {(mp, d) for d in {u, u + g} & set(K.FETCHED[(q - 1) // K.BLOCK])}
    assert {d for _, d in fetched} >= {63, 64, 129, 130, 127, 128}
    assert {mp for mp, _ in fetched} >= {65, 66, 127, 130}
    gf = K.case('wide', 'indels_maxperiod_65_gap_free')
    assert gf.params[4] == 0 and not any(m.any() for m in K.expected(gf))
    for delta, listed in ((7, [False, True, True, True]), (0, [False, False, False, True])):
        c = K.case('wide', 'job_edge_delta%d' % delta)
        lens = sorted({len(K.clipped(c, k)) for k in range(len(c.iv))})
        assert lens == [63, 64, 65, 66] and c.params[3:] == (130, delta)
        assert [K.first_diagonal(1, delta) < n for n in lens] == listed             # the second block's job: left out, listed
        assert all(K.first_diagonal(2, delta) >= n for n in lens)
    c = K.case('wide', 'shuffled')
    lens = [len(K.clipped(c, k)) for k in range(len(c.iv))]
    assert min(lens) == 0 and sum(1 for n in lens if 0 < n < 40) >= 10 and sum(1 for n in lens if n >= 63) >= 12
    assert lens != sorted(lens, reverse=True) and {ch for ch, _, _ in c.iv} == {0, 1}   # the job list's sort has something to reorder
    assert sum(1 for m in K.expected(c) if m.any()) >= 8 and sum(1 for m in K.expected(c) if m.size and not m.any()) >= 8
