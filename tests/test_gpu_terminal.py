"""Terminal repeats of features (mimeo_terminal_repeats, kernel K17; engine.terminal_repeats) against the numpy restatement of
the header's rules (tests/terminal_spec.py): every record field by field, every path block by block, and through K9
(mimeo_path_stats) and K11 (mimeo_path_text) the contracts that the header promises.  Equality is exact."""
import ctypes as C

import numpy as np
import pytest

from mimeo_amd import _ffi
from tests import terminal_spec as S

pytestmark = pytest.mark.gpu

FIELDS = _ffi.ALIGNMENT.names
COMP = {65: 84, 67: 71, 71: 67, 84: 65}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def rand(rng, n):
    return np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n)].copy()


def revcomp(s):
    return np.array([COMP.get(int(c), 78) for c in s[::-1]], dtype=np.uint8)


def substitute(rng, s, k):
    """k substitutions at distinct places, none at either end"""
    s = s.copy()
    for p in rng.choice(np.arange(1, len(s) - 1), size=k, replace=False):
        s[p] = ord('ACGT'[('ACGT'.index(chr(s[p])) + 1 + int(rng.integers(0, 3))) % 4])
    return s


def cat(*parts):
    return np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, bytes) else p for p in parts]).astype(np.uint8)


class Case:
    """scaffolds on the device, and the check of a call against the restatement"""

    def __init__(self, eng, seqs):
        self.eng, self.seqs = eng, [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs]
        self.g = eng.Genome(['s%d' % i for i in range(len(seqs))], self.seqs)

    def close(self):
        self.g.close()

    def check(self, items, **kw):
        got = self.eng.terminal_repeats(self.g, items, **kw)
        exp = S.terminal_repeats(self.seqs, items, **kw)
        recs, first, blocks = got
        assert recs.dtype == _ffi.ALIGNMENT and first.dtype == np.dtype('<u8') and blocks.dtype == _ffi.PATH_BLOCK
        for f in FIELDS:
            assert np.array_equal(recs[f], exp[0][f]), (f, recs[f].tolist(), exp[0][f].tolist())
        assert np.array_equal(first, exp[1])
        for f in ('t', 'q', 'len'):
            assert np.array_equal(blocks[f], exp[2][f]), f
        self.contracts(recs, first, blocks, S.params(**kw))
        return got

    def contracts(self, recs, first, blocks, P):
        st = self.eng.path_stats(self.g, None, recs, first, blocks)   # every path passes K9's checks, the empty ones too
        n = {f: st[f].astype(np.int64) for f in st.dtype.names}
        found = recs['score'] > 0
        assert np.array_equal(found, np.diff(first.astype(np.int64)) > 0) and (recs['score'][found] >= P['min_score']).all()
        assert np.array_equal(n['matches'], recs['id_n'])
        assert np.array_equal(n['matches'] + n['transitions'] + n['transversions'] + n['ambiguous'], recs['id_d'])
        assert np.array_equal(n['del_bases'], recs['tend'].astype(np.int64) - recs['tstart'] - recs['id_d'])
        assert np.array_equal(n['ins_bases'], recs['qend'].astype(np.int64) - recs['qstart'] - recs['id_d'])
        score = (P['match'] * n['matches'] - P['mismatch'] * (n['transitions'] + n['transversions'] + n['ambiguous'])
                 - P['gap_open'] * (n['ins_runs'] + n['del_runs']) - P['gap_extend'] * (n['ins_bases'] + n['del_bases']))
        assert np.array_equal(score, recs['score'])
        for k in np.flatnonzero(~found):   # nothing found: zero but tid, qid and qstrand
            assert all(int(recs[k][f]) == 0 for f in FIELDS if f not in ('tid', 'qid', 'qstrand')) and recs[k]['qstrand'] == k % 2
        return st

    def rows(self, recs, first, blocks):
        rf, trow, qrow = self.eng.path_text(self.g, None, recs, first, blocks)
        return [(bytes(trow[rf[i]:rf[i + 1]]).replace(b'-', b''), bytes(qrow[rf[i]:rf[i + 1]]).replace(b'-', b'')) for i in range(len(recs))]


@pytest.fixture(scope='module')
def plain(eng):
    """two random scaffolds: at min_score 1 every window finds something, gaps and all"""
    rng = np.random.default_rng(1701)
    c = Case(eng, [rand(rng, 3000), rand(rng, 1031)])
    yield c
    c.close()


# ---- window sizes -------------------------------------------------------------------------------------------------------------

WIDTHS = (1, 2, 63, 64, 65, 127, 128, 129, 200)


@pytest.mark.parametrize('w', WIDTHS)
def test_window_through_the_parameter(plain, w):
    recs, _, _ = plain.check([(0, 0, 3000), (0, 17, 2999), (1, 0, 1031), (1, 500, 1031)], window=w, min_score=1)
    assert w < 63 or (recs['score'] > 0).all()
    plain.check([(0, 0, 3000), (1, 0, 1031)], window=w)


@pytest.mark.parametrize('w', WIDTHS)
def test_window_through_short_items(plain, w):
    # window > L / 2: even and odd L, an item at base 0, one that ends at the scaffold's last base (the inverted tail starts
    # at base 0 of the rc strand)
    items = [(0, 100, 100 + 2 * w), (0, 100, 101 + 2 * w), (0, 0, 2 * w), (0, 0, 2 * w + 1), (1, 1031 - 2 * w, 1031), (1, 1030 - 2 * w, 1031)]
    plain.check(items, window=4096, min_score=1)
    plain.check(items, min_score=1)


def test_items_without_a_window(plain):
    recs, first, blocks = plain.check([(0, 5, 5), (0, 5, 6), (0, 5, 7), (1, 1031, 1031), (0, 0, 0), (0, 0, 1)], min_score=1)
    empty = [0, 1, 2, 3, 6, 7, 8, 9, 10, 11]   # L of 0 and 1: w == 0, nothing found whatever the threshold; L of 2: one cell
    assert (recs['score'][empty] == 0).all() and (np.diff(first.astype(np.int64))[empty] == 0).all() and blocks.size <= 2


# ---- planted repeats ----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def planted(eng):
    rng = np.random.default_rng(42)
    ltr = rand(rng, 300)
    ltr2 = substitute(rng, ltr, 9)
    ltr2 = cat(ltr2[:140], ltr2[145:])   # 3 % substitutions and one 5-base indel
    tir = rand(rng, 40)
    tir2 = revcomp(substitute(rng, tir, 2))
    s0 = cat(rand(rng, 500), ltr, rand(rng, 2400), ltr2, rand(rng, 500))                     # item [500, 500 + 2995)
    s1 = cat(rand(rng, 300), tir, rand(rng, 1120), tir2, rand(rng, 300))                     # item [300, 1500)
    s2 = cat(rand(rng, 200), tir, ltr, rand(rng, 1500), ltr2, tir2, rand(rng, 100))          # both: item [200, 200 + 2175)
    s3 = rand(rng, 4000)                                                                     # neither
    c = Case(eng, [s0, s1, s2, s3])
    c.ltr, c.ltr2, c.tir = ltr, ltr2, tir
    yield c
    c.close()


def test_planted_direct_repeat(planted):
    recs, first, blocks = planted.check([(0, 500, 3495)])
    d, i = recs[0], recs[1]
    assert i['score'] == 0 and d['score'] >= 2 * 295 - 5 * 9 - 15 - 5
    assert d['tstart'] <= 505 and d['tend'] >= 795 and d['qstart'] <= 3205 and d['qend'] >= 3490
    t, q = planted.rows(recs, first, blocks)[0]   # K11 reads the planted sequences back
    assert t == bytes(planted.seqs[0][d['tstart']:d['tend']]) and q == bytes(planted.seqs[0][d['qstart']:d['qend']])
    st = planted.eng.path_stats(planted.g, None, recs, first, blocks)
    assert st[0]['ins_bases'] + st[0]['del_bases'] == 5 and st[0]['transitions'] + st[0]['transversions'] == 9


def test_repeat_longer_than_the_window(planted):
    # the 300-base LTR under a window of 200: the head holds its first 200 bases, the tail the last 200 of the other copy, and
    # what they share runs from the tail window's first column into the head window's last row
    recs, _, _ = planted.check([(0, 500, 3495)], window=200)
    d = recs[0]
    assert d['tend'] == 700 and 3295 <= d['qstart'] <= 3297 and d['tstart'] <= 600 and d['qend'] >= 3395 and d['score'] > 150
    for w in (170, 250):   # beyond half the repeat the two windows share a part of it
        recs, _, _ = planted.check([(0, 500, 3495)], window=w)
        assert recs[0]['tend'] == 500 + w and recs[0]['qstart'] <= 3495 - w + 3   # a substitution at the border is cut off


def test_planted_inverted_repeat(planted):
    recs, first, blocks = planted.check([(1, 300, 1500)])
    d, i = recs[0], recs[1]
    assert d['score'] == 0 and i['score'] == 2 * 38 - 3 * 2
    # plus-strand coordinates of the planted tail
    assert (i['tstart'], i['tend'], i['qstart'], i['qend']) == (300, 340, 1460, 1500)
    t, q = planted.rows(recs, first, blocks)[1]
    assert t == bytes(planted.tir) and q == bytes(revcomp(planted.seqs[1][1460:1500]))


def test_both_and_neither(planted):
    recs, _, _ = planted.check([(2, 200, 2375), (3, 100, 3900)])
    assert recs['score'][0] > 400 and recs['score'][1] >= 2 * 38 - 6 and (recs['score'][2:] == 0).all()
    recs, _, _ = planted.check([(3, 100, 3900)], min_score=1)
    assert (recs['score'] > 0).all()   # chance alone finds something at the lowest threshold


# ---- window edges, ties, N, scoring -------------------------------------------------------------------------------------------

def test_window_edges(eng):
    rng = np.random.default_rng(7)
    r = rand(rng, 90)
    x, y = rand(rng, 110), rand(rng, 110)
    flush = cat(x, r, y, r)                                   # item == scaffold, L = 2 w: the best cell is (w - 1, w - 1)
    long_r = rand(rng, 500)
    tandem = cat(long_r, substitute(rng, long_r, 12))         # the repeat fills both windows: the path runs from border to border
    rr = rand(rng, 31)
    # the repeat lies across the border of the 64-column strip in the tail and across the rows 56 / 64 in the head
    border = cat(rand(rng, 48), rr, rand(rng, 121), rand(rng, 50), rr, rand(rng, 119))
    c = Case(eng, [flush, tandem, border])
    try:
        recs, _, _ = c.check([(0, 0, 400)], min_score=1)
        assert (recs[0]['tend'], recs[0]['qend']) == (200, 400) and recs[0]['score'] >= 180
        recs, _, _ = c.check([(1, 0, 1000)])
        assert (recs[0]['tstart'], recs[0]['tend'], recs[0]['qstart'], recs[0]['qend']) == (0, 500, 500, 1000)
        recs, _, _ = c.check([(2, 0, 400)], window=200)
        assert recs[0]['tstart'] <= 48 and recs[0]['tend'] >= 79 and recs[0]['qstart'] <= 250 and recs[0]['qend'] >= 281
        for w in (56, 57, 64, 65, 72):
            c.check([(2, 0, 400)], window=w, min_score=1)
    finally:
        c.close()


def test_ties(eng):
    rng = np.random.default_rng(11)
    r = rand(rng, 30)
    copy = cat(b'N' * 10, r, b'N' * 10)   # no column beyond the repeat pays: the copies tie exactly
    twice_tail = cat(rand(rng, 20), copy, rand(rng, 130), rand(rng, 30), copy, rand(rng, 20), copy, rand(rng, 50))   # L = 400
    twice_head = cat(rand(rng, 20), copy, rand(rng, 20), copy, rand(rng, 60), rand(rng, 100), copy, rand(rng, 50))   # L = 400
    p, s = rand(rng, 40), rand(rng, 40)
    homo = cat(p, b'AAAAA', s, rand(rng, 230), p, b'AAAAAAA', s, rand(rng, 13))                                         # L = 415
    c = Case(eng, [twice_tail, twice_head, homo])
    try:
        recs, _, _ = c.check([(0, 0, 400)], window=200)
        assert (recs[0]['score'], recs[0]['tstart'], recs[0]['qstart']) == (60, 30, 240)   # the smaller j: not 310
        recs, _, _ = c.check([(1, 0, 400)], window=200)
        assert (recs[0]['score'], recs[0]['tstart'], recs[0]['qstart']) == (60, 30, 310)   # the smaller i: not 100
        recs, first, blocks = c.check([(2, 0, 415)], window=200)
        st = c.eng.path_stats(c.g, None, recs, first, blocks)
        assert st[0]['ins_bases'] == 2 and st[0]['ins_runs'] == 1 and recs[0]['score'] == 2 * 85 - 5 - 4
    finally:
        c.close()


def test_insertion_next_to_deletion(eng):
    rng = np.random.default_rng(12)
    x, y = rand(rng, 60), rand(rng, 60)
    x[-1], y[0] = ord('G'), ord('T')   # neither run can slide into its neighbours
    seq = cat(x, b'A' * 8, y, rand(rng, 144), x, b'C' * 6, y, rand(rng, 2))
    c = Case(eng, [seq])
    try:
        recs, first, blocks = c.check([(0, 0, len(seq))], window=130, mismatch=50)
        st = c.eng.path_stats(c.g, None, recs, first, blocks)
        assert (st[0]['ins_runs'], st[0]['ins_bases'], st[0]['del_runs'], st[0]['del_bases']) == (1, 6, 1, 8)
        b = blocks[int(first[0]):int(first[1])]
        assert len(b) == 2 and b[1]['t'] > b[0]['t'] + b[0]['len'] and b[1]['q'] > b[0]['q'] + b[0]['len']   # both jump
    finally:
        c.close()


def test_n_bases(eng):
    rng = np.random.default_rng(13)
    r = rand(rng, 120)
    rn = r.copy()
    rn[30:34] = ord('N')
    r2 = r.copy()
    r2[80:82] = ord('N')
    r2[31] = ord('N')   # N against N is a mismatch too
    seq = cat(rand(rng, 7), b'NNN', rn, b'NNN', rand(rng, 197), r2, rand(rng, 10), b'NNNNN')
    c = Case(eng, [seq])
    try:
        recs, first, blocks = c.check([(0, 0, len(seq) - 5), (0, 0, len(seq))], window=150)
        st = c.eng.path_stats(c.g, None, recs, first, blocks)
        assert st[0]['ambiguous'] == 6 and recs[0]['score'] == 2 * 114 - 3 * 6 and recs[0]['id_d'] == 120
    finally:
        c.close()


@pytest.mark.parametrize('kw', [dict(gap_open=0), dict(mismatch=1000, match=1), dict(gap_open=0, gap_extend=1, match=1, mismatch=1),
                                dict(match=1000, mismatch=1, gap_open=1000, gap_extend=1000)])
def test_other_scoring(plain, planted, kw):
    plain.check([(0, 0, 3000), (1, 3, 1028)], window=150, min_score=1, **kw)
    planted.check([(0, 500, 3495), (1, 300, 1500)], window=400, **kw)


# ---- the largest windows, batching ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize('w', (1024, 4096))
def test_largest_windows(eng, w):
    rng = np.random.default_rng(w)
    r = rand(rng, 3 * w // 4)
    r2 = substitute(rng, r, w // 40)
    r2 = cat(r2[:w // 3], rand(rng, 7), r2[w // 3:w // 2], r2[w // 2 + 3:])
    seq = cat(rand(rng, 50), r, rand(rng, 2 * w + 100), r2, rand(rng, 60))
    c = Case(eng, [seq])
    try:
        recs, _, _ = c.check([(0, 50, len(seq) - 60)], window=w)
        assert recs[0]['score'] > w and recs[0]['tend'] - recs[0]['tstart'] >= 3 * w // 4 - 8
    finally:
        c.close()


def test_batching(eng, plain, planted, monkeypatch, capfd):
    rng = np.random.default_rng(5)
    items = []
    for k in range(100):   # 200 jobs: windows of 0 .. 400 bases in no order, the planted repeats among them
        L = int(rng.integers(0, 800)) if k % 7 else int(rng.integers(0, 4))
        s = int(rng.integers(0, 4000 - L))
        items.append((3, s, s + L))
    items[17], items[60] = (0, 500, 3495), (1, 300, 1500)
    monkeypatch.setenv('MIMEO_TERMINAL_STATS', '1')
    capfd.readouterr()
    a = planted.eng.terminal_repeats(planted.g, items, window=400, min_score=20)
    one = capfd.readouterr().err
    monkeypatch.setenv('MIMEO_TERMINAL_SCRATCH_MB', '1')
    b = planted.eng.terminal_repeats(planted.g, items, window=400, min_score=20)
    many = capfd.readouterr().err
    assert '[k17] checked: 100 items' in one and ', 1 launches' in one and '[k17] checked: 100 items' in many and ', 1 launches' not in many
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    monkeypatch.delenv('MIMEO_TERMINAL_STATS')
    planted.check(items[:30], window=400, min_score=20)   # ... and under the small budget they are the restatement's
    assert a[0]['score'][2 * 17] > 400 and a[0]['score'][2 * 60 + 1] == 70


# ---- errors -------------------------------------------------------------------------------------------------------------------

def test_errors_launch_nothing(plain, monkeypatch, capfd):
    eng, g = plain.eng, plain.g
    monkeypatch.setenv('MIMEO_TERMINAL_STATS', '1')
    capfd.readouterr()
    for items, kw, text, code in [
            ([(0, 0, 10), (2, 0, 10)], {}, 'item 1: chrom 2 is outside the genome', -1),
            ([(0, 11, 10)], {}, 'item 0: [11, 10) is not an interval of scaffold 0', -1),
            ([(0, 0, 10), (0, 0, 10), (1, 1000, 1032)], {}, 'item 2: [1000, 1032) is not an interval of scaffold 1 (1031 bases)', -1),
            ([(0, 0, 10)], dict(window=0), 'window = 0 is outside 1 .. 4096', -5),
            ([(0, 0, 10)], dict(window=4097), 'window = 4097 is outside 1 .. 4096', -5),
            ([(0, 0, 10)], dict(match=0), 'match = 0 is outside 1 .. 1000', -1),
            ([(0, 0, 10)], dict(match=1001), 'match = 1001', -1),
            ([(0, 0, 10)], dict(mismatch=0), 'mismatch = 0 is outside 1 .. 1000', -1),
            ([(0, 0, 10)], dict(mismatch=1001), 'mismatch = 1001', -1),
            ([(0, 0, 10)], dict(gap_open=-1), 'gap_open = -1 is outside 0 .. 1000', -1),
            ([(0, 0, 10)], dict(gap_open=1001), 'gap_open = 1001', -1),
            ([(0, 0, 10)], dict(gap_extend=0), 'gap_extend = 0 is outside 1 .. 1000', -1),
            ([(0, 0, 10)], dict(gap_extend=1001), 'gap_extend = 1001', -1),
            ([(0, 0, 10)], dict(min_score=0), 'min_score = 0 is outside >= 1', -1)]:
        with pytest.raises(RuntimeError) as e:
            eng.terminal_repeats(g, items, **kw)
        assert 'mimeo_terminal_repeats: ' + text in str(e.value) and '(code %d)' % code in str(e.value), str(e.value)
    with pytest.raises(TypeError):
        eng.terminal_repeats(g, [(0, 0, 10)], windows=3)
    # a reserved field: through the binding itself
    lib = _ffi.load()
    P = _ffi.TerminalParams()
    assert lib.mimeo_terminal_params_default(C.byref(P)) == 0
    assert [getattr(P, n) for n in P.NAMES] == [1024, 2, 3, 5, 2, 40] and list(P.reserved) == [0, 0]
    P.reserved[1] = 1
    iv = np.zeros(1, dtype=_ffi.INTERVAL)
    out = np.zeros(2, dtype=_ffi.ALIGNMENT)
    pf, pb, nb = C.c_void_p(), C.c_void_p(), C.c_uint64()
    assert lib.mimeo_terminal_repeats(g._h, iv.ctypes.data, 1, C.byref(P), out.ctypes.data, C.byref(pf), C.byref(pb), C.byref(nb)) == -1
    assert b'reserved must be 0' in lib.mimeo_last_error()
    assert lib.mimeo_terminal_repeats(g._h, iv.ctypes.data, 1, None, out.ctypes.data, C.byref(pf), C.byref(pb), C.byref(nb)) == -1
    # the library prints "[k17] checked" where the checks are behind, before its first HIP call: no such line, no device work
    assert '[k17]' not in capfd.readouterr().err
    eng.terminal_repeats(g, [(0, 0, 10)])
    err = capfd.readouterr().err
    assert err.index('[k17] checked: 1 items') < err.index('[k17] terminal repeats: 1 items')   # ... and a good call prints both
    recs, first, blocks = eng.terminal_repeats(g, [])
    assert recs.size == 0 and first.tolist() == [0] and blocks.size == 0
    recs, first, blocks = eng.terminal_repeats(g, np.zeros(0, dtype=_ffi.INTERVAL), window=7)
    assert recs.size == 0 and first.tolist() == [0] and blocks.size == 0
    assert '[k17]' not in capfd.readouterr().err   # n == 0 returns at once
