"""Flank repeats (mimeo_flank_repeats, kernel K18; engine.flank_repeats) and open frames (mimeo_open_frames, kernel K19;
engine.open_frames) against the restatements of the header's rules (tests/elements_spec.py), field by field, on the designed
inputs of tests/elements_cases.py and on random ones.  Equality is exact."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi
from tests import elements_cases as K
from tests import elements_spec as S

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def genome(eng, seqs):
    return eng.Genome(['s%d' % i for i in range(len(seqs))], [np.ascontiguousarray(s, dtype=np.uint8) for s in seqs])


def same(got, exp, what):
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    for f in got.dtype.names:
        assert np.array_equal(got[f], exp[f]), (what, f, np.flatnonzero((got[f] != exp[f]).ravel())[:5].tolist(), got[f].ravel()[:12].tolist(),
                                                exp[f].ravel()[:12].tolist())


# ---- K18 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', K.k18_cases(), ids=lambda c: c[0])
def test_flank_designed(eng, case):
    name, seqs, items, kw, expected = case
    g = genome(eng, seqs)
    try:
        got = eng.flank_repeats(g, items, **kw)
    finally:
        g.close()
    assert got.dtype == _ffi.FLANK_REPEAT
    same(got, S.flank_repeats(seqs, items, **kw), name)
    same(got, S.flank_repeats(seqs, items, impl=S.flank_loops, **kw), name)
    for r, e, (_, start, end) in zip(got, expected, items):
        if e is not None:
            assert (int(r['len']), int(r['mismatches']), int(r['dl']), int(r['dr'])) == e, (name, r, e)
        if int(r['len']):
            assert int(r['left_start']) == start + int(r['dl']) - int(r['len']) and int(r['right_start']) == end + int(r['dr'])
        else:
            assert all(int(r[f]) == 0 for f in r.dtype.names)


def test_flank_random_items_in_one_call(eng, monkeypatch):
    seqs, items = K.k18_random()
    exp = S.flank_repeats(seqs, items, min_len=2)
    assert 2000 < int((exp['len'] > 0).sum()) < 5000 and len({int(d) for d in exp['dl']}) == 5
    g = genome(eng, seqs)
    try:
        got = eng.flank_repeats(g, items, min_len=2)
        same(got, exp, 'random')
        sub = slice(0, 300)
        same(got[sub], S.flank_repeats(seqs, items[sub], impl=S.flank_loops, min_len=2), 'random, loops')
        for kw in (dict(min_len=3, max_len=32, slack=8, max_mismatch=2), dict(min_len=2, max_len=9, slack=5, max_mismatch=1)):
            same(eng.flank_repeats(g, items[:200], **kw), S.flank_repeats(seqs, items[:200], **kw), str(kw))
        monkeypatch.setenv('MIMEO_PATH_LAUNCH_JOBS', '777')   # the same items in seven launches
        same(eng.flank_repeats(g, items, min_len=2), exp, 'random, cut into launches')
        assert eng.flank_repeats(g, []).shape == (0,)
    finally:
        g.close()


def test_flank_argument_errors(eng):
    seqs = [K.rand(np.random.default_rng(5), 100), K.rand(np.random.default_rng(6), 40)]
    g = genome(eng, seqs)
    try:
        for items, kw, text in (([(2, 0, 10)], {}, 'item 0: chrom 2 is outside the genome'), ([(0, 0, 10), (1, 5, 41)], {}, 'item 1: [5, 41) is not an interval'),
                                ([(0, 11, 10)], {}, 'item 0: [11, 10) is not an interval'), ([(0, 0, 10)], dict(min_len=1), 'min_len = 1 is outside 2 .. 32'),
                                ([(0, 0, 10)], dict(min_len=33, max_len=33), 'min_len = 33'), ([(0, 0, 10)], dict(max_len=3), 'max_len = 3 is outside min_len .. 32'),
                                ([(0, 0, 10)], dict(max_len=33), 'max_len = 33'), ([(0, 0, 10)], dict(slack=-1), 'slack = -1 is outside 0 .. 8'),
                                ([(0, 0, 10)], dict(slack=9), 'slack = 9'), ([(0, 0, 10)], dict(max_mismatch=3), 'max_mismatch = 3 is outside 0 .. 2'),
                                ([(0, 0, 10)], dict(max_mismatch=-1), 'max_mismatch = -1'), ([], dict(slack=9), 'slack = 9')):
            with pytest.raises(RuntimeError) as e:
                eng.flank_repeats(g, items, **kw)
            assert 'libmimeo_hip: mimeo_flank_repeats: ' in str(e.value) and text in str(e.value) and '(code -1)' in str(e.value), str(e.value)
        with pytest.raises(TypeError):
            eng.flank_repeats(g, [(0, 0, 10)], window=3)
        lib = _ffi.load()
        P = _ffi.FlankParams()
        lib.mimeo_flank_params_default(C.byref(P))
        P.reserved[3] = 1
        iv = np.zeros(1, dtype=_ffi.INTERVAL)
        out = np.zeros(1, dtype=_ffi.FLANK_REPEAT)
        assert lib.mimeo_flank_repeats(g._h, iv.ctypes.data, 1, C.byref(P), out.ctypes.data) == -1
        assert lib.mimeo_last_error().decode() == 'mimeo_flank_repeats: reserved must be 0'
        P.reserved[3] = 0
        assert lib.mimeo_flank_repeats(g._h, None, 0, C.byref(P), None) == 0   # n == 0
        assert lib.mimeo_flank_repeats(g._h, None, 1, C.byref(P), out.ctypes.data) == -1
        # K19: the same checks under its own name, and the flags
        for items, text in (([(2, 0, 10)], 'item 0: chrom 2 is outside the genome'), ([(0, 0, 10), (1, 5, 41)], 'item 1: [5, 41) is not an interval'),
                            ([(0, 11, 10)], 'item 0: [11, 10) is not an interval')):
            with pytest.raises(RuntimeError) as e:
                eng.open_frames(g, items)
            assert 'libmimeo_hip: mimeo_open_frames: ' in str(e.value) and text in str(e.value) and '(code -1)' in str(e.value), str(e.value)
        fr = np.zeros(6, dtype=_ffi.OPEN_FRAME)
        assert lib.mimeo_open_frames(g._h, iv.ctypes.data, 1, 1, fr.ctypes.data) == -1
        assert lib.mimeo_last_error().decode() == 'mimeo_open_frames: flags = 1 must be 0'
        assert lib.mimeo_open_frames(g._h, None, 0, 0, None) == 0
        assert eng.open_frames(g, []).shape == (0, 6)
    finally:
        g.close()


# ---- K19 --------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('case', K.k19_cases(), ids=lambda c: c[0])
def test_frames_designed(eng, case):
    name, seqs, items = case
    g = genome(eng, seqs)
    try:
        got = eng.open_frames(g, items)
    finally:
        g.close()
    assert got.dtype == _ffi.OPEN_FRAME and got.shape == (len(items), 6)
    same(got, S.open_frames(seqs, items), name)
    if max(e - s for _, s, e in items) < 200:
        same(got, S.open_frames(seqs, items, impl=S.frames_loops), name)
    empty = got['codons'] == 0
    assert all((got[f][empty] == 0).all() for f in got.dtype.names) and (got['met'] <= got['codons']).all()
    assert ((got['end'] - got['start']) == 3 * got['codons']).all()


def test_frames_designed_answers(eng):
    run = K.sense_run(np.random.default_rng(2), 10)
    seqs = [K.cat(b'TAA', run, b'TAG', b'ATG', run, b'TGA', b'CC')]   # frame 0: ten codons, then eleven that start with ATG
    g = genome(eng, seqs)
    try:
        got = eng.open_frames(g, [(0, 0, 74), (0, 3, 33), (0, 0, 2)])
    finally:
        g.close()
    assert got[0, 0].tolist() == (36, 69, 11, 0) and got[1, 0].tolist()[:3] == (3, 33, 10) and not got[2]['codons'].any()


CHILD = ('import json, sys; sys.path.insert(0, %r); import numpy as np; from mimeo_amd import engine; from tests import elements_cases as K; '
         'engine.init(0); s = K.k19_long(); g = engine.Genome(["s"], [s]); '
         'r = engine.open_frames(g, [(0, 0, 10000), (0, 1, 9999), (0, 4095, 4099)]); g.close(); print(json.dumps(r.tolist()))' % ROOT)


def test_frames_one_run_over_three_steps_and_chunks(eng):
    s = K.k19_long()
    items = [(0, 0, 10000), (0, 1, 9999), (0, 4095, 4099)]
    exp = S.open_frames([s], items)
    assert exp[0, 0].tolist()[:3] == (0, 9999, 3333)
    g = genome(eng, [s])
    try:
        got = eng.open_frames(g, items)
    finally:
        g.close()
    same(got, exp, 'one run over three steps')
    # the same items cut into chunks of one step, in a fresh process: equal records
    env = dict(os.environ, MIMEO_FRAMES_CHUNK='4096', MIMEO_ELEMENTS_STATS='1')
    r = subprocess.run([sys.executable, '-c', CHILD], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    assert 'chunks of 4096 bases' in r.stderr and '3 items, 14 chunk jobs' in r.stderr, r.stderr[-2000:]
    assert [[tuple(f) for f in item] for item in json.loads(r.stdout.splitlines()[-1])] == [[tuple(f) for f in item] for item in got.tolist()]


def test_frames_long_and_many_items(eng):
    rng = np.random.default_rng(191)
    big = K.rand(rng, 300_001)
    big[150_000:150_900] = K.sense_run(rng, 300)   # one long frame in the noise
    seqs, items = K.k19_random()
    g = genome(eng, [big] + seqs)
    try:
        one = eng.open_frames(g, [(0, 1, 300_001)])
        many = eng.open_frames(g, [(c + 1, a, b) for c, a, b in items])
    finally:
        g.close()
    same(one, S.open_frames([big], [(0, 1, 300_001)]), '300 000 bases')
    assert int(one['codons'].max()) >= 300
    same(many, S.open_frames(seqs, items), '2000 items')
