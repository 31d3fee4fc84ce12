"""K5's three chain kernels on the designed HSP sets of tests/k5_wave_cases.py (every edge of the wave kernel's steps: short tiles,
pure waves around 64 and 512 members, windows of 1 to 57 and of 448 to 3000 entries, tree blocks, cross-source ties, equal ends, the
top of the score and coordinate domain; tests/test_host_k5_wave.py proves on the CPU that the sets hold them).  Through
`mimeo_chain_hsps`, one group per call:

* the wave kernel (MIMEO_K5_BIG_MIN=1): flags, order and value fields equal the oracle's O(n^2) chain, and the step census it prints
  under MIMEO_K5_STATS equals the model's, number for number;
* the tile kernel (MIMEO_K5_NO_BIG=1) and the two-level kernel (MIMEO_K5_BIG=old, blocks of 2048): the wave kernel's bytes.
Everything is integer: no tolerance."""
import numpy as np
import pytest

from tests import k5_wave_cases as W

pytestmark = pytest.mark.gpu

ENV = ('MIMEO_K5_BIG_MIN', 'MIMEO_K5_BIG', 'MIMEO_K5_NO_BIG', 'MIMEO_K5_STATS')
MODES = {'wave': {'MIMEO_K5_BIG_MIN': '1', 'MIMEO_K5_STATS': '1'}, 'tiles': {'MIMEO_K5_NO_BIG': '1'},
         'two-level': {'MIMEO_K5_BIG_MIN': '1', 'MIMEO_K5_BIG': 'old'}}
_expected = {}


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def expected(family, name):
    """the oracle's chain of the set, made once"""
    if (family, name) not in _expected:
        from oracle import oracle as O
        exp = O.chain_hsps(W.case(family, name)[0])
        exp.setflags(write=False)
        _expected[family, name] = exp
    return _expected[family, name]


def run(eng, monkeypatch, capfd, h, mode):
    """the engine's chain under one kernel and the `[k5w]` lines it printed"""
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    for k, v in MODES[mode].items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    got = eng.chain_hsps(h)
    err = capfd.readouterr().err
    for e in ENV:
        monkeypatch.delenv(e, raising=False)
    return got, [l for l in err.splitlines() if l.startswith('[k5w]')]


@pytest.mark.parametrize('family', list(W.FAMILIES))
def test_designed_sets_under_the_three_kernels(eng, monkeypatch, capfd, family):
    for name in W.FAMILIES[family]:
        h, m = W.case(family, name)
        exp = expected(family, name)
        got, census = run(eng, monkeypatch, capfd, h, 'wave')
        tag = (family, name)
        assert got.size == exp.size == h.size, tag
        for f in ('tstart', 'qstart', 'length', 'score', 'raw_score'):
            assert np.array_equal(got[f], exp[f]), (tag, f)
        bad = np.flatnonzero((got['flags'] & 1) != (exp['flags'] & 1))
        where = [(int(k), int(m.step_of[k]), m.src[k], int(m.pred[k]), int(m.qcnt[k]) >> W.BLOCK_SHIFT) for k in bad[:8]]
        assert bad.size == 0, (tag, 'wave', bad.size, '(member, step, source, predecessor, tree block):', where)
        assert np.array_equal(got['flags'], exp['flags'] & 1), tag
        print(family, name, census)
        assert census == [W.census_line(m)], (tag, census, W.census_line(m))
        for mode in ('tiles', 'two-level'):
            other, lines = run(eng, monkeypatch, capfd, h, mode)
            assert not lines, (tag, mode, lines)
            assert np.array_equal(other['flags'] & 1, exp['flags'] & 1), (tag, mode, np.flatnonzero(other['flags'] != got['flags'])[:8])
            assert other.tobytes() == got.tobytes(), (tag, mode)
