"""K8 tandem scorer on the designed slices of tests/k8_cases.py (the threshold at 49 / 50, the array's place in the mask words, fully
masked slices beside all-zero ones, slices that begin inside an array, letters outside ACGT, more than 64 mask words, the densest
marking, the band and tie rules, the wide kernel's block ends and job list; tests/test_host_k8_edges.py proves on the CPU that the
slices hold these edges and tell nine wrong rules apart).  Per family: `engine.tandem_mask` equals `mask_by_rule` bit for bit, slice by
slice; the counts that came with the masks, and those of `engine.tandem_masked`, are the masks' sums; the hand-derived answers hold.
Everything is integer: no tolerance."""
import numpy as np
import pytest

from tests import k8_cases as K

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def eng():
    from mimeo_amd import engine
    engine.init(0)
    return engine


def check_case(eng, family, name):
    c = K.case(family, name)
    exp = K.expected(c)
    g = eng.Genome(['s%d' % i for i in range(len(c.seqs))], c.seqs)
    try:
        iv = np.array(c.iv, dtype=np.uint32)
        masks, with_masks = eng.tandem_mask(g, iv, *c.params, counts=True)
        counts = eng.tandem_masked(g, iv, *c.params)
    finally:
        g.close()
    assert len(masks) == len(c.iv) == counts.size == with_masks.size, (family, name)
    for k, (got, want) in enumerate(zip(masks, exp)):
        tag = (family, name, k, c.iv[k], c.params)
        assert got.dtype == bool and got.shape == want.shape, (tag, got.shape, want.shape)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (tag, '%d positions differ, the first:' % bad.size,
                               [(int(i), 'engine' if got[i] else 'rule') for i in bad[:12]], 'masked by the engine / the rule:',
                               int(got.sum()), int(want.sum()))
        hand = K.hand_mask(c, k)
        if hand is not None:
            assert np.array_equal(got, hand), (tag, c.hand[k] if isinstance(c.hand[k], str) else 'positions by hand')
        assert int(with_masks[k]) == int(counts[k]) == int(want.sum()), (tag, int(with_masks[k]), int(counts[k]), int(want.sum()))


@pytest.mark.parametrize('family', list(K.FAMILIES))
def test_designed_slices_mask_equals_the_rule(eng, family):
    assert sum(K.cost(K.case(family, name)) for name in K.FAMILIES[family]) < K.COST_CAP
    for name in K.FAMILIES[family]:
        check_case(eng, family, name)


def test_mask_of_no_slices_and_of_empty_slices_only(eng):
    g = eng.Genome(['s'], [b'ACGT' * 20])
    try:
        assert eng.tandem_mask(g, np.zeros((0, 3), dtype=np.uint32)) == []
        masks, counts = eng.tandem_mask(g, np.array([(0, 10, 10), (0, 50, 20), (0, 80, 90)], dtype=np.uint32), counts=True)
        assert [m.size for m in masks] == [0, 0, 0] and counts.tolist() == [0, 0, 0]
        with pytest.raises(RuntimeError, match='out of range'):
            eng.tandem_mask(g, np.array([(1, 0, 10)], dtype=np.uint32))
    finally:
        g.close()
