"""CPU side of mimeo_params.bound_extensions (CLI --boundExtensions): the ABI slot, the flag and its rule, the workflow's
check, and the specification that the GPU tests of tests/test_gpu_bounds.py compare against (tests/bounded_oracle.c): with the
clause off it is the study oracle's path rule, with it on the alignments of a (pair, strand) never cross or touch, and on
every flanked-array case of the two test files it gives other records than the unbounded path rule."""
import ctypes as C

import numpy as np
import pytest

from mimeo_amd.synth import flanked_tandem_genome, tandem_genome
from tests import bounded_oracle as B

def test_params_property_maps_to_the_first_reserved_slot():
    from mimeo_amd import _ffi
    assert C.sizeof(_ffi.Params) == 64 and _ffi.Params.reserved.size == 5 * 4 and _ffi.Params.reserved.offset == 44
    p = _ffi.Params()
    assert p.bound_extensions == 0
    p.bound_extensions = 1
    assert p.reserved[0] == 1 and list(p.reserved)[1:] == [0, 0, 0, 0]
    assert p.as_dict()['bound_extensions'] == 1 and 'reserved' not in p.as_dict()
    setattr(p, 'bound_extensions', 0)   # what engine.default_params(bound_extensions=...) does
    assert p.reserved[0] == 0


def test_default_params_takes_the_keyword():
    from mimeo_amd import engine
    p = engine.default_params(anchor_rule=1, bound_extensions=1)
    assert p.anchor_rule == 1 and p.bound_extensions == 1 and p.reserved[0] == 1
    assert engine.default_params().bound_extensions == 0


def test_flag_on_every_command_and_only_with_the_path_rule(capsys):
    from mimeo_amd import run_interspecies, run_map, run_self
    for mod, base in ((run_self, ['--afasta', 'g.fa']), (run_interspecies, ['--afasta', 'a.fa', '--bfasta', 'b.fa']),
                      (run_map, ['--afasta', 'a.fa', '--bfasta', 'b.fa'])):
        assert mod.mainArgs(base).boundExtensions is False
        assert mod.mainArgs(base + ['--anchorRule', 'path']).boundExtensions is False
        assert mod.mainArgs(base + ['--anchorRule', 'path', '--boundExtensions']).boundExtensions is True
        for bad in (['--boundExtensions'], ['--anchorRule', 'box', '--boundExtensions']):
            with pytest.raises(SystemExit) as e:
                mod.mainArgs(base + bad)
            assert e.value.code == 2 and '--boundExtensions needs --anchorRule path' in capsys.readouterr().err


def test_workflow_refuses_bounds_without_the_path_rule(tmp_path):
    from mimeo_amd import workflow
    with pytest.raises(ValueError):
        workflow.gapped_params(3000, 'box', True)
    with pytest.raises(ValueError):
        workflow.self_repeats(None, [], str(tmp_path / 'a.tab'), str(tmp_path / 'a.gff3'), bound_extensions=True)
    with pytest.raises(ValueError):
        workflow.map_hits(None, None, [], str(tmp_path / 'b.tab'), anchor_rule=0, bound_extensions=True)
    p = workflow.gapped_params(2500, 'path', True)
    assert (p.hspthresh, p.anchor_rule, p.bound_extensions) == (2500, 1, 1)
    assert workflow.gapped_params(3000, 'path', False).bound_extensions == 0


def test_unbounded_specification_is_the_study_oracle_path_rule():
    """bounded = 0 restates orc_align_pair_rule(..., path_rule=1) byte for byte"""
    from tests import study_oracle as S
    _, seqs = tandem_genome(3, 2, 200_000)
    _, fl = flanked_tandem_genome(B.FLANKED_PAIR_SEEDS[0], 2)
    for T, Q in ((seqs[0], seqs[1]), (fl[0], fl[1])):
        T, Q = T.tobytes(), Q.tobytes()
        mine, ref = B.align_bounded(T, Q, 0), S.align_rule(T, Q, 1)
        assert ref.size > 0 and mine.tobytes() == ref.tobytes()


def test_every_flanked_case_parts_from_the_unbounded_path_rule():
    cases = B.flanked_cases()
    _, g = flanked_tandem_genome(B.FLANKED_GENOME_SEED, 8)
    ring = [(t, (t + 1) % 8) for t in range(8)]
    jobs = [(T.tobytes(), Q.tobytes(), b, kw) for _, T, Q, kw in cases for b in (0, 1)] + \
           [(g[t].tobytes(), g[q].tobytes(), b, {}) for t, q in ring for b in (0, 1)]
    out = B.many(jobs)
    cov = lambda r: int((r['tend'].astype(np.int64) - r['tstart']).sum())
    for k, (tag, _, _, _) in enumerate(cases):
        unb, bnd = out[2 * k], out[2 * k + 1]
        print(tag, 'alignments', unb.size, bnd.size, 'aligned target bases', cov(unb), cov(bnd))
        assert bnd.size > 0 and unb.tobytes() != bnd.tobytes(), (tag, 'the case shows nothing')
        assert cov(bnd) < cov(unb), tag   # unbounded, the flanks are aligned once per extra accepted anchor
    parted = 0
    for k, pr in enumerate(ring):
        unb, bnd = out[2 * (len(cases) + k)], out[2 * (len(cases) + k) + 1]
        parted += unb.tobytes() != bnd.tobytes()
    print('genome: ring pairs that part', parted, 'of', len(ring))
    assert parted >= 4, 'the 8-scaffold genome shows nothing'


@pytest.mark.parametrize('case', [0, 3, 6, 7])
def test_bounded_alignments_never_cross_or_touch(case):
    """From the exported paths alone: for every ordered pair (e earlier, f later) of extended alignments of a (pair, strand)
    and every target base where both have a diagonal step, f's diagonal differs from e's and lies on the side of e on which
    f's anchor diagonal d0 lies; e never has a step on d0 in such a row."""
    tag, T, Q, kw = B.flanked_cases()[case]
    recs, paths = B.align_bounded(T.tobytes(), Q.tobytes(), 1, paths=True, **kw)
    assert recs.size > 0
    checked = 0
    for minus in (0, 1):
        al = [p for p in paths if p[0] == minus]
        split = [((k >> np.uint64(32)).astype(np.int64), (k & np.uint64(0xFFFFFFFF)).astype(np.int64)) for _, _, _, _, k in al]
        for fi in range(len(al)):
            tf, qf = split[fi]
            d0 = al[fi][2] - al[fi][1]
            assert np.unique(tf).size == tf.size   # one diagonal step per target base
            for ei in range(fi):
                te, qe = split[ei]
                _, ie, jf = np.intersect1d(te, tf, return_indices=True)
                if not ie.size:
                    continue
                de, df = (qe - te)[ie], (qf - tf)[jf]
                checked += ie.size
                assert not (de == d0).any(), (tag, minus, ei, fi)
                assert not (de == df).any(), (tag, minus, ei, fi)
                assert (df[de < d0] > de[de < d0]).all() and (df[de > d0] < de[de > d0]).all(), (tag, minus, ei, fi)
    assert checked > 0, 'no two alignments share a target base: the case shows nothing'


def test_unbounded_path_rule_does_cross():
    """the invariant is the clause's doing: without it the same case has alignments that share diagonal steps' rows on the
    wrong side (or the same diagonal)"""
    tag, T, Q, kw = B.flanked_cases()[0]
    _, paths = B.align_bounded(T.tobytes(), Q.tobytes(), 0, paths=True, **kw)
    broken = 0
    for minus in (0, 1):
        al = [p for p in paths if p[0] == minus]
        for fi in range(len(al)):
            tf = (al[fi][4] >> np.uint64(32)).astype(np.int64)
            qf = (al[fi][4] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            d0 = al[fi][2] - al[fi][1]
            for ei in range(fi):
                te = (al[ei][4] >> np.uint64(32)).astype(np.int64)
                qe = (al[ei][4] & np.uint64(0xFFFFFFFF)).astype(np.int64)
                _, ie, jf = np.intersect1d(te, tf, return_indices=True)
                de, df = (qe - te)[ie], (qf - tf)[jf]
                broken += int(((de <= d0) & (df <= de)).sum() + ((de >= d0) & (df >= de)).sum())
    assert broken > 0
