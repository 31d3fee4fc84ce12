"""CPU side of the path anchor rule: the ABI field, the CLI flag, the workflow's rule names, and the study oracle that the GPU
tests of tests/test_gpu_path_rule.py take as the specification (its box rule must be the CPU oracle's gapped stage)."""
import ctypes as C

import numpy as np
import pytest

from mimeo_amd.synth import synth_genome, tandem_genome


def test_params_field_and_size():
    from mimeo_amd import _ffi
    assert C.sizeof(_ffi.Params) == 64
    names = [n for n, _ in _ffi.Params._fields_]
    assert names[names.index('strand') + 1] == 'anchor_rule'
    assert _ffi.Params.anchor_rule.offset == 40 and _ffi.Params.reserved.size == 5 * 4
    assert _ffi.ANCHOR_RULES == {'box': 0, 'path': 1}


def test_anchor_rule_flag_on_every_command():
    from mimeo_amd import run_interspecies, run_map, run_self
    for mod, base in ((run_self, ['--afasta', 'g.fa']), (run_interspecies, ['--afasta', 'a.fa', '--bfasta', 'b.fa']),
                      (run_map, ['--afasta', 'a.fa', '--bfasta', 'b.fa'])):
        assert mod.mainArgs(base).anchorRule == 'box'
        assert mod.mainArgs(base + ['--anchorRule', 'path']).anchorRule == 'path'
        assert mod.mainArgs(base + ['--anchorRule', 'box']).anchorRule == 'box'
        with pytest.raises(SystemExit):
            mod.mainArgs(base + ['--anchorRule', 'lastz'])


def test_workflow_rule_names():
    from mimeo_amd import workflow
    assert workflow.anchor_rule_code('box') == 0 and workflow.anchor_rule_code('path') == 1 and workflow.anchor_rule_code(1) == 1
    with pytest.raises(ValueError):
        workflow.anchor_rule_code('Path')


def test_tandem_genome_keeps_synth_genome_and_adds_arrays():
    names, base = synth_genome(9, 3 * 120_000, 3)
    tnames, tand = tandem_genome(9, 3, 120_000)
    assert tnames == names and [a.size for a in tand] == [a.size for a in base]
    again = synth_genome(9, 3 * 120_000, 3)[1]
    assert all(np.array_equal(a, b) for a, b in zip(base, again))   # the helper changes copies only
    assert all((a != b).sum() > 1000 for a, b in zip(base, tand))


@pytest.mark.parametrize('seed', [3, 11])
def test_study_oracle_box_rule_is_the_oracle(seed):
    """box_vs_path.c:227 — orc_align_pair_rule(..., path_rule=0) reproduces orc_align_pair; on these genomes the path rule
    gives other records."""
    from oracle import oracle as O
    from tests import study_oracle as S
    names, seqs = tandem_genome(seed, 2, 200_000)
    T, Q = seqs[0].tobytes(), seqs[1].tobytes()
    box = S.align_rule(T, Q, 0)
    assert box.size > 0 and box.tobytes() == O.align_pair(T, Q).tobytes()
    one = S.align_rule(T, Q, 0, strand=2)
    assert one.tobytes() == O.align_pair(T, Q, O.default_params(strand=2)).tobytes()
    assert S.align_rule(T, Q, 1).tobytes() != box.tobytes()
