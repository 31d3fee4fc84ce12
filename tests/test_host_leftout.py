"""The "left out" contract on the host: the designed genome of tests/leftout_cases.py is what it claims to be (checked with
the oracle, no engine), and workflow.drop_failed_pairs — what a job does after its gather — drops a failed scaffold pair's
records and paths on every rank, alone and over gloo."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np

from mimeo_amd import _ffi, formats, workflow
from mimeo_amd.dist import Dist
from tests import leftout_cases as LC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNDESIGNED = [(0, 1), (3, 4), (2, 2), (2, 5), (4, 3), (1, 0)]


def test_the_design_is_valid_against_the_oracle():
    _, seqs = LC.genome(6)
    rows = LC.oracle_rows(seqs, list(LC.F) + UNDESIGNED)
    for pr, strand in LC.F.items():
        r = rows[pr]
        cols = (r['tend'] - r['tstart']).astype(np.int64)
        on = r['qstrand'] == strand
        long = on & (cols >= 0.9 * LC.LONG_BP)
        assert long.any(), (pr, strand, cols.tolist())
        assert (r['id_n'][long] < r['id_d'][long]).all(), (pr, 'an identical half needs no pool and cannot fail')
        other = cols[~on]
        if pr[0] == pr[1]:   # the main diagonal of a self pair: the identical-suffix shortcut, no pool
            diag = ~on & (r['tstart'] == 0) & (r['id_n'] == r['id_d']) & (cols == seqs[pr[0]].size)
            assert int(diag.sum()) == 1
            other = cols[~on & ~diag]
        assert other.size == 0 or int(other.max()) <= 1500, (pr, other.tolist())
    for pr in UNDESIGNED:
        r = rows[pr]
        cols = (r['tend'] - r['tstart']).astype(np.int64)
        if pr[0] == pr[1]:
            cols = cols[~((r['qstrand'] == 0) & (r['tstart'] == 0) & (r['id_n'] == r['id_d']))]
        assert cols.size and int(cols.max()) <= 1500, (pr, cols.tolist())
    # what the per-pair GPU test needs: the designed pairs have rows on the strand that does not fail
    assert (rows[(0, 3)]['qstrand'] == LC.PLUS).any() and (rows[(1, 4)]['qstrand'] == LC.MINUS).any()


def test_the_six_scaffold_genome_is_the_head_of_the_nine_scaffold_one():
    _, s6 = LC.genome(6)
    _, s9 = LC.genome(9)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(s6, s9))
    _, bg = LC.genome(9, long_regions=False)
    assert [a.size for a in bg] == [a.size for a in s9]
    assert bg[2].tobytes() == s9[2].tobytes() and bg[0].tobytes() != s9[0].tobytes()


def _made_up(spec, seed):
    """records of the (tid, qid, qstrand) in `spec`, alignment i with 1 + i % 3 blocks; the blocks name their record"""
    rng = np.random.default_rng(seed)
    recs = np.zeros(len(spec), dtype=_ffi.ALIGNMENT)
    first, blocks = [0], []
    for i, (t, q, s) in enumerate(spec):
        recs[i]['tid'], recs[i]['qid'], recs[i]['qstrand'] = t, q, s
        recs[i]['score'] = int(rng.integers(3000, 90000))
        for k in range(1 + i % 3):
            blocks.append((1000 * seed + i, k, 10 + k))
        recs[i]['id_d'] = sum(b[2] for b in blocks[first[-1]:])
        first.append(len(blocks))
    return recs, np.array(first, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK)


def _rows(recs, first, blocks):
    return [recs[i].tobytes() + blocks[int(first[i]):int(first[i + 1])].tobytes() for i in range(recs.size)]


def test_drop_failed_pairs_on_made_up_records():
    spec = [(0, 3, 1), (1, 2, 0), (3, 0, 0), (0, 3, 0), (2, 2, 0), (0, 3, 1), (1, 2, 1), (3, 0, 1)]
    recs, first, blocks = _made_up(spec, 1)
    rows = _rows(recs, first, blocks)
    d = Dist()
    a, f, b, union = workflow.drop_failed_pairs(d, recs, first, blocks, [])
    assert union == [] and _rows(a, f, b) == rows and a is recs          # an empty failed set changes nothing
    a, f, b, union = workflow.drop_failed_pairs(d, recs, first, blocks, [(0, 3), (0, 3), (2, 2)])
    assert union == [(0, 3), (2, 2)]
    keep = [i for i, s in enumerate(spec) if (s[0], s[1]) not in union]
    assert keep == [1, 2, 6, 7]
    assert _rows(a, f, b) == [rows[i] for i in keep]                      # gone with their blocks, the order of the rest kept
    assert f.size == a.size + 1 and int(f[0]) == 0 and int(f[-1]) == b.size
    assert (np.diff(f.astype(np.int64)) == [1 + i % 3 for i in keep]).all()
    f2, b2 = formats.select_paths(first, blocks, keep)
    assert f.tolist() == f2.tolist() and b.tobytes() == b2.tobytes()
    # without paths; a failed pair without records; everything failed; no records at all
    a, f, b, union = workflow.drop_failed_pairs(d, recs, None, None, [(3, 0), (7, 7)])
    assert f is None and b is None and union == [(3, 0), (7, 7)]
    assert a.tobytes() == recs[[0, 1, 3, 4, 5, 6]].tobytes()
    a, f, b, _ = workflow.drop_failed_pairs(d, recs, first, blocks, sorted({(s[0], s[1]) for s in spec}))
    assert a.size == 0 and f.tolist() == [0] and b.size == 0
    a, f, b, union = workflow.drop_failed_pairs(d, recs[:0], first[:1], blocks[:0], [(0, 3)])
    assert a.size == 0 and f.tolist() == [0] and b.size == 0 and union == [(0, 3)]


WORKER = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, %r)
    import numpy as np
    from mimeo_amd import workflow
    from mimeo_amd.dist import Dist
    from tests.test_host_leftout import _made_up, _rows
    d = Dist().init('gloo')
    spec = [[(0, 3, 1), (3, 0, 0), (1, 2, 0), (0, 3, 1)], [(0, 3, 0), (2, 2, 0)]]
    failed = [[(0, 3)], []]
    if os.environ.get('IDLE_RANK1'):   # a rank with no work still joins the collectives
        spec[1] = []
    recs, first, blocks = _made_up(spec[d.rank], d.rank)
    first, blocks = d.allgather_paths(first, blocks)
    recs = d.allgather_records(recs)
    a, f, b, union = workflow.drop_failed_pairs(d, recs, first, blocks, failed[d.rank])
    assert union == [(0, 3)], union
    parts = [_made_up(s, r) for r, s in enumerate(spec)]
    exp = [row for p, s in zip(parts, spec) for row, x in zip(_rows(*p), s) if (x[0], x[1]) != (0, 3)]
    assert len(exp) == (2 if os.environ.get('IDLE_RANK1') else 3)
    assert _rows(a, f, b) == exp, (d.rank, a)
    assert f.size == a.size + 1 and int(f[-1]) == b.size
    d.barrier()
    print('rank', d.rank, 'ok')
''')


def _run_world2(extra_env=None):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
        env.update(extra_env or {})
        procs.append(subprocess.Popen([sys.executable, '-c', WORKER % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_drop_failed_pairs_gloo_world2():
    """Rank 0 reports (0, 3) and holds records of (0, 3), (3, 0) and (1, 2); rank 1 reports nothing and holds (0, 3) on the
    other strand and (2, 2): both end with the same union and the same surviving records."""
    _run_world2()


def test_drop_failed_pairs_gloo_with_an_idle_rank():
    _run_world2({'IDLE_RANK1': '1'})
