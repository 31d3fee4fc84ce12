"""Alignment paths, host side: the CIGAR / PAF writers on made-up records with the expected lines written out by hand, the
box-rule path oracle the GPU tests compare against (tests/paths_oracle.c) held to the two oracles it restates, the
all-gatherv of (records, first, blocks) over gloo, and the row ordering of mimeo_align_units_paths under the sanitizers."""
import os
import socket
import subprocess
import sys
import textwrap

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rec(tstart, tend, qstart, qend, score, id_n, id_d, qstrand):
    r = np.zeros(1, dtype=_ffi.ALIGNMENT)
    r['tstart'], r['tend'], r['qstart'], r['qend'], r['score'], r['id_n'], r['id_d'], r['qstrand'] = tstart, tend, qstart, qend, score, id_n, id_d, qstrand
    return r


def _blk(*b):
    return np.array(list(b), dtype=_ffi.PATH_BLOCK)


def test_cigar_and_paf_lines_by_hand():
    # plus row: an insertion of 3 query bases, then a deletion of 5 target bases
    plus = _blk((100, 50, 20), (120, 73, 15), (140, 88, 20))
    # minus row, query of 800 bases: blocks in reverse-complement coordinates 300 .. 342 -> plus strand 458 .. 500
    minus = _blk((200, 300, 10), (210, 312, 30))
    # the two halves leave the anchor with a gap: 7 query bases and 4 target bases between the blocks
    both = _blk((300, 400, 12), (316, 419, 8))
    single = _blk((10, 10, 100))
    assert formats.cigar(plus) == '20M3I15M5D20M'
    assert formats.cigar(minus) == '10M2I30M'
    assert formats.cigar(both) == '12M7I4D8M'
    assert formats.cigar(single) == '100M'
    assert formats.cigar(_blk()) == ''
    recs = np.concatenate([_rec(100, 160, 50, 108, 4000, 50, 55, 0), _rec(200, 240, 458, 500, 3500, 38, 40, 1),
                           _rec(300, 324, 400, 427, 3100, 20, 20, 0), _rec(10, 110, 10, 110, 9100, 100, 100, 0)])
    recs['qid'] = [0, 0, 1, 1]
    blocks = np.concatenate([plus, minus, both, single])
    first = np.array([0, 3, 5, 7, 8], dtype=np.uint64)
    got = formats.paf_lines(recs, first, blocks, ['chrT'], [1000], ['chrQ', 'q2'], [800, 500])
    assert got == [
        'chrQ\t800\t50\t108\t+\tchrT\t1000\t100\t160\t50\t63\t255\tAS:i:4000\tcg:Z:20M3I15M5D20M',
        'chrQ\t800\t458\t500\t-\tchrT\t1000\t200\t240\t38\t42\t255\tAS:i:3500\tcg:Z:10M2I30M',
        'q2\t500\t400\t427\t+\tchrT\t1000\t300\t324\t20\t31\t255\tAS:i:3100\tcg:Z:12M7I4D8M',
        'q2\t500\t10\t110\t+\tchrT\t1000\t10\t110\t100\t100\t255\tAS:i:9100\tcg:Z:100M',
    ]
    # a selection of rows in another order takes its blocks along
    f2, b2 = formats.select_paths(first, blocks, [3, 1])
    assert f2.tolist() == [0, 1, 3] and b2.tolist() == single.tolist() + minus.tolist()
    assert formats.paf_lines(recs[[3, 1]], f2, b2, ['chrT'], [1000], ['chrQ', 'q2'], [800, 500]) == [got[3], got[1]]
    f0, b0 = formats.select_paths(first, blocks, [])
    assert f0.tolist() == [0] and b0.size == 0


def test_tab_blocks_names_the_rows_it_wrote():
    """tab_blocks(rows=...): the index of every TAB row's record, in block order; the two return values are unchanged."""
    rng = np.random.default_rng(3)
    a = np.zeros(300, dtype=_ffi.ALIGNMENT)
    a['tid'], a['qid'] = rng.integers(0, 3, a.size), rng.integers(0, 3, a.size)
    a['tstart'] = rng.integers(0, 5000, a.size)
    a['tend'] = a['tstart'] + rng.integers(50, 400, a.size)
    a['qstart'] = rng.integers(0, 5000, a.size)
    a['qend'] = a['qstart'] + (a['tend'] - a['tstart'])
    a['id_d'] = a['tend'] - a['tstart']
    a['id_n'] = (a['id_d'] * rng.uniform(0.7, 1.0, a.size)).astype(np.uint32)
    a['score'] = rng.integers(3000, 90000, a.size)
    names = ['s0', 's1', 's2']
    blocks, kept = formats.tab_blocks(a, names, names, 100, 80)
    rows = []
    blocks2, kept2 = formats.tab_blocks(a, names, names, 100, 80, rows=rows)
    assert blocks2 == blocks and np.array_equal(kept, kept2) and len(rows) == 1
    idx = rows[0]
    assert 0 < idx.size < a.size and idx.size == kept.shape[0] == sum(len(v) for v in blocks.values())
    lines = [l for pr in sorted(blocks) for l in blocks[pr]]
    for line, i in zip(lines, idx.tolist()):
        f = line.split('\t')
        assert (f[0], int(f[2]) - 1, int(f[3]), f[4], int(f[8])) == (names[a['tid'][i]], a['tstart'][i], a['tend'][i], names[a['qid'][i]], a['score'][i])
    rows = []
    formats.tab_blocks(a[:0], names, names, 100, 80, rows=rows)
    assert rows[0].size == 0


def _cases():
    from mimeo_amd.synth import flanked_tandem_genome, tandem_genome
    from tests import bounded_oracle as B
    _, s = tandem_genome(3, 2, 60_000)
    _, f = flanked_tandem_genome(1, 2)
    return [('tandem', s[0], s[1]), ('flanked rc', f[0], B.revcomp(f[1]))]


@pytest.mark.parametrize('case', [0, 1])
def test_paths_oracle_restates_the_two_oracles(case):
    """Box rule: the records of tests/paths_oracle.c are those of the parity oracle.  Path rule: its records and its dump of
    the extended alignments are those of tests/bounded_oracle.c run unbounded."""
    from oracle import oracle as O
    from tests import bounded_oracle as B
    from tests import paths_oracle as PO
    tag, T, Q = _cases()[case]
    recs, ext = PO.align_paths(T, Q, 0)
    assert recs.tobytes() == O.align_pair(T.tobytes(), Q.tobytes()).tobytes(), tag
    assert len(ext) >= recs.size >= 2
    for minus, at, aq, score, keys in ext:   # an alignment's steps are distinct and hold its anchor's diagonal neighbourhood
        assert np.unique(keys).size == keys.size
    precs, pext = PO.align_paths(T, Q, 1)
    brecs, bext = B.align_bounded(T, Q, 0, paths=True)
    assert precs.tobytes() == brecs.tobytes() and len(pext) == len(bext), tag
    for a, b in zip(pext, bext):
        assert a[:4] == b[:4] and np.array_equal(a[4], b[4]), (tag, a[:4], b[:4])
    assert precs.tobytes() != recs.tobytes(), 'the rules do not part on this input'
    if case == 1:
        assert all(e[0] == 1 for e in ext), 'every alignment of this case is on the minus strand'


WORKER = textwrap.dedent('''
    import os, sys
    sys.path.insert(0, %r)
    import numpy as np
    from mimeo_amd import _ffi
    from mimeo_amd.dist import Dist
    d = Dist().init('gloo')
    # rank 0: three alignments of 2, 0 and 3 blocks; rank 1: none
    cnt = [2, 0, 3] if d.rank == 0 else []
    a = np.zeros(len(cnt), dtype=_ffi.ALIGNMENT)
    a['score'] = 1000 + np.arange(len(cnt))
    first = np.zeros(len(cnt) + 1, dtype=np.uint64)
    first[1:] = np.cumsum(cnt)
    b = np.zeros(int(first[-1]), dtype=_ffi.PATH_BLOCK)
    b['t'], b['q'], b['len'] = 10 * np.arange(b.size), 7 * np.arange(b.size), 1 + np.arange(b.size)
    f2, b2 = d.allgather_paths(first, b)
    g = d.allgather_records(a)
    assert g.size == 3 and list(g['score']) == [1000, 1001, 1002]
    assert f2.dtype == np.uint64 and f2.tolist() == [0, 2, 2, 5], f2
    assert b2.dtype == _ffi.PATH_BLOCK and b2['t'].tolist() == [0, 10, 20, 30, 40] and b2['len'].tolist() == [1, 2, 3, 4, 5]
    if os.environ.get('BOTH_RANKS'):   # and a second round with rows on both ranks: rank order
        cnt = [1] if d.rank == 0 else [2, 1]
        first = np.zeros(len(cnt) + 1, dtype=np.uint64)
        first[1:] = np.cumsum(cnt)
        b = np.zeros(int(first[-1]), dtype=_ffi.PATH_BLOCK)
        b['t'] = 100 * (d.rank + 1) + np.arange(b.size)
        f2, b2 = d.allgather_paths(first, b)
        assert f2.tolist() == [0, 1, 3, 4] and b2['t'].tolist() == [100, 200, 201, 202]
    d.barrier()
    print('rank', d.rank, 'ok')
''')


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_allgather_paths_gloo_world2_one_rank_empty():
    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE='2', LOCAL_RANK=str(r), MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), BOTH_RANKS='1')
        procs.append(subprocess.Popen([sys.executable, '-c', WORKER % ROOT], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    for p, o in zip(procs, outs):
        assert p.returncode == 0, o


def test_single_process_allgather_paths_is_the_identity():
    from mimeo_amd.dist import Dist
    first, b = np.array([0, 2], dtype=np.uint64), np.zeros(2, dtype=_ffi.PATH_BLOCK)
    f2, b2 = Dist().allgather_paths(first, b)
    assert f2 is first and b2 is b


def test_plus_strand_first_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'paths_order.cc')
    exe = tmp_path / 'paths_order_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'paths_order: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]


def test_cli_takes_paf(capsys):
    from mimeo_amd import run_interspecies, run_map, run_self
    assert run_self.mainArgs(['--afasta', 'a.fa']).paf is None
    assert run_self.mainArgs(['--afasta', 'a.fa', '--paf', 'x.paf']).paf == 'x.paf'
    assert run_map.mainArgs(['--afasta', 'a.fa', '--bfasta', 'b.fa', '--paf', 'y.paf']).paf == 'y.paf'
    assert run_interspecies.mainArgs(['--afasta', 'a.fa', '--bfasta', 'b.fa', '--paf', 'z.paf']).paf == 'z.paf'
