"""Terminal repeats (K17, mimeo_terminal_repeats) without a device: the two restatements of the header's rules against each
other, the optimality of their paths, formats.terminal_repeat_lines by hand, the CLI flags, the binding, and the HIP-free host
side (mimeo_amd/csrc/terminal_host.h) under ASan and UBSan as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi, formats
from tests import terminal_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_struct_and_binding():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    for name in ('mimeo_terminal_repeats', 'mimeo_terminal_params_default'):
        assert name in declared and name in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    m = re.search(r'typedef struct mimeo_terminal_params \{(.*?)\} mimeo_terminal_params;', hdr, re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    assert tuple(re.findall(r'\b([a-z_]+)(?:\[2\])?\s*;', body)) == _ffi.TerminalParams.NAMES + ('reserved',)
    assert C.sizeof(_ffi.TerminalParams) == 32 and [f[0] for f in _ffi.TerminalParams._fields_] == list(_ffi.TerminalParams.NAMES) + ['reserved']
    m = re.search(r'int mimeo_terminal_repeats\((.*?)\);', hdr, re.S)
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['G', 'iv', 'n', 'p', 'out', 'path_first', 'blocks', 'nblocks']
    lib = _ffi.load()
    want = [C.POINTER(_ffi.TerminalParams) if 'mimeo_terminal_params' in a else C.POINTER(C.c_void_p) if '**' in a else C.POINTER(C.c_uint64) if a == 'uint64_t *nblocks'
            else C.c_void_p if '*' in a else C.c_uint64 for a in args]
    assert list(lib.mimeo_terminal_repeats.argtypes) == want
    for name in _ffi.SYMBOLS:
        assert hasattr(lib, name), name
    P = _ffi.TerminalParams()
    assert lib.mimeo_terminal_params_default(C.byref(P)) == 0   # needs no device
    assert {n: getattr(P, n) for n in P.NAMES} == S.DEFAULTS and list(P.reserved) == [0, 0]
    assert lib.mimeo_terminal_params_default(None) == -1
    from mimeo_amd import engine
    assert callable(engine.terminal_repeats)


def test_no_cpu_fallback():
    # a process that never called mimeo_init: MIMEO_ERR_NO_DEVICE before any argument is looked at, and nothing handed back
    code = ('import ctypes as C, sys; sys.path.insert(0, %r); from mimeo_amd import _ffi; lib = _ffi.load(); P = _ffi.TerminalParams(); '
            'lib.mimeo_terminal_params_default(C.byref(P)); pf, pb, nb = C.c_void_p(), C.c_void_p(), C.c_uint64(); '
            'rc = lib.mimeo_terminal_repeats(None, None, 0, C.byref(P), None, C.byref(pf), C.byref(pb), C.byref(nb)); '
            'print(rc, pf.value, pb.value, lib.mimeo_last_error().decode())' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.startswith('-2 None None ') and 'no CPU fallback' in r.stdout


def _random_pair(rng, w, alphabet):
    return rng.integers(0, alphabet, w).astype(np.uint8), rng.integers(0, alphabet, w).astype(np.uint8)


def test_restatements_agree_on_random_inputs():
    rng = np.random.default_rng(17)
    found = 0
    for t in range(250):
        w = int(rng.integers(1, 65))
        a, b = _random_pair(rng, w, int(rng.choice([2, 4, 5])))   # two letters: ties everywhere; five: N
        P = S.params(min_score=int(rng.choice([1, 1, 8])), gap_open=int(rng.choice([0, 1, 5])), gap_extend=int(rng.choice([1, 2])),
                     match=int(rng.choice([1, 2, 5])), mismatch=int(rng.choice([1, 3, 1000])))
        x, y = S.gotoh_loops(a, b, P), S.gotoh_sweep(a, b, P)
        assert x == y, (t, x, y)
        if x is None:
            continue
        found += 1
        score, blocks, id_n = x
        assert S.path_score(a, b, blocks, P) == score >= P['min_score']   # the path is worth the best H
        assert id_n == sum(int(a[i + c] == b[j + c] and a[i + c] < 4) for i, j, ln in blocks for c in range(ln))
        for (i, j, ln), (i2, j2, _) in zip(blocks, blocks[1:]):   # the contract of mimeo_path_block
            assert i2 >= i + ln and j2 >= j + ln and (i2 - i - ln) + (j2 - j - ln) > 0
        assert all(ln >= 1 for _, _, ln in blocks) and blocks[-1][0] + blocks[-1][2] <= w and blocks[-1][1] + blocks[-1][2] <= w
    assert found > 200


def test_restatements_agree_on_designed_inputs():
    c = S.codes
    P = S.params(min_score=1)
    # a perfect repeat: one block, the best cell at its end
    assert S.gotoh_loops(c(b'ACGTACGGTA'), c(b'ACGTACGGTA'), P) == S.gotoh_sweep(c(b'ACGTACGGTA'), c(b'ACGTACGGTA'), P) == (20, [(0, 0, 10)], 10)
    # N never matches, not even N; lower case is the letter
    assert S.gotoh_sweep(c(b'ACNNGT'), c(b'ACNNGT'), P) == (4, [(0, 0, 2)], 2)
    assert S.gotoh_sweep(c(b'acgtac'), c(b'ACGTAC'), P) == (12, [(0, 0, 6)], 6)
    # ties between cells: the smallest i, then the smallest j
    assert S.gotoh_sweep(c(b'GTTTTGAC'), c(b'ACCCCCAC'), P) == S.gotoh_loops(c(b'GTTTTGAC'), c(b'ACCCCCAC'), P) == (4, [(6, 0, 2)], 2)
    assert S.gotoh_sweep(c(b'ACTTTTAC'), c(b'GGGGGGAC'), P)[1] == [(0, 6, 2)]
    # a homopolymer of another length: the traceback prefers the diagonal, so the gap lands at the run's far end
    a, b = c(b'GATTACAGCAAAAATCGGCTTAGC'), c(b'GATTACAGCAAAAAAATCGGCTTA')
    x = S.gotoh_loops(a, b, P)
    assert x == S.gotoh_sweep(a, b, P) and x[0] == 2 * 22 - 5 - 4 and x[1] == [(0, 0, 9), (9, 11, 13)]
    # nothing found: below the threshold, and the empty window
    assert S.gotoh_sweep(c(b'ACGT'), c(b'ACGT'), S.params()) is None and S.gotoh_loops(c(b'ACGT'), c(b'ACGT'), S.params()) is None
    assert S.gotoh_sweep(c(b''), c(b''), P) is None
    assert S.gotoh_sweep(c(b'AAAA'), c(b'CCCC'), P) is None
    # the records: both orientations, plus-strand coordinates of the inverted one
    seq = b'TTGACCATGCATCAGGCTAA' + b'C' * 15 + b'A' * 15 + b'TTAGCCTGATGCATGGTCAA'
    recs, first, blocks = S.terminal_repeats([seq], [(0, 0, 70), (0, 0, 0), (0, 3, 4)], gotoh=S.gotoh_loops, min_score=30)
    assert first.tolist() == [0, 0, 1, 1, 1, 1, 1] and recs['qstrand'].tolist() == [0, 1] * 3
    r = recs[1]
    assert (r['tstart'], r['tend'], r['qstart'], r['qend'], r['score'], r['id_n'], r['id_d']) == (0, 20, 50, 70, 40, 20, 20)
    assert blocks.tolist() == [(0, 0, 20)]   # the tail ends at the scaffold's last base: base 0 of the stored reverse complement
    assert all(int(recs[k][f]) == 0 for k in (0, 2, 3, 4, 5) for f in recs.dtype.names if f != 'qstrand')
    st = S.column_stats([seq], recs, first, blocks)
    assert st[1]['matches'] == 20 and int(st['matches'].sum()) == 20
    assert S.windows(3, 10, 50, 1024) == (3, 3, 7, 40) and S.windows(3, 4, 50, 1024)[0] == 0 and S.windows(0, 50, 50, 7) == (7, 0, 43, 0)


def test_sweep_at_the_largest_window():
    rng = np.random.default_rng(3)
    a = rng.integers(0, 4, 1024).astype(np.uint8)
    b = a.copy()
    b[::29] = (b[::29] + 1) % 4
    b = np.concatenate([b[:500], b[504:], rng.integers(0, 4, 4).astype(np.uint8)])
    P = S.params()
    score, blocks, id_n = S.gotoh_sweep(a, b, P)
    assert S.path_score(a, b, blocks, P) == score and len(blocks) == 2 and blocks[1][0] - blocks[0][0] - blocks[0][2] == 4


def test_terminal_repeat_lines_by_hand():
    regions = np.zeros(3, dtype=_ffi.INTERVAL)
    regions['chrom'], regions['start'], regions['end'] = [1, 0, 0], [100, 5, 900], [2100, 45, 1500]
    recs = np.zeros(6, dtype=_ffi.ALIGNMENT)
    stats = np.zeros(6, dtype=_ffi.COLUMN_STATS)
    recs['qstrand'] = [0, 1] * 3
    recs[0] = (1, 1, 100, 352, 1850, 2100, 466, 240, 250, 0, 0)
    stats[0] = (240, 6, 4, 0, 1, 0, 1, 2)
    recs[5] = (0, 0, 900, 930, 1470, 1500, 60, 30, 30, 1, 0)
    stats[5] = (30, 0, 0, 0, 0, 0, 0, 0)
    recs[4] = (0, 0, 901, 921, 1400, 1420, 40, 10, 20, 0, 0)
    stats[4] = (10, 10, 0, 0, 0, 0, 0, 0)   # saturated: no kd
    lines = formats.terminal_repeat_lines(regions, ['a', 'b'], 'Rep', 1024, recs, stats)
    assert lines[0] == formats.TERMINAL_REPEATS_HEADER == '\t'.join(
        ['#feature', 'seqid', 'start', 'end', 'kind', 'window', 'left_start', 'left_end', 'right_start', 'right_end', 'score', 'columns', 'matches', 'ts', 'tv',
         'ambiguous', 'gap_runs', 'gap_bases', 'identity', 'kd'])
    kd = formats.divergence_values(stats[0])[3]
    assert lines[1].split('\t') == ['Rep_00001', 'b', '100', '2100', 'LTR', '1000', '100', '352', '1850', '2100', '466', '250', '240', '6', '4', '0', '2', '2',
                                    '0.9600', '%.4f' % kd]
    assert lines[2].split('\t') == ['Rep_00003', 'a', '900', '1500', 'LTR', '300', '901', '921', '1400', '1420', '40', '20', '10', '10', '0', '0', '0', '0', '0.5000', '.']
    assert lines[3].split('\t') == ['Rep_00003', 'a', '900', '1500', 'TIR', '300', '900', '930', '1470', '1500', '60', '30', '30', '0', '0', '0', '0', '0', '1.0000',
                                    '0.0000']
    assert len(lines) == 4   # the second region has neither
    assert formats.terminal_repeat_lines(regions, ['a', 'b'], 'Rep', 20, recs, stats, header=False)[0].split('\t')[5] == '20'
    assert formats.terminal_repeat_lines(regions[:0], ['a'], 'Rep', 1024, recs[:0], stats[:0]) == [formats.TERMINAL_REPEATS_HEADER]


def test_cli_flags(capsys):
    from mimeo_amd import run_filter, run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    args = run_self.mainArgs(base)
    assert (args.terminalRepeats, args.terminalWindow, args.terminalMinScore) == (None, 1024, 40)
    args = run_self.mainArgs(base + ['--terminalRepeats', 't.tsv'])   # needs none of --paf, --families, --consensus
    assert (args.terminalRepeats, args.paf, args.families, args.consensus) == ('t.tsv', None, None, None)
    args = run_self.mainArgs(base + ['--terminalRepeats', 't.tsv', '--terminalWindow', '4096', '--terminalMinScore', '1', '--strictSelf'])
    assert (args.terminalWindow, args.terminalMinScore, args.strictSelf) == (4096, 1, True)
    for bad, text in ((['--terminalWindow', '0'], '--terminalWindow must be in 1..4096'), (['--terminalWindow', '4097'], '--terminalWindow must be in 1..4096'),
                      (['--terminalMinScore', '0'], '--terminalMinScore must be at least 1'), (['--terminalRepeats'], 'expected one argument')):
        with pytest.raises(SystemExit) as e:
            run_self.mainArgs(base + bad)
        assert e.value.code == 2 and text in capsys.readouterr().err
    for flag in ('--terminalRepeats', '--terminalWindow', '--terminalMinScore'):
        for mod, b2 in ((run_interspecies, base + ['--bfasta', 'b.fa']), (run_map, base + ['--bfasta', 'b.fa']), (run_filter, ['--infile', 'x.fa'])):
            with pytest.raises(SystemExit) as e:   # self only
                mod.mainArgs(b2 + [flag, '7'])
            assert e.value.code == 2
            assert 'unrecognized arguments: %s' % flag in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run_self.mainArgs(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--terminalRepeats FILE' in text and 'kind LTR' in text and 'kind TIR' in text and '19..25' in text and 'perfect 20-base repeat' in text


def test_workflow_refuses_terminal_repeats_of_two_genomes():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='terminal_repeats needs a self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), terminal_repeats='t.tsv')
    with pytest.raises(ValueError, match='terminal_window must be in 1..4096'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', terminal_repeats='t.tsv', terminal_window=0)
    with pytest.raises(ValueError, match='terminal_min_score must be at least 1'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', terminal_repeats='t.tsv', terminal_min_score=0)


def test_terminal_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'terminal_check.cc')
    exe = tmp_path / 'terminal_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'terminal_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
