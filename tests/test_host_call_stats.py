"""Copy-to-consensus divergence, host side: the layout of mimeo_call_stats and the declaration of mimeo_path_call_stats against the
binding, the representative's own row, the copy divergence file and the landscape (formats.own_call_stats,
formats.copy_divergence_lines, formats.landscape_lines) worked out by hand, the --copyDivergence and --landscape options of
`mimeo self`, and the host side of mimeo_path_call_stats (mimeo_amd/csrc/call_stats_host.h) under the sanitizers as a stand-alone
program."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_bases', 'del_bases', 'q_lo', 'q_hi')


def _rows(dtype, *rows):
    r = np.zeros(len(rows), dtype=dtype)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def test_call_stats_layout_binding_and_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    dt = _ffi.CALL_STATS
    assert dt.itemsize == 32 and dt.names == FIELDS and formats.CALL_STATS == dt
    assert [dt.fields[n] for n in FIELDS] == [(np.dtype('<u4'), k) for k in range(0, 32, 4)]
    m = re.search(r'typedef struct mimeo_call_stats \{(.*?)\} mimeo_call_stats;\s*/\* (\d+) bytes \*/', hdr, re.S)
    assert m
    body = re.sub(r'/\*.*?\*/', '', m.group(1))
    assert tuple(re.findall(r'\b([a-z_0-9]+)\s*[,;]', body)) == FIELDS
    assert set(re.findall(r'\b(u?int\d+_t)\b', body)) == {'uint32_t'} and int(m.group(2)) == dt.itemsize
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_call_stats' in declared and 'mimeo_path_call_stats' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    assert '"Pileup v4, rows against the call"' in hdr
    # the declaration, argument by argument, against the binding: pointers as void *, the counts 64 bits
    m = re.search(r'int mimeo_path_call_stats\((.*?)\);', hdr, re.S)
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['T', 'Q', 'aln', 'n', 'path_first', 'blocks', 'nblocks', 'windows', 'nwin', 'items', 'nitems',
                                                         'sites', 'nsites', 'call', 'icall', 'out']
    # up to nsites the arguments are those of mimeo_path_stack, word for word
    p = re.search(r'int mimeo_path_stack\((.*?)\);', hdr, re.S)
    assert args[:13] == [a.strip() for a in re.sub(r'/\*.*?\*/', '', p.group(1)).split(',')][:13]
    assert args[13:] == ['const uint8_t *call', 'const uint8_t *icall', 'mimeo_call_stats *out']
    want = [C.c_void_p if '*' in a else {'uint64_t': C.c_uint64}[a.split()[0]] for a in args]
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_call_stats') and list(lib.mimeo_path_call_stats.argtypes) == want
    for name in _ffi.SYMBOLS:   # exported by the library that was built, beside the old symbols
        assert hasattr(lib, name), name
    from mimeo_amd import engine
    assert callable(engine.call_stats)


def test_own_call_stats_by_hand():
    """three windows, the second empty.  Window 0 = [10, 18): own ACGTNACG under the call AC-CNGTA, column by column A/A and C/C
    matches, '-' a base that the consensus lacks, C/T a transition, N/N ambiguous, then G/A, T/C and A/G transitions.  Its two
    sites `T-` and `GN-` hold three letter columns: three bases that the representative lacks.  Window 2 = [3, 5) without a
    site: N/T ambiguous, A/T a transversion."""
    win = _rows(_ffi.PILEUP_WINDOW, (0, 10, 18), (1, 7, 7), (1, 3, 5))
    own = np.frombuffer(b'ACGTNACG' + b'TT', dtype=np.uint8)
    call = np.frombuffer(b'AC-CNGTA' + b'NA', dtype=np.uint8)
    sites = _rows(_ffi.INSERT_SITE, (0, 10, 2, 3), (0, 15, 3, 3))
    icall = np.frombuffer(b'T-' + b'GN-', dtype=np.uint8)
    got = formats.own_call_stats(own, call, sites, icall, win)
    assert got.dtype == formats.CALL_STATS and got.tolist() == [(2, 4, 0, 1, 1, 3, 10, 18), (0, 0, 0, 0, 0, 0, 7, 7), (0, 0, 1, 1, 0, 0, 3, 5)]
    # transversions: A<->C, A<->T, G<->C, G<->T
    got = formats.own_call_stats(np.frombuffer(b'ACGTAG', dtype=np.uint8), np.frombuffer(b'CATGTC', dtype=np.uint8), sites[:0], icall[:0],
                                 _rows(_ffi.PILEUP_WINDOW, (0, 0, 6)))
    assert got.tolist() == [(0, 0, 6, 0, 0, 0, 0, 6)]
    assert formats.own_call_stats(own[:0], call[:0], sites[:0], icall[:0], win[:0]).size == 0


def _s(m, ts, tv, amb=0, ins=0, dl=0, q_lo=0, q_hi=0):
    return _rows(formats.CALL_STATS, (m, ts, tv, amb, ins, dl, q_lo, q_hi))[0]


def test_copy_stretch():
    assert formats.copy_stretch(1000, 0, 0, 10) == (0, 10, '+')
    # the aligned strand is the reverse complement: its bases [0, 10) are the plus strand's last ten
    assert formats.copy_stretch(1000, 1, 0, 10) == (990, 1000, '-')
    assert formats.copy_stretch(1000, 1, 990, 1000) == (0, 10, '-')
    # the same bases as stockholm_row_name names 1-based
    assert formats.stockholm_row_name('c', 1000, 1, 7, 30) == 'c/993-971' and formats.copy_stretch(1000, 1, 7, 30) == (970, 993, '-')


def test_copy_divergence_lines_by_hand():
    kd = lambda p, q: -0.5 * math.log((1 - 2 * p - q) * math.sqrt(1 - 2 * q))
    members = [('F1', 'rep', 'chrA', 100, 200, '+', _s(90, 6, 4, 0, 2, 3)),
               ('F1', 'copy', 'chrB', 5, 104, '-', _s(99, 0, 0)),
               ('F1', 'copy', 'chrB', 300, 320, '+', _s(5, 5, 10)),       # saturated: 1 - 2P - Q = 0
               ('F2_intra', 'copy', 'chrA', 0, 3, '+', _s(0, 0, 0, 3))]   # no unambiguous column
    lines = formats.copy_divergence_lines(members)
    assert lines[0] == '#family\trole\tseqid\tstart\tend\tstrand\tmatches\ttransitions\ttransversions\tambiguous\tins_bases\tdel_bases\tdiv\tkd'
    assert lines[0] == formats.COPY_DIVERGENCE_HEADER
    assert lines[1] == 'F1\trep\tchrA\t100\t200\t+\t90\t6\t4\t0\t2\t3\t0.1000\t%.4f' % kd(0.06, 0.04)
    assert lines[1].endswith('\t0.1080')
    assert lines[2] == 'F1\tcopy\tchrB\t5\t104\t-\t99\t0\t0\t0\t0\t0\t0.0000\t0.0000'
    assert lines[3] == 'F1\tcopy\tchrB\t300\t320\t+\t5\t5\t10\t0\t0\t0\t0.7500\tNA'
    assert lines[4] == 'F2_intra\tcopy\tchrA\t0\t3\t+\t0\t0\t0\t3\t0\t0\tNA\tNA'
    assert len(lines) == 5 and formats.copy_divergence_lines(members, header=False) == lines[1:]
    assert formats.copy_divergence_lines([]) == [formats.COPY_DIVERGENCE_HEADER]


def test_landscape_bins():
    """a copy exactly on a bin edge belongs to the bin that starts there, for every edge as the decimal is written"""
    for k in range(50):
        assert formats.landscape_bin(float('%.2f' % (k / 100))) == k, k
        assert formats.landscape_bin(math.nextafter(k / 100, 1.0)) == k
        if k:
            assert formats.landscape_bin(math.nextafter(k / 100, 0.0)) == k - 1
    assert formats.landscape_bin(0.29) == 29 and int(0.29 / 0.01) == 28   # why the edges are not divided
    assert formats.landscape_bin(0.5) == 50 and formats.landscape_bin(0.4999999) == 49 and formats.landscape_bin(7.0) == 50
    assert formats.landscape_bin(None) == 51


def test_landscape_lines_by_hand():
    # kd of (m, ts, tv) = (100, 0, 0) is 0: on the edge of the first bin; (90, 6, 4): 0.1080; (45, 3, 2), the same ratios: the same bin
    members = [('F1', 'rep', 'a', 0, 100, '+', _s(100, 0, 0, 2)),
               ('F1', 'copy', 'b', 0, 100, '+', _s(90, 6, 4, 1, 9, 9)),   # ins_bases and del_bases are no bases of the landscape
               ('F1', 'copy', 'c', 0, 50, '-', _s(45, 3, 2)),
               ('F1', 'copy', 'c', 0, 20, '+', _s(5, 5, 10)),             # saturated
               ('F3', 'rep', 'a', 500, 600, '+', _s(100, 0, 0)),
               ('F3', 'copy', 'a', 700, 720, '+', _s(10, 0, 10)),         # Q = 0.5: saturated as well
               ('F3', 'copy', 'a', 800, 900, '+', _s(60, 20, 20))]        # P = Q = 0.2: kd = 0.5859, beyond 0.50
    kd = formats.divergence_values({'matches': 60, 'transitions': 20, 'transversions': 20, 'ambiguous': 0, 'ins_runs': 0, 'del_runs': 0})[3]
    assert round(kd, 4) == 0.5859
    lines = formats.landscape_lines(members, families=['F1', 'F2', 'F3'])   # F2: an empty family writes nothing
    assert lines == ['#family\tkd_lo\tkd_hi\tcopies\tbases',
                     'F1\t0.00\t0.01\t1\t102', 'F1\t0.10\t0.11\t2\t151', 'F1\tNA\tNA\t1\t20',
                     'F3\t0.00\t0.01\t1\t100', 'F3\t0.50\tinf\t1\t100', 'F3\tNA\tNA\t1\t20',
                     'all\t0.00\t0.01\t2\t202', 'all\t0.10\t0.11\t2\t151', 'all\t0.50\tinf\t1\t100', 'all\tNA\tNA\t2\t40']
    assert formats.landscape_lines(members) == lines   # the families in the order of their first member
    assert formats.landscape_lines(members, header=False) == lines[1:]
    assert formats.landscape_lines([]) == [formats.LANDSCAPE_HEADER]
    # a copy exactly on an edge: Kimura's distance of identical sequences is 0.0, the first bin's lower edge
    assert formats.landscape_lines([('F1', 'copy', 'a', 0, 9, '+', _s(9, 0, 0))], header=False) == ['F1\t0.00\t0.01\t1\t9', 'all\t0.00\t0.01\t1\t9']


def test_copy_divergence_and_landscape_options(capsys):
    from mimeo_amd import run_filter, run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    args = run_self.mainArgs(base)
    assert args.copyDivergence is None and args.landscape is None
    args = run_self.mainArgs(base + ['--copyDivergence', 'd.tsv'])   # each flag works alone and needs none of the others
    assert (args.copyDivergence, args.landscape, args.families, args.consensus, args.familyAlignments, args.familyCover) == ('d.tsv', None, None, None, None, 80)
    args = run_self.mainArgs(base + ['--landscape', 'l.tsv'])
    assert (args.copyDivergence, args.landscape, args.families, args.consensus, args.familyAlignments) == (None, 'l.tsv', None, None, None)
    args = run_self.mainArgs(base + ['--landscape', 'l.tsv', '--copyDivergence', 'd.tsv', '--familyCover', '60', '--strictSelf'])
    assert (args.copyDivergence, args.landscape, args.familyCover, args.strictSelf) == ('d.tsv', 'l.tsv', 60, True)
    with pytest.raises(SystemExit) as e:   # --familyCover applies
        run_self.mainArgs(base + ['--landscape', 'l.tsv', '--familyCover', '0'])
    assert e.value.code == 2 and '--familyCover must be in 1..100' in capsys.readouterr().err
    for flag in ('--copyDivergence', '--landscape'):
        with pytest.raises(SystemExit) as e:
            run_self.mainArgs(base + [flag])
        assert e.value.code == 2
        capsys.readouterr()
        for mod, b2 in ((run_interspecies, base + ['--bfasta', 'b.fa']), (run_map, base + ['--bfasta', 'b.fa']), (run_filter, ['--infile', 'x.fa'])):
            with pytest.raises(SystemExit) as e:   # self only
                mod.mainArgs(b2 + [flag, 'x.tsv'])
            assert e.value.code == 2
            assert 'unrecognized arguments: %s' % flag in capsys.readouterr().err


def test_workflow_refuses_copy_divergence_of_two_genomes():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='copy_divergence needs a self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), copy_divergence='d.tsv')
    with pytest.raises(ValueError, match='landscape needs a self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), landscape='l.tsv')
    for flag in ('copy_divergence', 'landscape'):
        with pytest.raises(ValueError, match='family_cover must be in 1..100'):
            workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', family_cover=0, **{flag: 'x.tsv'})


def test_call_stats_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'call_stats_check.cc')
    exe = tmp_path / 'call_stats_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'call_stats_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
