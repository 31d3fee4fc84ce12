"""Alignment text, host side: formats.maf_lines and formats.cs_tag on hand-written rows, the PAF writer with cs:Z:, the --maf /
--cs options of the command line, the symbol, and the host side of mimeo_path_text (mimeo_amd/csrc/path_text_host.h) under
the sanitizers as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(*pairs):
    """(row_first, trow, qrow) of hand-written (target row, query row) strings"""
    first = np.zeros(len(pairs) + 1, dtype=np.uint64)
    first[1:] = np.cumsum([len(t) for t, _ in pairs])
    assert all(len(t) == len(q) for t, q in pairs)
    return (first, np.frombuffer(''.join(t for t, _ in pairs).encode(), dtype=np.uint8), np.frombuffer(''.join(q for _, q in pairs).encode(), dtype=np.uint8))


def _cs(t, q):
    return formats.cs_tag(np.frombuffer(t.encode(), dtype=np.uint8), np.frombuffer(q.encode(), dtype=np.uint8))


def test_cs_tag_by_hand():
    # a record without gaps: ':<n>' alone
    assert _cs('ACGTACGT', 'ACGTACGT') == ':8'
    # substitutions one column each, target letter first
    assert _cs('ACGTAC', 'ACCAAC') == ':2*gc*ta:2'
    # an insertion next to a deletion: the insertion first
    assert _cs('AC--GTTA', 'ACTG--TA') == ':2+tg-gt:2'
    assert _cs('ACGT-A', 'A--TCA') == ':1-cg:1+c:1'
    # N over N is a column of its own kind, never a match; N over A and A over N likewise
    assert _cs('ANNA', 'ANAA') == ':1*nn*na:1'
    assert _cs('AACA', 'ANCA') == ':1*an:2'
    # a column of N at a row's first and last position
    assert _cs('NCGTN', 'NCGTN') == '*nn:3*nn'
    assert _cs('NCGTA', 'ACGTN') == '*na:3*an'
    # N inside gaps
    assert _cs('A-NA', 'ANNA') == ':1+n*nn:1'
    assert _cs('ANA', 'A-A') == ':1-n:1'
    # an empty record
    assert _cs('', '') == ''
    with pytest.raises(ValueError):
        _cs('AC', 'A')
    # the ':' lengths sum to the matches, and the walk gives the CIGAR back
    tag = _cs('ACGT--ACGTNACGTACG', 'ACTTGGAC--NACGTAAG')
    assert tag == ':2*gt:1+gg:2-gt*nn:5*ca:1'
    assert sum(int(x) for x in re.findall(r':(\d+)', tag)) == 11


def _rec(tid, qid, tstart, tend, qstart, qend, score, qstrand):
    r = np.zeros(1, dtype=_ffi.ALIGNMENT)
    r['tid'], r['qid'], r['tstart'], r['tend'], r['qstart'], r['qend'], r['score'], r['qstrand'] = tid, qid, tstart, tend, qstart, qend, score, qstrand
    return r


def test_maf_lines_by_hand():
    # a '+' record with an insertion next to a deletion, a '-' record, an empty record
    recs = np.concatenate([_rec(0, 1, 100, 108, 50, 58, 4000, 0), _rec(0, 0, 200, 206, 780, 785, 3500, 1), _rec(0, 1, 7, 7, 9, 9, 0, 0),
                           _rec(0, 0, 7, 7, 30, 30, 0, 1)])
    blocks = np.array([(100, 50, 3), (105, 55, 3), (200, 15, 2), (203, 17, 3)], dtype=_ffi.PATH_BLOCK)
    first = np.array([0, 2, 4, 4, 4], dtype=np.uint64)
    row_first, trow, qrow = _rows(('ACG--TTACG', 'ACGNA--ACT'), ('GANCCA', 'GA-CCA'), ('', ''), ('', ''))
    got = formats.maf_lines(recs, row_first, trow, qrow, first, blocks, ['chrT'], [1000], ['chrQ', 'q2'], [800, 500])
    assert got == [
        'a score=4000\ns chrT 100 8 + 1000 ACG--TTACG\ns q2 50 8 + 500 ACGNA--ACT\n',
        # the query start of a '-' row is on the aligned strand: the first block's q = 800 - 785
        'a score=3500\ns chrT 200 6 + 1000 GANCCA\ns chrQ 15 5 - 800 GA-CCA\n',
        'a score=0\ns chrT 7 0 + 1000 \ns q2 9 0 + 500 \n',
        'a score=0\ns chrT 7 0 + 1000 \ns chrQ 770 0 - 800 \n',
    ]
    assert formats.MAF_HEADER == '##maf version=1 scoring=mimeo-amd'
    # the column count of a row from its path alone
    assert formats.path_columns(first, blocks).tolist() == [10, 6, 0, 0]
    assert formats.cs_tags(row_first, trow, qrow) == [':3+na-tt:2*gt', ':2-n:3', '', '']


PLAIN = [   # the lines tests/test_host_paths.py::test_cigar_and_paf_lines_by_hand expects of the same inputs
    'chrQ\t800\t50\t108\t+\tchrT\t1000\t100\t160\t50\t63\t255\tAS:i:4000\tcg:Z:20M3I15M5D20M',
    'chrQ\t800\t458\t500\t-\tchrT\t1000\t200\t240\t38\t42\t255\tAS:i:3500\tcg:Z:10M2I30M',
]


def test_paf_lines_with_cs():
    def rec(tstart, tend, qstart, qend, score, id_n, id_d, qstrand):
        r = _rec(0, 0, tstart, tend, qstart, qend, score, qstrand)
        r['id_n'], r['id_d'] = id_n, id_d
        return r
    blocks = np.array([(100, 50, 20), (120, 73, 15), (140, 88, 20), (200, 300, 10), (210, 312, 30)], dtype=_ffi.PATH_BLOCK)
    first = np.array([0, 3, 5], dtype=np.uint64)
    recs = np.concatenate([rec(100, 160, 50, 108, 4000, 50, 55, 0), rec(200, 240, 458, 500, 3500, 38, 40, 1)])
    args = (recs, first, blocks, ['chrT'], [1000], ['chrQ'], [800])
    assert formats.paf_lines(*args) == PLAIN and formats.paf_lines(*args, cs=None) == PLAIN
    got = formats.paf_lines(*args, cs=[':20+acg:15-ttttt:20', ':10+aa:30'])
    assert got == [PLAIN[0] + '\tcs:Z::20+acg:15-ttttt:20', PLAIN[1] + '\tcs:Z::10+aa:30']
    assert all(g.startswith(p) for g, p in zip(got, PLAIN))   # the row without it is a prefix
    # behind the divergence tags as well: cs:Z: is the last field
    stats = np.zeros(2, dtype=_ffi.COLUMN_STATS)
    both = formats.paf_lines(*args, stats=stats, cs=['x', 'y'])
    assert both == [l + '\tcs:Z:' + c for l, c in zip(formats.paf_lines(*args, stats=stats), 'xy')]


def test_text_runs_and_file_order():
    from mimeo_amd import workflow
    cols = [5, 5, 5, 100, 1, 0, 9, 10]
    assert workflow.text_runs(cols, 10) == [(0, 2), (2, 3), (3, 4), (4, 7), (7, 8)]   # a single longer row goes alone
    assert workflow.text_runs(cols, 1000) == [(0, 8)] and workflow.text_runs([], 10) == []
    assert workflow.text_runs(cols, 0) == [(i, i + 1) for i in range(8)]
    blocks = {(0, 0): ['a', 'b'], (0, 1): ['c'], (1, 0): ['d', 'e', 'f'], (1, 1): ['g']}
    pairs = [(1, 1), (0, 1), (0, 0), (1, 0), (2, 2)]
    assert workflow.file_order(pairs, blocks).tolist() == [6, 2, 0, 1, 3, 4, 5]
    assert workflow.file_order(pairs, blocks, splitSelf=True).tolist() == [2, 3, 4, 5, 6, 0, 1]
    assert workflow.file_order(pairs, {}).size == 0


def test_cs_needs_paf(capsys):
    from mimeo_amd import run_interspecies, run_map, run_self
    for mod, base in ((run_self, ['--afasta', 'a.fa']), (run_interspecies, ['--afasta', 'a.fa', '--bfasta', 'b.fa']),
                      (run_map, ['--afasta', 'a.fa', '--bfasta', 'b.fa'])):
        args = mod.mainArgs(base)
        assert args.cs is False and args.maf is None
        with pytest.raises(SystemExit) as e:
            mod.mainArgs(base + ['--cs'])
        assert e.value.code == 2
        assert '--cs needs --paf' in capsys.readouterr().err
        args = mod.mainArgs(base + ['--paf', 'x.paf', '--cs'])
        assert args.cs is True and args.paf == 'x.paf'
        assert mod.mainArgs(base + ['--maf', 'x.maf']).maf == 'x.maf'   # --maf needs no --paf
        with pytest.raises(SystemExit) as e:
            mod.mainArgs(['--help'])
        assert e.value.code == 0
        text = capsys.readouterr().out
        assert '--maf FILE' in text and '--cs' in text
        assert 'neither case nor IUPAC' in ' '.join(text.split())   # what the letters are is said where the user reads it


def test_path_text_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_text' in declared and 'mimeo_path_text' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr)
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_text') and len(lib.mimeo_path_text.argtypes) == 10


def test_path_text_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'path_text_check.cc')
    assert re.search(r'^int main\(', open(src).read(), re.M)   # a stand-alone program: nothing of it is loaded into this process
    exe = tmp_path / 'path_text_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'path_text_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
