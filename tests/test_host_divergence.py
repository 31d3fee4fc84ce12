"""Alignment divergence, host side: the tags of formats.divergence_tags worked out by hand, the PAF writer with and without
statistics, the --divergence / --paf rule of the command line, the layout of mimeo_column_stats, and the host checks of
mimeo_path_stats (mimeo_amd/csrc/path_stats_host.h) under the sanitizers as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_runs', 'ins_bases', 'del_runs', 'del_bases')


def _stats(*rows):
    s = np.zeros(len(rows), dtype=_ffi.COLUMN_STATS)
    for i, r in enumerate(rows):
        for k, v in zip(FIELDS, r):
            s[k][i] = v
    return s


def _tags(*row):
    return formats.divergence_tags(_stats(row)[0]).split('\t')


def test_divergence_tags_by_hand():
    # mism = 15; NM = 15 + 3 + 4; de = (15 + 3 runs) / (85 + 15 + 3) = 18 / 103; P = 0.10, Q = 0.05:
    # -0.5 ln(0.75 * sqrt(0.9)) = -0.5 ln(0.711512) = 0.170185
    assert _tags(85, 10, 5, 0, 1, 3, 2, 4) == ['NM:i:22', 'de:f:0.1748', 'ts:i:10', 'tv:i:5', 'kd:f:0.1702']
    # identical sequences: no minus sign in front of a zero
    assert _tags(100, 0, 0, 0, 0, 0, 0, 0) == ['NM:i:0', 'de:f:0.0000', 'ts:i:0', 'tv:i:0', 'kd:f:0.0000']
    # 1 - 2P - Q = 0.1 is still defined: -0.5 ln(0.1 * sqrt(0.4)) = 1.380364
    assert _tags(40, 30, 30, 0, 0, 0, 0, 0) == ['NM:i:60', 'de:f:0.6000', 'ts:i:30', 'tv:i:30', 'kd:f:1.3804']
    # 1 - 2Q = 0: saturated, no kd
    assert _tags(50, 0, 50, 0, 0, 0, 0, 0) == ['NM:i:50', 'de:f:0.5000', 'ts:i:0', 'tv:i:50']
    # 1 - 2P - Q = 0
    assert _tags(50, 25, 0, 0, 0, 0, 0, 0)[-1].startswith('kd:f:') and _tags(50, 50, 0, 0, 0, 0, 0, 0)[-1] == 'tv:i:0'
    # all ambiguous: n = 0, every column a mismatch
    assert _tags(0, 0, 0, 10, 0, 0, 0, 0) == ['NM:i:10', 'de:f:1.0000', 'ts:i:0', 'tv:i:0']
    # ambiguous columns count in NM and de, not in kd: n = 90
    assert _tags(80, 10, 0, 10, 0, 0, 0, 0) == ['NM:i:20', 'de:f:0.2000', 'ts:i:10', 'tv:i:0', 'kd:f:%.4f' % (-0.5 * np.log(1 - 2 * 10 / 90))]
    # a mapping serves as well as a row of the structured array
    assert formats.divergence_tags(dict(zip(FIELDS, (85, 10, 5, 0, 1, 3, 2, 4)))) == 'NM:i:22\tde:f:0.1748\tts:i:10\ttv:i:5\tkd:f:0.1702'


def _rec(tstart, tend, qstart, qend, score, id_n, id_d, qstrand):
    r = np.zeros(1, dtype=_ffi.ALIGNMENT)
    r['tstart'], r['tend'], r['qstart'], r['qend'], r['score'], r['id_n'], r['id_d'], r['qstrand'] = tstart, tend, qstart, qend, score, id_n, id_d, qstrand
    return r


PLAIN = [   # the lines tests/test_host_paths.py::test_cigar_and_paf_lines_by_hand expects of the same inputs
    'chrQ\t800\t50\t108\t+\tchrT\t1000\t100\t160\t50\t63\t255\tAS:i:4000\tcg:Z:20M3I15M5D20M',
    'chrQ\t800\t458\t500\t-\tchrT\t1000\t200\t240\t38\t42\t255\tAS:i:3500\tcg:Z:10M2I30M',
    'q2\t500\t400\t427\t+\tchrT\t1000\t300\t324\t20\t31\t255\tAS:i:3100\tcg:Z:12M7I4D8M',
    'q2\t500\t10\t110\t+\tchrT\t1000\t10\t110\t100\t100\t255\tAS:i:9100\tcg:Z:100M',
]


def test_paf_lines_with_and_without_stats():
    blocks = np.array([(100, 50, 20), (120, 73, 15), (140, 88, 20), (200, 300, 10), (210, 312, 30), (300, 400, 12), (316, 419, 8),
                       (10, 10, 100)], dtype=_ffi.PATH_BLOCK)
    first = np.array([0, 3, 5, 7, 8], dtype=np.uint64)
    recs = np.concatenate([_rec(100, 160, 50, 108, 4000, 50, 55, 0), _rec(200, 240, 458, 500, 3500, 38, 40, 1),
                           _rec(300, 324, 400, 427, 3100, 20, 20, 0), _rec(10, 110, 10, 110, 9100, 100, 100, 0)])
    recs['qid'] = [0, 0, 1, 1]
    args = (recs, first, blocks, ['chrT'], [1000], ['chrQ', 'q2'], [800, 500])
    assert formats.paf_lines(*args) == PLAIN
    assert formats.paf_lines(*args, stats=None) == PLAIN
    stats = _stats((50, 3, 2, 0, 1, 3, 1, 5), (38, 1, 1, 0, 1, 2, 0, 0), (20, 0, 0, 0, 1, 7, 1, 4), (100, 0, 0, 0, 0, 0, 0, 0))
    got = formats.paf_lines(*args, stats=stats)
    assert len(got) == 4
    for line, plain, s in zip(got, PLAIN, stats):
        f, p = line.split('\t'), plain.split('\t')
        assert f[:13] == p[:13] and f[-1] == p[-1] and len(f) == len(p) + 5
        assert f[13:-1] == formats.divergence_tags(s).split('\t')
    assert got[0].split('\t')[13:15] == ['NM:i:13', 'de:f:%.4f' % (7 / 57)]
    assert got[3].split('\t')[13:18] == ['NM:i:0', 'de:f:0.0000', 'ts:i:0', 'tv:i:0', 'kd:f:0.0000']


def test_divergence_needs_paf(capsys):
    from mimeo_amd import run_interspecies, run_map, run_self
    for mod, base in ((run_self, ['--afasta', 'a.fa']), (run_interspecies, ['--afasta', 'a.fa', '--bfasta', 'b.fa']),
                      (run_map, ['--afasta', 'a.fa', '--bfasta', 'b.fa'])):
        args = mod.mainArgs(base)
        assert args.divergence is False and args.paf is None
        with pytest.raises(SystemExit) as e:
            mod.mainArgs(base + ['--divergence'])
        assert e.value.code == 2
        assert '--divergence needs --paf' in capsys.readouterr().err
        args = mod.mainArgs(base + ['--paf', 'x.paf', '--divergence'])
        assert args.divergence is True and args.paf == 'x.paf'
        assert mod.mainArgs(base + ['--paf', 'x.paf']).divergence is False


def test_column_stats_layout_and_symbol():
    assert _ffi.COLUMN_STATS.itemsize == 32
    assert _ffi.COLUMN_STATS.names == FIELDS
    assert [_ffi.COLUMN_STATS.fields[n][1] for n in FIELDS] == list(range(0, 32, 4))
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_stats' in declared and 'mimeo_path_stats' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    m = re.search(r'typedef struct mimeo_column_stats \{(.*?)\} mimeo_column_stats;', hdr, re.S)
    assert m and tuple(re.findall(r'\b([a-z_]+)\s*[,;]', re.sub(r'/\*.*?\*/', '', m.group(1)))) == FIELDS
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr)
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_stats') and len(lib.mimeo_path_stats.argtypes) == 8


def test_path_stats_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'path_stats_check.cc')
    exe = tmp_path / 'path_stats_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'path_stats_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
