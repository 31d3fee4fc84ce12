"""Element structure (K18 mimeo_flank_repeats, K19 mimeo_open_frames, `mimeo self --elements`) without a device: the binding,
the two restatements of each specification against each other on random and designed inputs, formats.element_lines by hand, the
CLI flags, and the HIP-free host sides (mimeo_amd/csrc/flank_host.h, frames_host.h) under ASan and UBSan as a stand-alone
program."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from mimeo_amd import _ffi, formats
from tests import elements_cases as K
from tests import elements_spec as S
from tests import terminal_spec as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_structs_and_bindings():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    for name in ('mimeo_flank_params_default', 'mimeo_flank_repeats', 'mimeo_open_frames'):
        assert name in declared and name in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    m = re.search(r'typedef struct mimeo_flank_params \{(.*?)\} mimeo_flank_params;', hdr, re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    assert tuple(re.findall(r'\b([a-z_]+)(?:\[4\])?\s*;', body)) == _ffi.FlankParams.NAMES + ('reserved',)
    assert C.sizeof(_ffi.FlankParams) == 32 and [f[0] for f in _ffi.FlankParams._fields_] == list(_ffi.FlankParams.NAMES) + ['reserved']
    m = re.search(r'typedef struct mimeo_flank_repeat \{(.*?)\} mimeo_flank_repeat;', hdr, re.S)
    body = re.sub(r'/\*.*?\*/', '', m.group(1), flags=re.S)
    ctype = {'uint32_t': '<u4', 'uint16_t': '<u2', 'int8_t': '|i1'}
    fields = [(n.strip(), ctype[t]) for t, names in re.findall(r'(u?int\d+_t)\s+([a-z_, ]+);', body) for n in names.split(',')]
    assert fields == [(n, _ffi.FLANK_REPEAT[n].str) for n in _ffi.FLANK_REPEAT.names] and _ffi.FLANK_REPEAT.itemsize == 16
    m = re.search(r'typedef struct mimeo_open_frame \{(.*?)\} mimeo_open_frame;', hdr, re.S)
    assert tuple(n.strip() for n in m.group(1).replace('uint32_t', '').strip(' ;').split(',')) == _ffi.OPEN_FRAME.names and _ffi.OPEN_FRAME.itemsize == 16
    lib = _ffi.load()
    for name in _ffi.SYMBOLS:
        assert hasattr(lib, name), name
    vp = C.c_void_p
    assert list(lib.mimeo_flank_repeats.argtypes) == [vp, vp, C.c_uint64, C.POINTER(_ffi.FlankParams), vp]
    assert list(lib.mimeo_open_frames.argtypes) == [vp, vp, C.c_uint64, C.c_uint32, vp]
    P = _ffi.FlankParams()
    assert lib.mimeo_flank_params_default(C.byref(P)) == 0   # needs no device
    assert {n: getattr(P, n) for n in P.NAMES} == S.FLANK_DEFAULTS and list(P.reserved) == [0] * 4
    assert lib.mimeo_flank_params_default(None) == -1
    from mimeo_amd import engine
    assert callable(engine.flank_repeats) and callable(engine.open_frames)


def test_no_cpu_fallback():
    # a process that never called mimeo_init: MIMEO_ERR_NO_DEVICE before any argument is looked at, and nothing written
    code = ('import ctypes as C, sys; sys.path.insert(0, %r); import numpy as np; from mimeo_amd import _ffi; lib = _ffi.load(); P = _ffi.FlankParams(); '
            'lib.mimeo_flank_params_default(C.byref(P)); out = np.full(16, 7, np.uint8); '
            'rc = lib.mimeo_flank_repeats(None, None, 1, C.byref(P), out.ctypes.data); print(rc, int(out.min()), lib.mimeo_last_error().decode()); '
            'out = np.full(96, 7, np.uint8); rc = lib.mimeo_open_frames(None, None, 1, 0, out.ctypes.data); '
            'print(rc, int(out.min()), lib.mimeo_last_error().decode())' % ROOT)
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 2 and all(ln.startswith('-2 7 ') and 'no CPU fallback' in ln for ln in lines), r.stdout
    src = open(os.path.join(ROOT, 'mimeo_amd', 'engine.py')).read()
    for name in ('flank_repeats', 'open_frames'):
        body = src.split('def %s(' % name)[1].split('\ndef ')[0]
        assert "raise RuntimeError('libmimeo_hip.so has no mimeo_%s: rebuild the library')" % name in body


def test_restatements_agree_on_random_inputs():
    rng = np.random.default_rng(1819)
    found = 0
    for t in range(300):
        L = int(rng.integers(0, 140))
        c = rng.integers(0, int(rng.choice([2, 4, 5])), L).astype(np.uint8)   # two letters: duplications and ties everywhere; five: N
        a = int(rng.integers(0, L + 1))
        b = int(rng.integers(a, L + 1))
        P = S.flank_params(min_len=int(rng.integers(2, 7)), max_len=int(rng.integers(7, 33)), slack=int(rng.integers(0, 9)), max_mismatch=int(rng.integers(0, 3)))
        x, y = S.flank_loops(c, a, b, P), S.flank_numpy(c, a, b, P)
        assert x == y, (t, x, y, P)
        if x is not None:
            found += 1
            p, r, k, m, dl, dr = x
            assert p == a + dl - k and r == b + dr and 0 <= p and r + k <= L and a + dl <= b + dr and k - 3 * m >= P['min_len']
            assert m == sum(int(not (c[p + i] < 4 and c[p + i] == c[r + i])) for i in range(k)) <= P['max_mismatch']
        rc = T.revcomp_codes(c)
        f1, f2 = S.frames_loops(c, rc, a, b), S.frames_numpy(c, rc, a, b)
        assert f1 == f2, (t, f1, f2)
        for j, (s, e, cod, met) in enumerate(f1):
            assert (cod == 0 and (s, e, met) == (0, 0, 0)) or (a <= s < e <= b and e - s == 3 * cod and met <= cod and (s - a if j < 3 else b - e) % 3 == j % 3)
    assert found > 100


def test_restatements_agree_on_designed_inputs():
    for name, seqs, items, kw, expected in K.k18_cases():
        x, y = S.flank_repeats(seqs, items, impl=S.flank_loops, **kw), S.flank_repeats(seqs, items, **kw)
        assert x.tobytes() == y.tobytes(), name
        for r, e in zip(x, expected):
            assert e is None or (int(r['len']), int(r['mismatches']), int(r['dl']), int(r['dr'])) == e, (name, r, e)
    for name, seqs, items in K.k19_cases():
        small = [it for it in items if it[2] - it[1] < 200]
        assert S.open_frames(seqs, small, impl=S.frames_loops).tobytes() == S.open_frames(seqs, small).tobytes(), name
    s = K.k19_long()
    assert S.open_frames([s], [(0, 0, 10000)])[0, 0].tolist()[:3] == (0, 9999, 3333)
    # the answers by hand: TAA, ten sense codons, TAG, ATG and ten more, TGA
    run = K.sense_run(np.random.default_rng(2), 10)
    seq = K.cat(b'TAA', run, b'TAG', b'ATG', run, b'TGA', b'CC')
    for impl in (S.frames_loops, S.frames_numpy):
        got = S.open_frames([seq], [(0, 0, 74), (0, 3, 33), (0, 0, 2)], impl=impl)
        assert got[0, 0].tolist() == (36, 69, 11, 0) and got[1, 0].tolist()[:3] == (3, 33, 10) and not got[2]['codons'].any()
    # the minus strand in plus-strand coordinates: the reverse complement of an open stretch, one base in
    rc = np.array([{65: 84, 67: 71, 71: 67, 84: 65}[int(x)] for x in K.cat(b'TAA', b'ATG', run, b'TAG')[::-1]], dtype=np.uint8)
    got = S.open_frames([K.cat(b'G', rc, b'CCA')], [(0, 0, 43)])
    assert got[0, 3 + 0].tolist() == (4, 37, 11, 0)   # sigma 1, frame 0: 43 - 3 - 3 - 33 = 4


def test_chance_rate_of_the_defaults():
    """the bound of the header and of the flag's help: (2 slack + 1)^2 * 4^-min_len * 4/3 = 0.13 admissible candidates at a random site, at
    most; the share of random sites with a duplication stays below it"""
    rng = np.random.default_rng(4)
    c = rng.integers(0, 4, 300_000).astype(np.uint8)
    P = S.flank_params()
    hits = sum(S.flank_numpy(c, a, a + 100, P) is not None for a in range(100, 200_100, 100))
    assert 0.05 < hits / 2000 < 25 * 4.0 ** -4 * 4 / 3


def _row(**kw):
    row = dict(kind=None, tsd=None, orf=None, ends='AC..GT', el=(100, 1100))
    row.update(kw)
    return row


def test_element_lines_by_hand():
    regions = np.zeros(9, dtype=_ffi.INTERVAL)
    regions['chrom'], regions['start'], regions['end'] = [1] + [0] * 8, np.arange(9) * 5000 + 98, np.arange(9) * 5000 + 1102
    st = np.zeros(1, dtype=_ffi.COLUMN_STATS)[0]
    st['matches'], st['transitions'], st['transversions'] = 240, 6, 4
    tr = dict(left_len=250, right_len=251, score=466, stats=st)
    tsd, orf, short = (5, 'ACGTN', 0, 2, -1), (0, 2, 400, 1000, 200, 20), (1, 0, 400, 460, 20, 20)
    rows = [_row(kind='LTR', tsd=tsd, orf=orf, **tr), _row(kind='LTR', tsd=tsd, orf=short, **tr), _row(kind='LTR', orf=orf, **tr),
            _row(kind='TIR', tsd=tsd, orf=orf, **tr), _row(kind='TIR', tsd=tsd, orf=short, el=(100, 900), **tr), _row(kind='TIR', tsd=tsd, el=(100, 901), **tr),
            _row(kind='TIR', orf=orf, **tr), _row(orf=orf), _row(orf=short, ends=None, el=(40098, 40098))]
    lines = formats.element_lines(regions, ['a', 'b'], 'Rep', rows, min_orf=200)
    assert lines[0] == formats.ELEMENTS_HEADER == '\t'.join(
        ['#feature', 'seqid', 'start', 'end', 'kind', 'el_start', 'el_end', 'left_len', 'right_len', 'tr_score', 'tr_identity', 'tr_kd', 'tsd_len', 'tsd',
         'tsd_mismatches', 'tsd_shift', 'ends', 'orf_strand', 'orf_frame', 'orf_start', 'orf_end', 'orf_codons', 'orf_met_codons', 'class'])
    kd = '%.4f' % formats.divergence_values(st)[3]
    assert lines[1].split('\t') == ['Rep_00001', 'b', '98', '1102', 'LTR', '100', '1100', '250', '251', '466', '0.9600', kd, '5', 'ACGTN', '0', '2,-1', 'AC..GT', '+', '3',
                                    '400', '1000', '200', '180', 'LTR_retrotransposon']
    assert lines[2].split('\t')[17:] == ['-', '1', '400', '460', '20', '0', 'LTR_nonautonomous']
    assert lines[3].split('\t')[12:17] == ['.', '.', '.', '.', 'AC..GT'] and lines[3].endswith('\tLTR_candidate')
    assert [ln.split('\t')[-1] for ln in lines[4:]] == ['DNA_transposon', 'MITE', 'DNA_nonautonomous', 'TIR_candidate', 'coding_repeat', '.']
    assert formats.MITE_MAX_LEN == 800 and lines[5].split('\t')[5:7] == ['100', '900'] and lines[6].split('\t')[17:23] == ['.'] * 6
    assert lines[8].split('\t')[4:12] == ['.', '100', '1100', '.', '.', '.', '.', '.'] and lines[9].split('\t')[16] == '.'
    assert formats.element_lines(regions, ['a', 'b'], 'Rep', rows, min_orf=201)[1].endswith('\tLTR_nonautonomous')
    assert formats.element_lines(regions[:2], ['a', 'b'], 'Rep', rows[:2], header=False)[0].startswith('Rep_00001\t')
    assert formats.element_lines(regions[:0], ['a'], 'Rep', []) == [formats.ELEMENTS_HEADER]


def test_restated_pipeline_on_a_planted_element():
    # TSD . TIR . interior . TIR' . TSD, the feature two bases wide on the left and one short on the right
    rng = np.random.default_rng(77)
    tir = K.rand(rng, 30)
    rc = np.array([{65: 84, 67: 71, 71: 67, 84: 65}[int(x)] for x in tir[::-1]], dtype=np.uint8)
    el, a = K.cat(tir, K.rand(rng, 300), rc), 207
    seq = K.cat(K.rand(rng, 200), b'GATTACA', el, b'GATTACA', K.rand(rng, 200))
    seq[a - 8], seq[a + 360 + 7] = K.other(rng, el[-1]), K.other(rng, el[0])
    row = S.element_rows([seq], [(0, a - 2, a + 359)], min_score=30)[0]
    assert row['kind'] == 'TIR' and row['el'] == (a, a + 360) and row['tsd'][:2] == (7, 'GATTACA') and row['tsd'][2] == 0
    assert row['ends'] == bytes(el[:2]).decode() + '..' + bytes(el[-2:]).decode()
    line = formats.element_lines(np.array([(0, a - 2, a + 359)], dtype=_ffi.INTERVAL), ['s'], 'R', [row])[1].split('\t')
    assert line[-1] == 'MITE' and line[5:7] == [str(a), str(a + 360)]
    none = S.element_rows([K.rand(rng, 500)], [(0, 100, 400), (0, 7, 7)])   # no terminal repeat: the feature itself, and its best frame
    assert [r['kind'] for r in none] == [None, None] and none[0]['el'] == (100, 400) and none[1]['ends'] is None and none[1]['orf'] is None


def test_cli_flags(capsys):
    from mimeo_amd import run_filter, run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    args = run_self.mainArgs(base)
    assert (args.elements, args.tsdMin, args.tsdMax, args.tsdSlack, args.tsdMismatch, args.elementMinOrf) == (None, 4, 20, 2, 0, 300)
    args = run_self.mainArgs(base + ['--elements', 'e.tsv'])   # needs none of --terminalRepeats, --paf, --families
    assert (args.elements, args.terminalRepeats, args.paf, args.families) == ('e.tsv', None, None, None)
    args = run_self.mainArgs(base + ['--elements', 'e.tsv', '--tsdMin', '2', '--tsdMax', '32', '--tsdSlack', '8', '--tsdMismatch', '2', '--elementMinOrf', '1',
                                     '--terminalRepeats', 't.tsv', '--terminalWindow', '300'])
    assert (args.tsdMin, args.tsdMax, args.tsdSlack, args.tsdMismatch, args.elementMinOrf, args.terminalWindow) == (2, 32, 8, 2, 1, 300)
    for bad, text in ((['--tsdMin', '1'], '--tsdMin must be in 2..32'), (['--tsdMin', '33', '--tsdMax', '33'], '--tsdMin must be in 2..32'),
                      (['--tsdMax', '3'], '--tsdMax must be in tsdMin..32'), (['--tsdMax', '33'], '--tsdMax must be in tsdMin..32'),
                      (['--tsdMin', '9', '--tsdMax', '8'], '--tsdMax must be in tsdMin..32'), (['--tsdSlack', '-1'], '--tsdSlack must be in 0..8'),
                      (['--tsdSlack', '9'], '--tsdSlack must be in 0..8'), (['--tsdMismatch', '3'], '--tsdMismatch must be in 0..2'),
                      (['--tsdMismatch', '-1'], '--tsdMismatch must be in 0..2'), (['--elementMinOrf', '0'], '--elementMinOrf must be at least 1'),
                      (['--elements', 'e.tsv', '--terminalWindow', '0'], '--terminalWindow must be in 1..4096'),
                      (['--elements', 'e.tsv', '--terminalMinScore', '0'], '--terminalMinScore must be at least 1'), (['--elements'], 'expected one argument')):
        with pytest.raises(SystemExit) as e:
            run_self.mainArgs(base + bad)
        assert e.value.code == 2 and text in capsys.readouterr().err
    for flag in ('--elements', '--tsdMin', '--tsdMax', '--tsdSlack', '--tsdMismatch', '--elementMinOrf'):
        for mod, b2 in ((run_interspecies, base + ['--bfasta', 'b.fa']), (run_map, base + ['--bfasta', 'b.fa']), (run_filter, ['--infile', 'x.fa'])):
            with pytest.raises(SystemExit) as e:   # self only
                mod.mainArgs(b2 + [flag, '7'])
            assert e.value.code == 2
            assert 'unrecognized arguments: %s' % flag in capsys.readouterr().err
    with pytest.raises(SystemExit):
        run_self.mainArgs(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--elements FILE' in text and '0.13 at the defaults' in text and '0.073 of 2000 random sites' in text and 'LTR_retrotransposon' in text
    assert '(61/64)^300' in text and '--tsdMin N' in text


def test_workflow_refuses_elements_of_two_genomes():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='elements needs a self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), elements='e.tsv')
    for kw, text in ((dict(terminal_window=0), 'terminal_window must be in 1..4096'), (dict(terminal_min_score=0), 'terminal_min_score must be at least 1'),
                     (dict(tsd_min=1), 'tsd_min must be in 2..32'), (dict(tsd_max=3), r'tsd_max must be in tsd_min..32'), (dict(tsd_max=33), 'tsd_max must be in'),
                     (dict(tsd_slack=9), 'tsd_slack must be in 0..8'), (dict(tsd_mismatch=3), 'tsd_mismatch must be in 0..2'),
                     (dict(element_min_orf=0), 'element_min_orf must be at least 1')):
        with pytest.raises(ValueError, match=text):
            workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', elements='e.tsv', **kw)


def test_host_sides_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'elements_check.cc')
    exe = tmp_path / 'elements_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'elements_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
