"""Consensus library, host side: the layout of mimeo_pileup_window / mimeo_pileup_column and the symbol, the representatives
(formats.family_representatives) and the FASTA records of --consensus (formats.consensus_records) worked out by hand, the
--consensus option of `mimeo self`, and the host side of mimeo_path_pileup (mimeo_amd/csrc/pileup_host.h) under the sanitizers
as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('a', 'c', 'g', 't', 'n', 'del', 'ins_runs', 'ins_bases')


def _regions(*rows):
    r = np.zeros(len(rows), dtype=_ffi.INTERVAL)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def _cols(*rows):
    c = np.zeros(len(rows), dtype=_ffi.PILEUP_COLUMN)
    for i, row in enumerate(rows):
        c[i] = row
    return c


def test_pileup_layout_binding_and_symbol():
    assert _ffi.PILEUP_WINDOW.itemsize == 12 and _ffi.PILEUP_WINDOW.names == ('tid', 'start', 'end')
    assert [_ffi.PILEUP_WINDOW.fields[n] for n in _ffi.PILEUP_WINDOW.names] == [(np.dtype('<u4'), k) for k in range(0, 12, 4)]
    assert _ffi.PILEUP_COLUMN.itemsize == 32 and _ffi.PILEUP_COLUMN.names == FIELDS
    assert [_ffi.PILEUP_COLUMN.fields[n] for n in FIELDS] == [(np.dtype('<u4'), k) for k in range(0, 32, 4)]
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    for name, names in (('mimeo_pileup_window', _ffi.PILEUP_WINDOW.names), ('mimeo_pileup_column', FIELDS)):
        m = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, re.S)
        assert m, name
        body = re.sub(r'/\*.*?\*/', '', m.group(1))
        assert tuple(re.findall(r'\b([a-z_0-9]+)\s*[,;]', body)) == names
        assert set(re.findall(r'\b(u?int\d+_t)\b', body)) == {'uint32_t'}
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_pileup' in declared and 'mimeo_path_pileup' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    # the declaration, argument by argument, against the binding: pointers as void *, the counts 64 bits
    m = re.search(r'int mimeo_path_pileup\((.*?)\);', hdr, re.S)
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['T', 'Q', 'aln', 'n', 'path_first', 'blocks', 'nblocks', 'windows', 'nwin', 'items', 'nitems',
                                                         'cols', 'call']
    want = [C.c_void_p if '*' in a else {'uint64_t': C.c_uint64}[a.split()[0]] for a in args]
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_pileup') and list(lib.mimeo_path_pileup.argtypes) == want
    assert [a for a in args if 'cols' in a or 'call' in a] == ['mimeo_pileup_column *cols', 'uint8_t *call']
    # exported by the library that was built, beside the old symbols
    for name in _ffi.SYMBOLS:
        assert hasattr(lib, name), name
    from mimeo_amd import engine
    assert callable(engine.pileup)


def test_family_representatives_by_hand():
    # the regions and families of tests/test_host_families.py: 0, 3 and 4 one family, 2 and 5 another, 1 alone
    regions = _regions((0, 100, 200), (0, 300, 450), (1, 0, 80), (1, 500, 1500), (2, 7, 9), (2, 20, 50))
    family = np.array([0, 1, 2, 0, 0, 2], dtype=np.uint32)
    # F1: region 3 has the most links.  F2: a family of one.  F3: a tie on links (1 and 1): the longer one, region 2 (80 > 30)
    assert formats.family_representatives(regions, family, np.array([2, 0, 1, 5_000_000_000, 1, 1], dtype=np.uint64)) == [(3, 3), (1, 1), (2, 2)]
    # F1: links decide before length (region 4 is 2 bases long).  F3: region 5 has more links than the longer region 2
    assert formats.family_representatives(regions, family, np.array([2, 0, 1, 2, 3, 2], dtype=np.uint64)) == [(4, 3), (1, 1), (5, 2)]
    # a tie on links and on length: the first.  Regions 0 and 4' of 100 bases each, region 3 shorter
    regions = _regions((0, 100, 200), (0, 300, 450), (1, 0, 80), (1, 500, 550), (2, 7, 107), (2, 120, 200))
    assert formats.family_representatives(regions, family, np.array([4, 0, 1, 4, 4, 1], dtype=np.uint64)) == [(0, 3), (1, 1), (2, 2)]
    # nobody linked to anybody: every region a family, in order; no region at all
    assert formats.family_representatives(regions, np.arange(6), np.zeros(6, dtype=np.uint64)) == [(i, 1) for i in range(6)]
    assert formats.family_representatives(regions[:0], [], []) == []
    # the order is that of family_lines' names: the family of the k-th record is named F<k> there
    lines = formats.family_lines(regions, ['a', 'b', 'c'], 'p', family, np.array([4, 0, 1, 4, 4, 1], dtype=np.uint64), header=False)
    reps = formats.family_representatives(regions, family, np.array([4, 0, 1, 4, 4, 1], dtype=np.uint64))
    assert [lines[i].split('\t')[4] for i, _ in reps] == ['F1', 'F2', 'F3']


def test_consensus_records_by_hand():
    regions = _regions((0, 100, 104), (1, 10, 140), (2, 5, 8))
    names = ['a', 'b', 'c']
    reps = [(1, 3), (0, 1), (2, 2)]   # F1: region 1 (130 columns), F2: region 0 (4 columns, a family of one), F3: region 2 (3 columns)
    # F1: 130 columns of depth 2, a 'G' everywhere but ten '-' (columns 20 .. 29): 120 letters, two full lines of 60
    c1 = _cols(*[(0, 0, 2, 0, 0, 0, 0, 0)] * 130)
    call1 = np.full(130, ord('G'), dtype=np.uint8)
    call1[20:30] = ord('-')
    call1[0], call1[59 + 10], call1[60 + 10], call1[129] = ord('A'), ord('C'), ord('T'), ord('N')   # letters 0, 59, 60 and 119 of the sequence
    # F2: nobody covers the family of one: depth 0, the target's own letters
    c2 = _cols(*[(0,) * 8] * 4)
    call2 = np.frombuffer(b'ACGT', dtype=np.uint8)
    # F3: the ins_sites rule at its boundary, 2 * ins_runs > depth + 1: depth 3 (a + del + n) with 2 runs is not (4 > 4), depth 2
    # with 2 runs is (4 > 3), depth 0 with 1 run is (2 > 1) — ins_bases plays no part
    c3 = _cols((1, 0, 0, 0, 1, 1, 2, 900), (0, 1, 0, 1, 0, 0, 2, 2), (0, 0, 0, 0, 0, 0, 1, 1))
    call3 = np.frombuffer(b'A-T', dtype=np.uint8)
    lines = formats.consensus_records(regions, names, 'Self_Repeat', reps, np.concatenate([c1, c2, c3]), np.concatenate([call1, call2, call3]))
    s1 = 'A' + 'G' * 58 + 'C', 'T' + 'G' * 58 + 'N'
    assert lines == ['>F1 rep=Self_Repeat_00002 b:10-140 members=3 length=120 mean_depth=2.00 ins_sites=0', s1[0], s1[1],
                     '>F2 rep=Self_Repeat_00001 a:100-104 members=1 length=4 mean_depth=0.00 ins_sites=0', 'ACGT',
                     '>F3 rep=Self_Repeat_00003 c:5-8 members=2 length=2 mean_depth=1.67 ins_sites=2', 'AT']
    assert all(len(l) <= 60 for l in lines if not l.startswith('>')) and formats.CONSENSUS_WIDTH == 60
    # ID, seqid, start and end are those of the representative's GFF3 row
    gff = [g.split('\t') for g in formats.gff_repeat_lines(regions, names, 'mimeo-self', 'Self_Repeat', 'Self_Repeat')]
    for l, (i, _) in zip([l for l in lines if l.startswith('>')], reps):
        assert l.split()[1] == 'rep=' + gff[i][8][3:] and l.split()[2] == '%s:%s-%s' % (gff[i][0], gff[i][3], gff[i][4])
    # 61 letters: a second line of one; the second block of --strictSelf carries its suffix; a run of families starts at its number
    lines = formats.consensus_records(_regions((0, 0, 61)), names, 'p', [(0, 1)], _cols(*[(1, 0, 0, 0, 0, 0, 0, 0)] * 61), np.full(61, ord('A'), dtype=np.uint8),
                                      suffix='_intra', number=7)
    assert lines == ['>F7_intra rep=p_00001 a:0-61 members=1 length=61 mean_depth=1.00 ins_sites=0', 'A' * 60, 'A']
    # every column deleted: a header and no sequence line; no family: no line
    lines = formats.consensus_records(_regions((0, 0, 2)), names, 'p', [(0, 2)], _cols((0, 0, 0, 0, 0, 3, 0, 0), (0, 0, 0, 0, 0, 3, 0, 0)),
                                      np.frombuffer(b'--', dtype=np.uint8))
    assert lines == ['>F1 rep=p_00001 a:0-2 members=2 length=0 mean_depth=3.00 ins_sites=0']
    assert formats.consensus_records(regions, names, 'p', [], _cols(), np.zeros(0, dtype=np.uint8)) == []
    # counts near 2^32 do not wrap in the depth
    big = _cols((4_000_000_000, 4_000_000_000, 0, 0, 0, 0, 4_000_000_001, 0))
    assert formats.consensus_records(_regions((0, 0, 1)), names, 'p', [(0, 1)], big, np.frombuffer(b'A', dtype=np.uint8))[0].endswith(
        'mean_depth=8000000000.00 ins_sites=1')


def test_consensus_option(capsys):
    from mimeo_amd import run_filter, run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    assert run_self.mainArgs(base).consensus is None
    args = run_self.mainArgs(base + ['--consensus', 'lib.fa'])
    assert (args.consensus, args.families, args.familyCover, args.paf) == ('lib.fa', None, 80, None)   # needs neither --families nor --paf
    args = run_self.mainArgs(base + ['--consensus', 'lib.fa', '--families', 'f.tsv', '--familyCover', '70', '--strictSelf'])
    assert (args.consensus, args.families, args.familyCover, args.strictSelf) == ('lib.fa', 'f.tsv', 70, True)
    # `mimeo x` has its query in another genome; `mimeo map` and `mimeo filter` read a library and make none
    for mod, b2 in ((run_interspecies, base + ['--bfasta', 'b.fa']), (run_map, base + ['--bfasta', 'b.fa']), (run_filter, ['--infile', 'x.fa'])):
        with pytest.raises(SystemExit) as e:
            mod.mainArgs(b2 + ['--consensus', 'lib.fa'])
        assert e.value.code == 2
        assert 'unrecognized arguments: --consensus' in capsys.readouterr().err
    for mod in (run_interspecies, run_map):
        assert not hasattr(mod.mainArgs(base + ['--bfasta', 'b.fa']), 'consensus')


def test_workflow_refuses_consensus_outside_a_self_job():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), consensus='lib.fa')
    for pct in (0, 101):   # --familyCover applies
        with pytest.raises(ValueError, match='family_cover'):
            workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', consensus='lib.fa', family_cover=pct)
    assert workflow.CONSENSUS_BUDGET == 1 << 22


def test_pileup_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'pileup_check.cc')
    exe = tmp_path / 'pileup_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'pileup_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
