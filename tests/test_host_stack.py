"""Family seed alignments, host side: the layout of mimeo_stack_row and the declaration of mimeo_path_stack against the binding,
the Stockholm blocks (formats.stockholm_blocks, formats.stockholm_row_name, formats.stack_sites) worked out by hand, the
--familyAlignments option of `mimeo self`, and the host side of mimeo_path_stack (mimeo_amd/csrc/stack_host.h) under the
sanitizers as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rows(dtype, *rows):
    r = np.zeros(len(rows), dtype=dtype)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def test_stack_layout_binding_and_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    names = ('q_lo', 'q_hi', 'bases', 'hidden')
    dt = _ffi.STACK_ROW
    assert dt.itemsize == 16 and dt.names == names
    assert [dt.fields[n] for n in names] == [(np.dtype('<u4'), k) for k in range(0, 16, 4)]
    m = re.search(r'typedef struct mimeo_stack_row \{(.*?)\} mimeo_stack_row;\s*/\* (\d+) bytes \*/', hdr, re.S)
    assert m
    body = re.sub(r'/\*.*?\*/', '', m.group(1))
    assert tuple(re.findall(r'\b([a-z_0-9]+)\s*[,;]', body)) == names
    assert set(re.findall(r'\b(u?int\d+_t)\b', body)) == {'uint32_t'} and int(m.group(2)) == dt.itemsize
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_stack' in declared and 'mimeo_path_stack' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    # the declaration, argument by argument, against the binding: pointers as void *, the counts 64 bits
    m = re.search(r'int mimeo_path_stack\((.*?)\);', hdr, re.S)
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['T', 'Q', 'aln', 'n', 'path_first', 'blocks', 'nblocks', 'windows', 'nwin', 'items', 'nitems',
                                                         'sites', 'nsites', 'res', 'row_first', 'rows']
    # up to nsites the arguments are those of mimeo_path_insertions, word for word
    p = re.search(r'int mimeo_path_insertions\((.*?)\);', hdr, re.S)
    assert args[:13] == [a.strip() for a in re.sub(r'/\*.*?\*/', '', p.group(1)).split(',')][:13]
    assert args[13:] == ['mimeo_stack_row *res', 'uint64_t **row_first', 'uint8_t **rows']
    want = [C.POINTER(C.c_void_p) if '**' in a else C.c_void_p if '*' in a else {'uint64_t': C.c_uint64}[a.split()[0]] for a in args]
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_stack') and list(lib.mimeo_path_stack.argtypes) == want
    for name in _ffi.SYMBOLS:   # exported by the library that was built, beside the old symbols
        assert hasattr(lib, name), name
    from mimeo_amd import engine
    assert callable(engine.stack)


def test_stack_sites_by_hand():
    win = _rows(_ffi.PILEUP_WINDOW, (0, 100, 104), (1, 7, 7), (1, 50, 52))   # an empty window in between
    cols = _rows(_ffi.PILEUP_COLUMN,
                 (5, 0, 0, 0, 0, 0, 1, 9),      # one row of six inserts: no majority site, but a site of the stack
                 (0, 0, 0, 0, 0, 0, 0, 0),
                 (0, 1, 0, 1, 0, 1, 3, 30),
                 (2, 0, 0, 0, 0, 0, 0, 0),
                 (0, 0, 0, 2, 0, 1, 3, 5000), (0, 0, 0, 2, 0, 0, 0, 0))
    first = formats.stack_sites(win, cols)
    assert first.dtype == _ffi.INSERT_SITE and first.tolist() == [(0, 100, 1, 6), (0, 102, 1, 4), (2, 50, 1, 4)]
    assert formats.insertion_sites(win, cols).tolist() == [(0, 102, 28, 4), (2, 50, 1024, 4)]   # the majority rule picks fewer
    # ncols from the longest run of every site, capped at 1024
    sites = formats.stack_sites(win, cols, max_len=[9, 12, 4999])
    assert sites.tolist() == [(0, 100, 9, 6), (0, 102, 12, 4), (2, 50, 1024, 4)]
    none = formats.stack_sites(win[:0], cols[:0])
    assert none.size == 0 and none.dtype == _ffi.INSERT_SITE
    assert formats.stack_sites(win[:1], cols[:4][[1, 3, 1, 3]]).size == 0


def test_stockholm_row_names():
    assert formats.stockholm_row_name('chr1', 1000, 0, 0, 10) == 'chr1/1-10'
    assert formats.stockholm_row_name('chr1', 1000, 0, 99, 100) == 'chr1/100-100'
    # the aligned strand is the reverse complement: its bases [0, 10) are the plus strand's last ten, read backwards: s > e
    assert formats.stockholm_row_name('chr1', 1000, 1, 0, 10) == 'chr1/1000-991'
    assert formats.stockholm_row_name('chr1', 1000, 1, 990, 1000) == 'chr1/10-1'
    assert formats.stockholm_row_name('a/b', 50, 1, 7, 8) == 'a/b/43-43'


def test_stockholm_blocks_by_hand():
    """two families: F1 = region 1 (b:10-14) with a site of two columns in front of its first base and one of one column in front
    of its third; F2 = region 0 (a:100-103) without a site and without a row"""
    regions = _rows(_ffi.INTERVAL, (0, 100, 103), (1, 10, 14))
    names = ['a', 'b']
    reps = [(1, 3), (0, 1)]
    sites = _rows(_ffi.INSERT_SITE, (0, 10, 2, 3), (0, 12, 1, 3))
    own = np.frombuffer(b'GGCG' + b'ACN', dtype=np.uint8)
    call = np.frombuffer(b'GG-G' + b'ACN', dtype=np.uint8)
    icall = np.frombuffer(b'T-' + b'-', dtype=np.uint8)
    rows = [(0, 'b/31-36', b'ta' + b'GG' + b'.' + b'-G'), (0, 'a/9-5', b'tcGGnCG'), (0, 'b/31-36', b'..' + b'.G' + b'.' + b'CG'), (0, 'b/31-36', np.frombuffer(b't.GG.CG', dtype=np.uint8))]
    lines = formats.stockholm_blocks(regions, names, 'p', reps, sites, own, call, icall, rows)
    assert lines == ['# STOCKHOLM 1.0', '#=GF ID F1', '#=GF DE rep=p_00002 b:10-14 members=3 rows=5 columns=7',
                     'b/11-14 ..GG.CG',
                     'b/31-36 taGG.-G',
                     'a/9-5 tcGGnCG',
                     'b/31-36.2 ...G.CG',
                     'b/31-36.3 t.GG.CG',
                     '#=GC RF ..xx.xx',
                     '#=GC cons T.GG.-G',
                     '//',
                     '# STOCKHOLM 1.0', '#=GF ID F2', '#=GF DE rep=p_00001 a:100-103 members=1 rows=1 columns=3',
                     'a/101-103 ACN', '#=GC RF xxx', '#=GC cons ACN', '//']
    # cons without '.' and '-' is the record of consensus_records with these bytes
    cols = _rows(_ffi.PILEUP_COLUMN, *[(0,) * 8] * 7)
    fasta = formats.consensus_records(regions, names, 'p', reps, cols, call, insertions=(sites, icall))
    cons = [l[10:].replace('.', '').replace('-', '') for l in lines if l.startswith('#=GC cons ')]
    assert cons == ['TGGG', 'ACN'] == fasta[1::2]
    # the second block of --strictSelf, a run of families that does not start at 1, and a row whose name is the representative's own
    lines = formats.stockholm_blocks(regions, names, 'p', reps[1:], sites[:0], own[4:], call[4:], icall[:0], [(0, 'a/101-103', b'AC-')], suffix='_intra', number=7)
    assert lines == ['# STOCKHOLM 1.0', '#=GF ID F7_intra', '#=GF DE rep=p_00001 a:100-103 members=1 rows=2 columns=3', 'a/101-103 ACN', 'a/101-103.2 AC-',
                     '#=GC RF xxx', '#=GC cons ACN', '//']
    # a row of the wrong width is a bug of the caller's, not a line of the file
    with pytest.raises(ValueError, match='row b/1-2 has 2 bytes for a block of 7 columns'):
        formats.stockholm_blocks(regions, names, 'p', reps, sites, own, call, icall, [(0, 'b/1-2', b'GG')])
    assert formats.stockholm_blocks(regions, names, 'p', [], sites[:0], own[:0], call[:0], icall[:0], []) == []


def test_family_alignments_option(capsys):
    from mimeo_amd import run_filter, run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    assert run_self.mainArgs(base).familyAlignments is None
    args = run_self.mainArgs(base + ['--familyAlignments', 'fam.sto'])   # needs neither --families nor --consensus
    assert (args.familyAlignments, args.families, args.consensus, args.familyCover) == ('fam.sto', None, None, 80)
    args = run_self.mainArgs(base + ['--familyAlignments', 'fam.sto', '--familyCover', '60', '--strictSelf', '--consensus', 'lib.fa', '--consensusInsertions'])
    assert (args.familyAlignments, args.familyCover, args.strictSelf, args.consensus) == ('fam.sto', 60, True, 'lib.fa')
    with pytest.raises(SystemExit) as e:   # --familyCover applies
        run_self.mainArgs(base + ['--familyAlignments', 'fam.sto', '--familyCover', '0'])
    assert e.value.code == 2 and '--familyCover must be in 1..100' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:
        run_self.mainArgs(base + ['--familyAlignments'])
    assert e.value.code == 2
    capsys.readouterr()
    for mod, b2 in ((run_interspecies, base + ['--bfasta', 'b.fa']), (run_map, base + ['--bfasta', 'b.fa']), (run_filter, ['--infile', 'x.fa'])):
        with pytest.raises(SystemExit) as e:   # self only
            mod.mainArgs(b2 + ['--familyAlignments', 'fam.sto'])
        assert e.value.code == 2
        assert 'unrecognized arguments: --familyAlignments' in capsys.readouterr().err


def test_workflow_refuses_family_alignments_of_two_genomes():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='family_alignments needs a self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), family_alignments='x.sto')
    with pytest.raises(ValueError, match='family_cover must be in 1..100'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', family_alignments='x.sto', family_cover=101)


def test_stack_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'stack_check.cc')
    exe = tmp_path / 'stack_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'stack_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
