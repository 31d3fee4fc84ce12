"""Inserted columns of the consensus library, host side: the layout of mimeo_insert_site / mimeo_insert_result /
mimeo_insert_column and the symbol, the sites (formats.insertion_sites) and the FASTA records with insertions
(formats.consensus_records) worked out by hand, the --consensusInsertions option of `mimeo self`, and the host side of
mimeo_path_insertions (mimeo_amd/csrc/insert_host.h) under the sanitizers as a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = (('mimeo_insert_site', 'INSERT_SITE', ('window', 'x', 'ncols', 'voters')), ('mimeo_insert_result', 'INSERT_RESULT', ('runs', 'bases', 'longer', 'max_len')),
           ('mimeo_insert_column', 'INSERT_COLUMN', ('a', 'c', 'g', 't', 'n')))


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


def _sites(*rows):
    s = np.zeros(len(rows), dtype=_ffi.INSERT_SITE)
    for i, row in enumerate(rows):
        s[i] = row
    return s


def test_insertion_layouts_binding_and_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    for cname, pyname, names in LAYOUTS:
        dt = getattr(_ffi, pyname)
        assert dt.itemsize == 4 * len(names) and dt.names == names
        assert [dt.fields[n] for n in names] == [(np.dtype('<u4'), k) for k in range(0, 4 * len(names), 4)]
        m = re.search(r'typedef struct %s \{(.*?)\} %s;\s*/\* (\d+) bytes \*/' % (cname, cname), hdr, re.S)
        assert m, cname
        body = re.sub(r'/\*.*?\*/', '', m.group(1))
        assert tuple(re.findall(r'\b([a-z_0-9]+)\s*[,;]', body)) == names
        assert set(re.findall(r'\b(u?int\d+_t)\b', body)) == {'uint32_t'} and int(m.group(2)) == dt.itemsize
    assert formats.INSERT_SITE == _ffi.INSERT_SITE and formats.INSERT_MAX_COLS == _ffi.INSERT_MAX_COLS == 1024
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_insertions' in declared and 'mimeo_path_insertions' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    # the declaration, argument by argument, against the binding: pointers as void *, the counts 64 bits
    m = re.search(r'int mimeo_path_insertions\((.*?)\);', hdr, re.S)
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['T', 'Q', 'aln', 'n', 'path_first', 'blocks', 'nblocks', 'windows', 'nwin', 'items', 'nitems',
                                                         'sites', 'nsites', 'res', 'icols', 'icall']
    # up to nitems the arguments are those of mimeo_path_pileup, word for word
    p = re.search(r'int mimeo_path_pileup\((.*?)\);', hdr, re.S)
    assert args[:11] == [a.strip() for a in re.sub(r'/\*.*?\*/', '', p.group(1)).split(',')][:11]
    want = [C.c_void_p if '*' in a else {'uint64_t': C.c_uint64}[a.split()[0]] for a in args]
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_insertions') and list(lib.mimeo_path_insertions.argtypes) == want
    assert args[11:] == ['const mimeo_insert_site *sites', 'uint64_t nsites', 'mimeo_insert_result *res', 'mimeo_insert_column *icols', 'uint8_t *icall']
    for name in _ffi.SYMBOLS:   # exported by the library that was built, beside the old symbols
        assert hasattr(lib, name), name
    from mimeo_amd import engine
    assert callable(engine.insertions)


def test_insertion_sites_by_hand():
    win = np.zeros(4, dtype=_ffi.PILEUP_WINDOW)
    win[0], win[1], win[2], win[3] = (0, 100, 104), (1, 7, 7), (1, 50, 53), (0, 100, 101)   # an empty window, and one base twice
    cols = _cols(
        # window 0, the rule at its boundary, 2 * ins_runs > depth + 1: depth 3 (a + n + del) with 2 runs is no site (4 > 4) ...
        (1, 0, 0, 0, 1, 1, 2, 900),
        # ... depth 2 with 2 runs is one (4 > 3): ncols = ins_bases - ins_runs + 1 = 9 - 2 + 1, voters = depth + 1
        (0, 1, 0, 1, 0, 0, 2, 9),
        (0, 0, 5, 0, 0, 0, 0, 0),
        # depth 0 with 1 run is one (2 > 1): a run of one base has one column, and only the own copy votes against it
        (0, 0, 0, 0, 0, 0, 1, 1),
        # window 2: ncols is capped at 1024 (5000 - 3 + 1 columns asked); one column short of the cap; exactly the cap
        (0, 0, 0, 2, 0, 1, 3, 5000), (0, 0, 0, 2, 0, 1, 3, 1025), (0, 0, 0, 2, 0, 1, 3, 1026),
        # window 3: counts near 2^32 do not wrap
        (4_000_000_000, 0, 0, 0, 0, 0, 4_000_000_000, 4_000_000_001))
    sites = formats.insertion_sites(win, cols)
    assert sites.dtype == _ffi.INSERT_SITE
    assert sites.tolist() == [(0, 101, 8, 3), (0, 103, 1, 1), (2, 50, 1024, 4), (2, 51, 1023, 4), (2, 52, 1024, 4), (3, 100, 2, 4_000_000_001)]
    # the expression is the one behind ins_sites=: the header of the same columns counts the same sites
    regions = _regions((0, 100, 104), (1, 50, 53))
    lines = formats.consensus_records(regions, ['a', 'b'], 'p', [(0, 1), (1, 1)], np.concatenate([cols[:4], cols[4:7]]), np.frombuffer(b'ACGTTTT', dtype=np.uint8))
    assert [l.split()[-1] for l in lines if l.startswith('>')] == ['ins_sites=2', 'ins_sites=3']
    # nothing: no window, no site
    none = formats.insertion_sites(win[:0], cols[:0])
    assert none.size == 0 and none.dtype == _ffi.INSERT_SITE
    assert formats.insertion_sites(win[:1], _cols(*[(3, 0, 0, 0, 0, 0, 2, 2)] * 4)).size == 0


def test_consensus_records_with_insertions_by_hand():
    regions = _regions((0, 100, 104), (1, 10, 14), (2, 5, 8))
    names = ['a', 'b', 'c']
    reps = [(1, 3), (0, 1), (2, 2)]   # F1: region 1 (columns 10 .. 13), F2: region 0 (100 .. 103), F3: region 2 (5 .. 7)
    c1 = _cols((0, 0, 2, 0, 0, 0, 2, 5), (0, 0, 2, 0, 0, 0, 0, 0), (0, 0, 0, 0, 0, 2, 2, 2), (0, 0, 2, 0, 0, 0, 0, 0))
    c2 = _cols(*[(0,) * 8] * 4)
    c3 = _cols((0, 2, 0, 0, 0, 0, 0, 0), (0, 2, 0, 0, 0, 0, 2, 4), (0, 2, 0, 0, 0, 0, 0, 0))
    cols = np.concatenate([c1, c2, c3])
    call = np.frombuffer(b'GG-G' + b'ACGT' + b'CCC', dtype=np.uint8)
    plain = ['>F1 rep=p_00002 b:10-14 members=3 length=3 mean_depth=2.00 ins_sites=2', 'GGG',
             '>F2 rep=p_00001 a:100-104 members=1 length=4 mean_depth=0.00 ins_sites=0', 'ACGT',
             '>F3 rep=p_00003 c:5-8 members=2 length=3 mean_depth=2.00 ins_sites=1', 'CCC']
    assert formats.consensus_records(regions, names, 'p', reps, cols, call) == plain                     # what it is today ...
    assert formats.consensus_records(regions, names, 'p', reps, cols, call, insertions=None) == plain    # ... also said aloud
    # F1: a site in front of the window's first column (4 columns: 'TA-' and a trailing '-': two letters), and a site in front of a
    # column whose own call is '-' (column 12: 'N' goes in, the column itself stays out).  F2: no site.  F3: a site whose icall is
    # all '-': nothing goes in, inserted=0
    win = np.zeros(3, dtype=_ffi.PILEUP_WINDOW)
    win[0], win[1], win[2] = (1, 10, 14), (0, 100, 104), (2, 5, 8)
    sites = formats.insertion_sites(win, cols)
    assert sites.tolist() == [(0, 10, 4, 3), (0, 12, 1, 3), (2, 6, 3, 3)]
    icall = np.frombuffer(b'TA--' + b'N' + b'---', dtype=np.uint8)
    lines = formats.consensus_records(regions, names, 'p', reps, cols, call, insertions=(sites, icall))
    assert lines == ['>F1 rep=p_00002 b:10-14 members=3 length=6 mean_depth=2.00 ins_sites=2 inserted=3', 'TAGGNG',
                     '>F2 rep=p_00001 a:100-104 members=1 length=4 mean_depth=0.00 ins_sites=0 inserted=0', 'ACGT',
                     '>F3 rep=p_00003 c:5-8 members=2 length=3 mean_depth=2.00 ins_sites=1 inserted=0', 'CCC']
    # length grows by exactly `inserted`, and everything in front of ins_sites= is the line without the flag
    for a, b in zip(plain[::2], lines[::2]):
        fa, fb = (dict(x.split('=') for x in l.split()[1:] if '=' in x) for l in (a, b))
        assert int(fb['length']) == int(fa['length']) + int(fb['inserted'])
        assert re.sub(r'length=\d+', '', b).startswith(re.sub(r'length=\d+', '', a))
    # a gap inside the inserted bytes is left out where it stands; a site in front of the last column; a run of families whose
    # number does not start at 1; lines of CONSENSUS_WIDTH letters
    sites = _sites((0, 3, 60, 2))
    icall = np.frombuffer(b'A-' * 30, dtype=np.uint8)
    lines = formats.consensus_records(_regions((0, 0, 4)), names, 'p', [(0, 2)], _cols(*[(1, 0, 0, 0, 0, 0, 0, 0)] * 4), np.frombuffer(b'CCCG', dtype=np.uint8),
                                      suffix='_intra', number=7, insertions=(sites, icall))
    assert lines == ['>F7_intra rep=p_00001 a:0-4 members=2 length=34 mean_depth=1.00 ins_sites=0 inserted=30', 'CCC' + 'A' * 30 + 'G']
    # the flag given and no site anywhere: every header says inserted=0
    lines = formats.consensus_records(regions, names, 'p', reps, cols, call, insertions=(_sites(), np.zeros(0, dtype=np.uint8)))
    assert lines == [l + ' inserted=0' if l.startswith('>') else l for l in plain]


def test_consensus_insertions_option(capsys):
    from mimeo_amd import run_filter, run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    assert run_self.mainArgs(base).consensusInsertions is False
    assert run_self.mainArgs(base + ['--consensus', 'lib.fa']).consensusInsertions is False
    args = run_self.mainArgs(base + ['--consensus', 'lib.fa', '--consensusInsertions'])
    assert (args.consensus, args.consensusInsertions, args.families) == ('lib.fa', True, None)
    args = run_self.mainArgs(base + ['--consensusInsertions', '--consensus', 'lib.fa', '--strictSelf'])
    assert (args.consensus, args.consensusInsertions, args.strictSelf) == ('lib.fa', True, True)
    # without --consensus there is no library to insert into: a parser error, before the engine starts
    with pytest.raises(SystemExit) as e:
        run_self.mainArgs(base + ['--consensusInsertions'])
    assert e.value.code == 2 and '--consensusInsertions needs --consensus' in capsys.readouterr().err
    for mod, b2 in ((run_interspecies, base + ['--bfasta', 'b.fa']), (run_map, base + ['--bfasta', 'b.fa']), (run_filter, ['--infile', 'x.fa'])):
        with pytest.raises(SystemExit) as e:
            mod.mainArgs(b2 + ['--consensusInsertions'])
        assert e.value.code == 2
        assert 'unrecognized arguments: --consensusInsertions' in capsys.readouterr().err
    for mod in (run_interspecies, run_map):
        assert not hasattr(mod.mainArgs(base + ['--bfasta', 'b.fa']), 'consensusInsertions')


def test_workflow_refuses_insertions_without_a_library():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='consensus_insertions needs consensus'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', consensus_insertions=True)


def test_insert_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'insert_check.cc')
    exe = tmp_path / 'insert_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'insert_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
