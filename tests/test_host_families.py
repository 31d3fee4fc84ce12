"""Repeat families, host side: the lines of --families (formats.family_lines) worked out by hand, the ctypes binding of
mimeo_link_regions and the symbol, the --families / --familyCover options of `mimeo self`, and the host side of the entry point
(mimeo_amd/csrc/link_regions_host.h) under the sanitizers as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _regions(*rows):
    r = np.zeros(len(rows), dtype=_ffi.INTERVAL)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def test_family_lines_by_hand():
    # six regions on three scaffolds; the union-find's labels are the smallest member: regions 0, 3 and 4 are one family,
    # 2 and 5 another, region 1 is linked to nobody
    regions = _regions((0, 100, 200), (0, 300, 450), (1, 0, 80), (1, 500, 1500), (2, 7, 9), (2, 20, 50))
    names = ['a', 'b', 'c']
    family = np.array([0, 1, 2, 0, 0, 2], dtype=np.uint32)
    links = np.array([2, 0, 1, 5_000_000_000, 1, 1], dtype=np.uint64)
    lines = formats.family_lines(regions, names, 'Self_Repeat', family, links)
    assert lines[0] == formats.FAMILY_HEADER == '#ID\tseqid\tstart\tend\tfamily\tmembers\tfamily_bases\tlinks'
    assert lines[1:] == ['Self_Repeat_00001\ta\t100\t200\tF1\t3\t1102\t2',        # 100 + 1000 + 2 bases
                         'Self_Repeat_00002\ta\t300\t450\tF2\t1\t150\t0',         # a singleton is a family of one, named in its turn
                         'Self_Repeat_00003\tb\t0\t80\tF3\t2\t110\t1',
                         'Self_Repeat_00004\tb\t500\t1500\tF1\t3\t1102\t5000000000',   # a count beyond 2^32 prints as it is
                         'Self_Repeat_00005\tc\t7\t9\tF1\t3\t1102\t1',
                         'Self_Repeat_00006\tc\t20\t50\tF3\t2\t110\t1']
    # ID, seqid, start and end are those of the GFF3 row, as in region_stat_lines
    for l, g in zip(lines[1:], formats.gff_repeat_lines(regions, names, 'mimeo-self', 'Self_Repeat', 'Self_Repeat')):
        gf = g.split('\t')
        assert l.split('\t')[:4] == [gf[8][3:], gf[0], gf[3], gf[4]]
    stat = formats.region_stat_lines(regions, names, 'Self_Repeat', np.zeros(6, dtype=_ffi.WINDOW_STATS), [0] * 6)
    assert [l.split('\t')[:4] for l in lines] == [l.split('\t')[:4] for l in stat]
    # the second block of --strictSelf: no header, restarted IDs, names with the suffix, numbered on their own
    intra = formats.family_lines(regions[2:], names, 'p', np.array([0, 1, 1, 0]), np.array([1, 1, 1, 1]), suffix='_intra', header=False)
    assert intra == ['p_00001\tb\t0\t80\tF1_intra\t2\t110\t1', 'p_00002\tb\t500\t1500\tF2_intra\t2\t1002\t1',
                     'p_00003\tc\t7\t9\tF2_intra\t2\t1002\t1', 'p_00004\tc\t20\t50\tF1_intra\t2\t110\t1']
    assert formats.family_lines(regions[:0], names, 'p', [], []) == [formats.FAMILY_HEADER]
    assert formats.family_lines(regions[:0], names, 'p', [], [], header=False) == []


def test_link_regions_binding_and_symbol():
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_link_regions' in declared and 'mimeo_link_regions' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    # the declaration, argument by argument, against the binding: pointers as void *, the counts 64 bits, the per cent 32
    m = re.search(r'int mimeo_link_regions\((.*?)\);', hdr, re.S)
    args = [a.strip() for a in re.sub(r'/\*.*?\*/', '', m.group(1)).split(',')]
    assert [a.split()[-1].lstrip('*') for a in args] == ['T', 'aln', 'n', 'path_first', 'blocks', 'nblocks', 'regions', 'nreg', 'chrom_of_scaf', 'items',
                                                         'nitems', 'min_cover_pct', 'family', 'links']
    import ctypes as C
    want = [C.c_void_p if '*' in a else {'uint64_t': C.c_uint64, 'uint32_t': C.c_uint32}[a.split()[0]] for a in args]
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_link_regions') and list(lib.mimeo_link_regions.argtypes) == want
    assert [a for a in args if 'family' in a or 'links' in a] == ['uint32_t *family', 'uint64_t *links']
    # the structs that cross the call: 12-byte intervals, 16-byte items
    assert _ffi.INTERVAL.itemsize == 12 and _ffi.INTERVAL.names == ('chrom', 'start', 'end')
    assert _ffi.WINDOW_ITEM.itemsize == 16 and _ffi.WINDOW_ITEM.names == ('aln', 'group', 'w0', 'w1')
    from mimeo_amd import engine
    assert callable(engine.link_regions)


def test_families_options(capsys):
    from mimeo_amd import run_interspecies, run_map, run_self
    base = ['--afasta', 'a.fa']
    args = run_self.mainArgs(base)
    assert args.families is None and args.familyCover == 80
    args = run_self.mainArgs(base + ['--families', 'f.tsv'])
    assert (args.families, args.familyCover, args.regionStats, args.paf) == ('f.tsv', 80, None, None)   # needs neither --paf nor --regionStats
    for pct in (1, 100, 50):
        assert run_self.mainArgs(base + ['--families', 'f.tsv', '--familyCover', str(pct)]).familyCover == pct
    args = run_self.mainArgs(base + ['--families', 'f.tsv', '--regionStats', 'r.tsv', '--strictSelf'])
    assert (args.families, args.regionStats, args.strictSelf) == ('f.tsv', 'r.tsv', True)
    for pct in ('0', '101', '-5'):
        with pytest.raises(SystemExit) as e:
            run_self.mainArgs(base + ['--families', 'f.tsv', '--familyCover', pct])
        assert e.value.code == 2
        assert '--familyCover must be in 1..100' in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:   # out of range is an error with or without --families
        run_self.mainArgs(base + ['--familyCover', '0'])
    assert e.value.code == 2
    capsys.readouterr()
    # `mimeo x` has its query in another genome, `mimeo map` has no regions
    for mod in (run_interspecies, run_map):
        b2 = base + ['--bfasta', 'b.fa']
        assert not hasattr(mod.mainArgs(b2), 'families') and not hasattr(mod.mainArgs(b2), 'familyCover')
        with pytest.raises(SystemExit) as e:
            mod.mainArgs(b2 + ['--families', 'f.tsv'])
        assert e.value.code == 2
        assert 'unrecognized arguments: --families' in capsys.readouterr().err


def test_workflow_refuses_families_outside_a_self_job():
    from mimeo_amd import workflow
    with pytest.raises(ValueError, match='self job'):
        workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', B=object(), families='f.tsv')
    for pct in (0, 101):
        with pytest.raises(ValueError, match='family_cover'):
            workflow.self_repeats(object(), [], 'x.tab', 'x.gff3', families='f.tsv', family_cover=pct)


def test_link_regions_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'link_regions_check.cc')
    exe = tmp_path / 'link_regions_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'link_regions_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
