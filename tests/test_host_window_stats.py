"""Per-region divergence, host side: the join of alignments and regions (formats.region_items) and the lines of --regionStats
(formats.region_stat_lines) worked out by hand, the layout of mimeo_window_item / mimeo_window_stats and the symbol, the
--regionStats option of the command line, and the host side of mimeo_path_window_stats
(mimeo_amd/csrc/window_stats_host.h) under the sanitizers as a stand-alone program."""
import os
import re
import subprocess

import numpy as np
import pytest

from mimeo_amd import _ffi, formats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_runs', 'ins_bases', 'del_runs', 'del_bases')


def _recs(*rows):
    """(tid, qid, tstart, tend, qstrand) per record"""
    r = np.zeros(len(rows), dtype=_ffi.ALIGNMENT)
    for i, (tid, qid, ts, te, strand) in enumerate(rows):
        r[i]['tid'], r[i]['qid'], r[i]['tstart'], r[i]['tend'], r[i]['qstrand'] = tid, qid, ts, te, strand
    return r


def _regions(*rows):
    r = np.zeros(len(rows), dtype=_ffi.INTERVAL)
    for i, row in enumerate(rows):
        r[i] = row
    return r


def _items(items):
    return [tuple(int(x) for x in it) for it in items]


# regions as the collapse returns them: sorted by (chrom, start), disjoint; chrom = rank of the scaffold's name
REGIONS = _regions((0, 100, 200), (0, 300, 400), (0, 400, 450), (0, 1000, 1100), (1, 50, 150), (2, 0, 80))


def test_region_items_by_hand():
    ident = [0, 1, 2]
    recs = _recs((0, 1, 120, 180, 0),    # 0: inside one region
                 (0, 1, 50, 250, 1),     # 1: overhanging both ends of it
                 (0, 2, 150, 420, 0),    # 2: spanning three regions, two of which abut
                 (0, 1, 199, 260, 0),    # 3: touching region 0 by its last base
                 (0, 1, 250, 301, 0),    # 4: touching region 1 by its first base
                 (0, 1, 200, 300, 0),    # 5: abutting regions 0 and 1 on either side: in neither
                 (0, 1, 450, 1000, 0),   # 6: abutting regions 2 and 3
                 (1, 0, 120, 180, 0),    # 7: the coordinates of record 0 on another scaffold: region 4, not region 0
                 (2, 0, 500, 600, 0),    # 8: on a scaffold whose only region lies elsewhere
                 (0, 1, 0, 5000, 0),     # 9: over every region of the scaffold
                 (1, 1, 70, 70, 0))      # 10: a record without a base
    items, rows = formats.region_items(recs, REGIONS, ident)
    assert items.dtype == _ffi.WINDOW_ITEM == formats.WINDOW_ITEM
    assert _items(items) == [(0, 0, 120, 180), (1, 0, 100, 200), (2, 0, 150, 200), (2, 1, 300, 400), (2, 2, 400, 420), (3, 0, 199, 200),
                             (4, 1, 300, 301), (7, 4, 120, 150), (9, 0, 100, 200), (9, 1, 300, 400), (9, 2, 400, 450), (9, 3, 1000, 1100)]
    assert rows.tolist() == [5, 3, 2, 1, 1, 0]
    # every window lies inside its region and inside its record, and is not empty
    for a, g, w0, w1 in _items(items):
        assert max(int(REGIONS[g]['start']), int(recs[a]['tstart'])) == w0 < w1 == min(int(REGIONS[g]['end']), int(recs[a]['tend']))
    # the alignment's true tstart, not the origin-one start1 of the BED projection: a record that starts on a region's last base
    # + 1 in origin-one terms (tstart 199 -> start1 200) is still in the region, one that starts at 200 is not
    assert _items(formats.region_items(_recs((0, 1, 200, 260, 0)), REGIONS, ident)[0]) == []


def test_region_items_chrom_of_tid_and_empty_inputs():
    # FASTA order 'zeta', 'alpha', 'mid': the collapse numbers the scaffolds alpha 0, mid 1, zeta 2
    chrom_of_tid = [2, 0, 1]
    recs = _recs((0, 0, 10, 60, 0), (1, 0, 120, 180, 0), (2, 0, 120, 180, 0))
    items, rows = formats.region_items(recs, REGIONS, chrom_of_tid)
    assert _items(items) == [(0, 5, 10, 60), (1, 0, 120, 180), (2, 4, 120, 150)]
    assert rows.tolist() == [1, 0, 0, 0, 1, 1]
    # no records, no regions
    items, rows = formats.region_items(recs[:0], REGIONS, chrom_of_tid)
    assert items.size == 0 and items.dtype == _ffi.WINDOW_ITEM and rows.tolist() == [0] * 6
    items, rows = formats.region_items(recs, REGIONS[:0], chrom_of_tid)
    assert items.size == 0 and rows.size == 0
    items, rows = formats.region_items(recs[:1], REGIONS[:5], chrom_of_tid)   # records, regions, and no overlap
    assert items.size == 0 and rows.tolist() == [0] * 5


def test_region_items_trivial_self_rows():
    recs = _recs((0, 0, 100, 200, 0),    # 0: the scaffold against itself: one block, t == q
                 (0, 0, 100, 200, 0),    # 1: same scaffold, one block off the diagonal
                 (0, 0, 100, 200, 1),    # 2: same scaffold, t == q in numbers, but the minus strand
                 (0, 0, 100, 200, 0),    # 3: same scaffold, starts on the diagonal, two blocks
                 (0, 1, 100, 200, 0),    # 4: one block with t == q on another scaffold
                 (1, 1, 60, 120, 0))     # 5: the other scaffold against itself
    blocks = np.array([(100, 100, 100), (100, 700, 100), (100, 100, 100), (100, 100, 40), (150, 140, 50), (100, 100, 100), (60, 60, 60)],
                      dtype=_ffi.PATH_BLOCK)
    first = np.array([0, 1, 2, 3, 5, 6, 7], dtype=np.uint64)
    items, rows = formats.region_items(recs, REGIONS, [0, 1, 2], first=first, blocks=blocks, self_job=True)
    assert _items(items) == [(1, 0, 100, 200), (2, 0, 100, 200), (3, 0, 100, 200), (4, 0, 100, 200)]
    assert rows.tolist() == [4, 0, 0, 0, 0, 0]
    # a two-genome job keeps them: scaffold 0 of A against scaffold 0 of B is an alignment like any other
    items, rows = formats.region_items(recs, REGIONS, [0, 1, 2], first=first, blocks=blocks, self_job=False)
    assert [it[0] for it in _items(items)] == [0, 1, 2, 3, 4, 5] and rows.tolist() == [5, 0, 0, 0, 1, 0]
    assert _items(formats.region_items(recs, REGIONS, [0, 1, 2])[0]) == _items(items)


def _wstats(*rows):
    s = np.zeros(len(rows), dtype=_ffi.WINDOW_STATS)
    for i, r in enumerate(rows):
        for k, v in zip(FIELDS, r):
            s[k][i] = v
    return s


def test_region_stat_lines_by_hand():
    regions = _regions((1, 100, 200), (0, 5, 50), (0, 60, 90), (2, 7, 9))
    names = ['a', 'b', 'c']
    # the numbers of tests/test_host_divergence.py::test_divergence_tags_by_hand: columns = 85 + 10 + 5 + 0 = 100, covered = 100 + 4,
    # identity = 85 / 100, de = (15 + 3 runs) / (85 + 15 + 3) = 0.1748, kd = -0.5 ln(0.75 sqrt(0.9)) = 0.1702
    stats = _wstats((85, 10, 5, 0, 1, 3, 2, 4), (0, 0, 0, 0, 0, 0, 0, 0), (50, 0, 50, 0, 0, 0, 0, 0), (5_000_000_000, 0, 0, 0, 0, 0, 0, 0))
    lines = formats.region_stat_lines(regions, names, 'Self_Repeat', stats, [3, 0, 2, 1])
    assert lines[0] == formats.REGION_STATS_HEADER == ('#ID\tseqid\tstart\tend\trows\tcovered\tcolumns\tmatches\ttransitions\ttransversions\tambiguous\t'
                                                       'ins_runs\tins_bases\tdel_runs\tdel_bases\tidentity\tde\tkd')
    assert lines[1] == 'Self_Repeat_00001\tb\t100\t200\t3\t104\t100\t85\t10\t5\t0\t1\t3\t2\t4\t0.8500\t0.1748\t0.1702'
    # no row: every derived quantity is undefined
    assert lines[2] == 'Self_Repeat_00002\ta\t5\t50\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t0\t.\t.\t.'
    # 1 - 2Q = 0: kd is saturated, identity and de are not
    assert lines[3] == 'Self_Repeat_00003\ta\t60\t90\t2\t100\t100\t50\t0\t50\t0\t0\t0\t0\t0\t0.5000\t0.5000\t.'
    # counts beyond 2^32 print as they are; identical sequences: no minus sign in front of a zero
    assert lines[4] == 'Self_Repeat_00004\tc\t7\t9\t1\t5000000000\t5000000000\t5000000000\t0\t0\t0\t0\t0\t0\t0\t1.0000\t0.0000\t0.0000'
    assert len(lines) == 5 and all(len(l.split('\t')) == 18 for l in lines)
    # ID, seqid, start and end are those of the GFF3 row
    for l, g in zip(lines[1:], formats.gff_repeat_lines(regions, names, 'mimeo-self', 'Self_Repeat', 'Self_Repeat')):
        gf = g.split('\t')
        assert l.split('\t')[:4] == [gf[8][3:], gf[0], gf[3], gf[4]]
    # a second block (--strictSelf) goes without the header, and its IDs restart
    assert formats.region_stat_lines(regions[:1], names, 'p', stats[:1], [3], header=False) == ['p_00001' + lines[1][len('Self_Repeat_00001'):]]
    assert formats.region_stat_lines(regions[:0], names, 'p', stats[:0], []) == [formats.REGION_STATS_HEADER]
    # only ambiguous columns: columns > 0, no unambiguous one
    assert formats.region_stat_lines(regions[:1], names, 'p', _wstats((0, 0, 0, 10, 0, 0, 0, 0)), [1], header=False)[0].split('\t')[15:] == ['0.0000', '1.0000', '.']


def test_window_stats_layout_and_symbol():
    assert _ffi.WINDOW_ITEM.itemsize == 16 and _ffi.WINDOW_ITEM.names == ('aln', 'group', 'w0', 'w1')
    assert [_ffi.WINDOW_ITEM.fields[n] for n in _ffi.WINDOW_ITEM.names] == [(np.dtype('<u4'), k) for k in range(0, 16, 4)]
    assert _ffi.WINDOW_STATS.itemsize == 64 and _ffi.WINDOW_STATS.names == FIELDS == _ffi.COLUMN_STATS.names
    assert [_ffi.WINDOW_STATS.fields[n] for n in FIELDS] == [(np.dtype('<u8'), k) for k in range(0, 64, 8)]
    hdr = open(os.path.join(ROOT, 'include', 'mimeo_hip.h')).read()
    for name, names, ctype in (('mimeo_window_item', _ffi.WINDOW_ITEM.names, 'uint32_t'), ('mimeo_window_stats', FIELDS, 'uint64_t')):
        m = re.search(r'typedef struct %s \{(.*?)\} %s;' % (name, name), hdr, re.S)
        assert m, name
        body = re.sub(r'/\*.*?\*/', '', m.group(1))
        assert tuple(re.findall(r'\b([a-z_0-9]+)\s*[,;]', body)) == names
        assert set(re.findall(r'\b(u?int\d+_t)\b', body)) == {ctype}
    declared = set(re.findall(r'\b(mimeo_[a-z_]+)\s*\(', hdr))
    assert 'mimeo_path_window_stats' in declared and 'mimeo_path_window_stats' in _ffi.SYMBOLS
    assert declared == set(_ffi.SYMBOLS)
    assert re.search(r'#define MIMEO_ABI_VERSION 3\b', hdr) and _ffi.ABI_VERSION == 3
    lib = _ffi.load()
    assert hasattr(lib, 'mimeo_path_window_stats') and len(lib.mimeo_path_window_stats.argtypes) == 11


def test_region_stats_option(capsys):
    from mimeo_amd import run_interspecies, run_map, run_self
    for mod, base in ((run_self, ['--afasta', 'a.fa']), (run_interspecies, ['--afasta', 'a.fa', '--bfasta', 'b.fa'])):
        assert mod.mainArgs(base).regionStats is None
        assert mod.mainArgs(base + ['--regionStats', 'r.tsv']).regionStats == 'r.tsv'   # needs neither --paf nor --divergence
        args = mod.mainArgs(base + ['--regionStats', 'r.tsv', '--paf', 'x.paf', '--divergence'])
        assert (args.regionStats, args.paf, args.divergence) == ('r.tsv', 'x.paf', True)
    assert run_self.mainArgs(['--afasta', 'a.fa', '--strictSelf', '--regionStats', 'r.tsv']).strictSelf is True
    # `mimeo map` has no regions
    base = ['--afasta', 'a.fa', '--bfasta', 'b.fa']
    assert not hasattr(run_map.mainArgs(base), 'regionStats')
    with pytest.raises(SystemExit) as e:
        run_map.mainArgs(base + ['--regionStats', 'r.tsv'])
    assert e.value.code == 2
    assert 'unrecognized arguments: --regionStats' in capsys.readouterr().err


def test_window_stats_host_checks_under_sanitizers(tmp_path):
    src = os.path.join(ROOT, 'tests', 'sanitize', 'window_stats_check.cc')
    exe = tmp_path / 'window_stats_check_asan_ubsan'
    r = subprocess.run(['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', src, '-o', str(exe)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'window_stats_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
