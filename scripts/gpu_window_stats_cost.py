"""Cost of asking for per-region statistics (profiles/r13_window_stats_cost.json): wall time and HIP-event kernel time of
mimeo_path_window_stats (K10) over the kept rows (minLen 100, minIdt 80, as bench.py) of C2 and of one C4 row against the
regions their coverage collapses to (minCov 3), medians of three calls after one warm-up call; next to each the same figures of
mimeo_path_stats (K9) on the same rows in the same process — the two kernels read the same columns, the difference is the
clipping and the atomics; and the longest single window tried, the (0, 0) self diagonal of a C4 scaffold (one block of 10 Mbp)
under one window of its length, as one wavefront's work (MIMEO_WINDOW_STATS_SPLIT_BASES=0) and cut into jobs (the default).
One fresh process per case; nothing more is started after a case fails.

    python scripts/gpu_window_stats_cost.py [case ...] > raw.json   (needs the GPU; cases: c2 c4row)
"""
import json
import os
import re
import statistics
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ('c2', 'c4row')


def mark(name):
    sys.stderr.write('MARK %s\n' % name)
    sys.stderr.flush()


def child(case):
    import numpy as np
    from mimeo_amd import _ffi, engine, formats
    from mimeo_amd.dist import units_of_row
    from mimeo_amd.synth import synth_genome
    os.environ['MIMEO_WINDOW_STATS_STATS'] = '1'
    os.environ['MIMEO_PATH_STATS_STATS'] = '1'
    engine.init(0)
    if case == 'c2':
        names, seqs = synth_genome(50, 50_000_000, 10)
    else:
        names, seqs = synth_genome(1000, 1_000_000_000, 100)
    A = engine.Genome(names, seqs)
    n = len(names)
    if case == 'c4row':
        A.build_indexes()
        units = units_of_row(0, n)
    else:
        units = [(t, q, 3) for t in range(n) for q in range(n)]
    out = {}

    def timed(name, call, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        mark(name)
        wall = []
        for rep in range(4):   # the first call is the warm-up
            t0 = time.perf_counter()
            st = call()
            wall.append((time.perf_counter() - t0) * 1e3)
        mark('end')
        for k in (env or {}):
            del os.environ[k]
        cols = int(sum(st[f].astype(np.int64).sum() for f in ('matches', 'transitions', 'transversions', 'ambiguous')))
        out[name] = {'columns': cols, 'wall_ms': [round(w, 3) for w in wall[1:]], 'totals': {f: int(st[f].astype(np.int64).sum()) for f in st.dtype.names}}
        return st

    recs, first, blocks = engine.align_units(A, None, units, paths=True)
    rows = []
    _, kept_rows = formats.tab_blocks(recs, names, names, 100, 80, rows=rows)
    f2, b2 = formats.select_paths(first, blocks, rows[0])
    kept = recs[rows[0]]
    # the regions of the kept rows, as workflow.collapse_to_gff makes them (the names of synth_genome sort like their numbers)
    iv = kept_rows[:, [0, 2, 3]].astype(np.uint32)
    regions = engine.coverage_collapse(iv, [int(s.size) for s in seqs], 3, 100)
    t0 = time.perf_counter()
    items, per_region = formats.region_items(kept, regions, list(range(n)), first=f2, blocks=b2, self_job=True)
    join_ms = (time.perf_counter() - t0) * 1e3
    st = timed('window_stats_kept_rows', lambda: engine.window_stats(A, None, kept, f2, b2, items, len(regions)))
    out['window_stats_kept_rows'].update({'alignments': int(kept.size), 'path_blocks': int(b2.size), 'regions': int(len(regions)), 'items': int(items.size),
                                          'region_items_ms': round(join_ms, 3), 'alignments_returned': int(recs.size)})
    k9 = timed('path_stats_kept_rows', lambda: engine.path_stats(A, None, kept, f2, b2))
    out['path_stats_kept_rows'].update({'alignments': int(kept.size), 'path_blocks': int(b2.size)})
    assert (k9['matches'] == kept['id_n']).all()
    assert int(st['matches'].sum()) <= int(k9['matches'].astype(np.int64).sum())   # the regions are disjoint: a column lies in at most one
    if case == 'c4row':
        d = np.zeros(1, dtype=_ffi.ALIGNMENT)
        L = int(seqs[0].size)
        blk = np.array([(0, 0, L)], dtype=_ffi.PATH_BLOCK)
        one = np.array([0, 1], dtype=np.uint64)
        win = np.array([(0, 0, 0, L)], dtype=np.uint32)
        a = timed('self_diagonal_window_one_wavefront', lambda: engine.window_stats(A, None, d, one, blk, win, 1), {'MIMEO_WINDOW_STATS_SPLIT_BASES': '0'})
        b = timed('self_diagonal_window_split', lambda: engine.window_stats(A, None, d, one, blk, win, 1))
        k = timed('self_diagonal_path_stats_split', lambda: engine.path_stats(A, None, d, one, blk))
        assert a.tobytes() == b.tobytes() and int(a['matches'][0]) + int(a['ambiguous'][0]) == L and int(k['matches'][0]) == int(a['matches'][0])
    print('OUT ' + json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child(sys.argv[2])
        sys.exit(0)
    res = {}
    for case in (sys.argv[1:] or CASES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case], capture_output=True, text=True, timeout=1000)
        if r.returncode != 0:
            print(case, 'failed', r.returncode, r.stderr[-2000:], file=sys.stderr)
            sys.exit(1)   # nothing more on the GPU after a failure
        out = json.loads([l for l in r.stdout.splitlines() if l.startswith('OUT ')][0][4:])
        name = None
        for l in r.stderr.splitlines():   # the [k10] / [k9] lines of a measurement lie between its two marks; the first is the warm-up's
            if l.startswith('MARK '):
                name = l[5:].strip() if l[5:].strip() != 'end' else None
            elif name and (l.startswith('[k10] window stats') or l.startswith('[k9] path stats')):
                out[name].setdefault('stats_lines', []).append(l.strip())
        for name, o in out.items():
            ev = [float(re.search(r'kernels ([0-9.]+) ms', l).group(1)) for l in o['stats_lines'][1:]]
            o['kernel_ms'] = ev
            o['wall_ms_median'], o['kernel_ms_median'] = statistics.median(o['wall_ms']), statistics.median(ev)
            o['columns_per_second_kernel'] = o['columns'] / (o['kernel_ms_median'] * 1e-3) if o['kernel_ms_median'] else None
            o['stats_lines'] = o['stats_lines'][-1:]
        res[case] = out
    print(json.dumps(res, indent=1))
