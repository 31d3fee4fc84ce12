"""Cost of a consensus library (DESIGN.md §4 "Pileup and consensus"): wall time and HIP-event kernel time of mimeo_path_pileup
(K13) on a C2-sized self job — the kept rows (minLen 100, minIdt 80, as bench.py) of C2, the regions their coverage collapses to
(minCov 3), the families of those regions (K12) and, as `mimeo self --consensus` asks for them, the representative region of
every family as a window with the items of that region — medians of three calls after one warm-up call; next to it the same
figures of mimeo_path_window_stats (K10) on the SAME items with one group per window: the existing neighbour that reads the same
records, blocks and query bases and keeps eight sums per window where K13 keeps eight counters per column.  Also the whole
region set as windows (every region, not only the representatives), the larger call a user of engine.pileup can make.  One
fresh process; nothing more is started after a failure.

    python scripts/gpu_pileup_cost.py > raw.json   (needs the GPU)
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


def mark(name):
    sys.stderr.write('MARK %s\n' % name)
    sys.stderr.flush()


def child():
    import numpy as np
    from mimeo_amd import _ffi, engine, formats
    from mimeo_amd.synth import synth_genome
    os.environ['MIMEO_PILEUP_STATS'] = '1'
    os.environ['MIMEO_WINDOW_STATS_STATS'] = '1'
    engine.init(0)
    names, seqs = synth_genome(50, 50_000_000, 10)
    A = engine.Genome(names, seqs)
    n = len(names)
    out = {}

    def timed(name, call):
        mark(name)
        wall = []
        for rep in range(4):   # the first call is the warm-up
            t0 = time.perf_counter()
            res = call()
            wall.append((time.perf_counter() - t0) * 1e3)
        mark('end')
        out[name] = {'wall_ms': [round(w, 3) for w in wall[1:]]}
        return res

    recs, first, blocks = engine.align_units(A, None, [(t, q, 3) for t in range(n) for q in range(n)], paths=True)
    rows = []
    _, kept_rows = formats.tab_blocks(recs, names, names, 100, 80, rows=rows)
    f2, b2 = formats.select_paths(first, blocks, rows[0])
    kept = recs[rows[0]]
    # the regions of the kept rows, as workflow.collapse_to_gff makes them (the names of synth_genome sort like their numbers)
    regions = engine.coverage_collapse(kept_rows[:, [0, 2, 3]].astype(np.uint32), [int(s.size) for s in seqs], 3, 100)
    items, _ = formats.region_items(kept, regions, list(range(n)), first=f2, blocks=b2, self_job=True)
    family, links = engine.link_regions(A, kept, f2, b2, regions, list(range(n)), items, 80)
    reps = formats.family_representatives(regions, family, links)

    def case(tag, which):
        """the regions `which` as windows, with their items"""
        win = np.zeros(which.size, dtype=_ffi.PILEUP_WINDOW)
        win['tid'], win['start'], win['end'] = regions['chrom'][which], regions['start'][which], regions['end'][which]
        window_of = np.full(len(regions), -1, dtype=np.int64)
        window_of[which] = np.arange(which.size)
        its = items[window_of[items['group'].astype(np.int64)] >= 0].copy()
        its['group'] = window_of[its['group'].astype(np.int64)]
        cols, call = timed('pileup_' + tag, lambda: engine.pileup(A, None, kept, f2, b2, win, its))
        ws = timed('window_stats_' + tag, lambda: engine.window_stats(A, None, kept, f2, b2, its, which.size))
        ncols = int(cols.size)
        depth = sum(int(cols[f].astype(np.int64).sum()) for f in ('a', 'c', 'g', 't', 'n', 'del'))
        # the second witness, on the way: the columns' sums are K10's
        assert sum(int(cols[f].astype(np.int64).sum()) for f in ('a', 'c', 'g', 't', 'n')) == sum(int(ws[f].sum()) for f in ('matches', 'transitions', 'transversions', 'ambiguous'))
        assert int(cols['del'].astype(np.int64).sum()) == int(ws['del_bases'].sum()) and int(cols['ins_bases'].astype(np.int64).sum()) == int(ws['ins_bases'].sum())
        for name in ('pileup_' + tag, 'window_stats_' + tag):
            out[name].update({'windows': int(which.size), 'items': int(its.size), 'columns': ncols, 'pile': depth, 'mean_depth': round(depth / max(ncols, 1), 3),
                              'alignments': int(kept.size), 'path_blocks': int(b2.size)})
        # bytes that cross the ABI per column (32 of counts, 1 of call), and what the device moves per column besides the pile
        # itself: the counts zeroed (32), added to at least once where a column is covered, read by k13_call (32), the call
        # written (1), both copied out (33)
        out['pileup_' + tag].update({'bytes_out_per_column': 33, 'device_bytes_per_column_floor': 32 + 32 + 1 + 33,
                                     'called': {chr(b): int(k) for b, k in zip(*np.unique(call, return_counts=True))}})

    case('representatives', np.array([i for i, _ in reps], dtype=np.int64))
    case('all_regions', np.arange(len(regions), dtype=np.int64))
    out['job'] = {'alignments_returned': int(recs.size), 'kept': int(kept.size), 'regions': int(len(regions)), 'families': len(reps)}
    print('OUT ' + json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child()
        sys.exit(0)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child'], capture_output=True, text=True, timeout=1000)
    if r.returncode != 0:
        print('failed', r.returncode, r.stderr[-3000:], file=sys.stderr)
        sys.exit(1)   # nothing more on the GPU after a failure
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('OUT ')][0][4:])
    name = None
    for l in r.stderr.splitlines():   # the [k13] / [k10] lines of a measurement lie between its two marks; the first is the warm-up's
        if l.startswith('MARK '):
            name = l[5:].strip() if l[5:].strip() != 'end' else None
        elif name and (l.startswith('[k13] pileup') or l.startswith('[k10] window stats')):
            out[name].setdefault('stats_lines', []).append(l.strip())
    for name, o in out.items():
        if 'stats_lines' not in o:
            continue
        ev = [float(re.search(r'kernels ([0-9.]+) ms', l).group(1)) for l in o['stats_lines'][1:]]
        o['kernel_ms'] = ev
        o['wall_ms_median'], o['kernel_ms_median'] = statistics.median(o['wall_ms']), statistics.median(ev)
        o['columns_per_second_kernel'] = o['columns'] / (o['kernel_ms_median'] * 1e-3) if o['kernel_ms_median'] else None
        o['stats_lines'] = o['stats_lines'][-1:]
        print(name + ': ' + o['stats_lines'][0], file=sys.stderr)
        print('%s: kernels %.3f ms, wall %.3f ms (medians of three)' % (name, o['kernel_ms_median'], o['wall_ms_median']), file=sys.stderr)
    print(json.dumps(out, indent=1))
