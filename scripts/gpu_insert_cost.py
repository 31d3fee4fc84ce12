"""Cost of the inserted columns of a consensus library (DESIGN.md §4 "Pileup and consensus", v2): wall time and HIP-event kernel
time of mimeo_path_insertions (K14) on a C2-sized self job, next to mimeo_path_pileup (K13) on the same windows and items — the
job of scripts/gpu_pileup_cost.py: the kept rows (minLen 100, minIdt 80, as bench.py) of C2, the regions their coverage collapses
to (minCov 3), the families of those regions (K12) and, as `mimeo self --consensus --consensusInsertions` asks for them, the
representative region of every family as a window with the items of that region, the sites formats.insertion_sites picks from
K13's counts, and one engine.insertions call over them — medians of three calls after one warm-up call.  Also the whole region
set as windows.  One fresh process; nothing more is started after a failure.

    python scripts/gpu_insert_cost.py > raw.json   (needs the GPU)
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
    os.environ['MIMEO_INSERT_STATS'] = '1'
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
        """the regions `which` as windows, with their items and the sites of their pile"""
        win = np.zeros(which.size, dtype=_ffi.PILEUP_WINDOW)
        win['tid'], win['start'], win['end'] = regions['chrom'][which], regions['start'][which], regions['end'][which]
        window_of = np.full(len(regions), -1, dtype=np.int64)
        window_of[which] = np.arange(which.size)
        its = items[window_of[items['group'].astype(np.int64)] >= 0].copy()
        its['group'] = window_of[its['group'].astype(np.int64)]
        cols, call = timed('pileup_' + tag, lambda: engine.pileup(A, None, kept, f2, b2, win, its))
        t0 = time.perf_counter()
        sites = formats.insertion_sites(win, cols)
        t_sites = (time.perf_counter() - t0) * 1e3
        res, icols, icall = timed('insertions_' + tag, lambda: engine.insertions(A, None, kept, f2, b2, win, its, sites))
        # the second witness, on the way: runs and bases are K13's at the sites' columns, and no run is longer than its site
        col_first = np.concatenate([[0], np.cumsum(win['end'].astype(np.int64) - win['start'])])
        at = col_first[sites['window'].astype(np.int64)] + sites['x'].astype(np.int64) - win['start'].astype(np.int64)[sites['window'].astype(np.int64)]
        assert (res['runs'] == cols['ins_runs'][at]).all() and (res['bases'] == cols['ins_bases'][at]).all() and not res['longer'].any()
        for name in ('pileup_' + tag, 'insertions_' + tag):
            out[name].update({'windows': int(which.size), 'items': int(its.size), 'columns': int(cols.size), 'alignments': int(kept.size),
                              'path_blocks': int(b2.size)})
        out['insertions_' + tag].update({'sites': int(sites.size), 'insertion_columns': int(icall.size), 'runs': int(res['runs'].astype(np.int64).sum()),
                                         'bases': int(res['bases'].astype(np.int64).sum()), 'longest_run': int(res['max_len'].max()) if res.size else 0,
                                         'insertion_sites_host_ms': round(t_sites, 3),
                                         'called': {chr(b): int(k) for b, k in zip(*np.unique(icall, return_counts=True))}})

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
    for l in r.stderr.splitlines():   # the [k13] / [k14] lines of a measurement lie between its two marks; the first is the warm-up's
        if l.startswith('MARK '):
            name = l[5:].strip() if l[5:].strip() != 'end' else None
        elif name and (l.startswith('[k13] pileup') or l.startswith('[k14] insertions')):
            out[name].setdefault('stats_lines', []).append(l.strip())
    for name, o in out.items():
        if 'stats_lines' not in o:
            continue
        ev = [float(re.search(r'kernels ([0-9.]+) ms', l).group(1)) for l in o['stats_lines'][1:]]
        o['kernel_ms'] = ev
        o['wall_ms_median'], o['kernel_ms_median'] = statistics.median(o['wall_ms']), statistics.median(ev)
        o['stats_lines'] = o['stats_lines'][-1:]
        print(name + ': ' + o['stats_lines'][0], file=sys.stderr)
        print('%s: kernels %.3f ms, wall %.3f ms (medians of three)' % (name, o['kernel_ms_median'], o['wall_ms_median']), file=sys.stderr)
    print(json.dumps(out, indent=1))
