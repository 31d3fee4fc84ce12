"""Cost of the copy-to-consensus divergence (DESIGN.md §4 "Pileup and consensus", v4): `mimeo self --copyDivergence --landscape` on
the C2-sized synthetic genome (the job of scripts/gpu_stack_cost.py: synth_genome(50, 50 Mbp, 10 scaffolds)) through
workflow.self_repeats: the whole job's wall time without and with the two flags, and of the one engine.call_stats call that the
flags make (its arguments are taken from a run of the job) the wall time and what mimeo_path_call_stats (K16) says about itself
(MIMEO_CALL_STATS_STATS: the HIP-event time of its kernels, the two k16_pack_call launches among them).  K10 runs beside it in the
same process on the same items, each alone in a group (engine.window_stats, MIMEO_WINDOW_STATS_STATS).  Medians of three after
one warm-up each.  One fresh process; nothing more is started after a failure.

    python scripts/gpu_call_stats_cost.py > profiles/r29_call_stats_cost.json   (needs the GPU)
"""
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    from mimeo_amd import engine, workflow
    from mimeo_amd.synth import synth_genome
    engine.init(0)
    names, seqs = synth_genome(50, 50_000_000, 10)
    A = engine.Genome(names, seqs)
    pairs = workflow.all_pairs(len(names))
    out, calls = {}, []
    real = engine.call_stats

    def keep(*args):
        calls.append(args)
        return real(*args)

    with tempfile.TemporaryDirectory() as d:
        flags = {'copy_divergence': os.path.join(d, 'd.tsv'), 'landscape': os.path.join(d, 'l.tsv')}
        for name, more in (('without', {}), ('with', flags)):
            wall = []
            for rep in range(4):   # the first run is the warm-up
                engine.call_stats = keep if more and rep == 0 else real
                t0 = time.perf_counter()
                workflow.self_repeats(A, pairs, os.path.join(d, 'a.tab'), os.path.join(d, 'a.gff3'), prefix='Self_Repeat', label='Self_Repeat', **more)
                wall.append((time.perf_counter() - t0) * 1e3)
            out[name] = {'wall_ms': [round(w, 1) for w in wall[1:]], 'wall_ms_median': round(statistics.median(wall[1:]), 1)}
        rows = open(flags['copy_divergence']).read().splitlines()[1:]
        out['with'].update({'families': len({r.split('\t')[0] for r in rows}), 'lines': len(rows), 'call_stats_calls': len(calls),
                            'landscape_lines': len(open(flags['landscape']).read().splitlines()) - 1})
    # the one call of the job, alone, and K10 on the same items
    _, B, recs, f2, b2, win, run, sites, call, icall = calls[0]
    alone = run.copy()
    alone['group'] = np.arange(alone.size)
    out['call'] = {'items': int(run.size), 'windows': int(win.size), 'sites': int(sites.size), 'columns': int(call.size), 'insertion_columns': int(icall.size)}
    os.environ['MIMEO_CALL_STATS_STATS'] = os.environ['MIMEO_WINDOW_STATS_STATS'] = '1'
    for name, fn in (('k16', lambda: real(A, B, recs, f2, b2, win, run, sites, call, icall)), ('k10', lambda: engine.window_stats(A, B, recs, f2, b2, alone, alone.size))):
        wall = []
        for rep in range(4):
            sys.stderr.write('MARK %s %d\n' % (name, rep))
            sys.stderr.flush()
            t0 = time.perf_counter()
            fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        out[name] = {'wall_ms': [round(w, 3) for w in wall[1:]], 'wall_ms_median': round(statistics.median(wall[1:]), 3)}
    A.close()
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
    ms, cur = {}, None
    for l in r.stderr.splitlines():   # the [k16] / [k10] line of a call lies behind its mark
        if l.startswith('MARK '):
            cur = tuple(l.split()[1:3])
        elif cur and cur[1] != '0' and l.startswith('[%s]' % cur[0]):
            m = re.search(r'(\d+) jobs, .*kernels ([0-9.]+) ms', l)
            ms.setdefault(cur[0], []).append(float(m.group(2)))
            out[cur[0]]['jobs'] = int(m.group(1))
    for name, v in ms.items():
        out[name].update({'kernel_ms': [round(x, 4) for x in v], 'kernel_ms_median': round(statistics.median(v), 4)})
    out = {'what': 'mimeo self --copyDivergence --landscape on the C2-sized synthetic genome (synth_genome(50, 50 Mbp, 10 scaffolds)) through workflow.self_repeats '
                   'with the defaults of mimeo self; one MI355X; medians of three after one warm-up; wall_ms of the whole job without and with the two flags; k16: '
                   'the one engine.call_stats call of the job alone, wall and HIP-event time of its kernels (MIMEO_CALL_STATS_STATS); k10: engine.window_stats on '
                   'the same items, each alone in a group, in the same process', 'made_by': 'python scripts/gpu_call_stats_cost.py', **out}
    print(json.dumps(out, indent=1))
