"""Cost of the terminal repeats (DESIGN.md §4 "Terminal repeats"): `mimeo self --terminalRepeats` on the C2-sized synthetic genome
(the job of scripts/gpu_call_stats_cost.py: synth_genome(50, 50 Mbp, 10 scaffolds)) through workflow.self_repeats — the whole job's
wall time without and with the flag — and two loads of the one entry point alone, with what mimeo_terminal_repeats (K17) says
about itself (MIMEO_TERMINAL_STATS: the HIP-event time of k17_dp and of k17_walk apart, the cells computed): `features`, the
engine.terminal_repeats call that the job makes (its arguments are taken from a run of the job), and `designed`, 2048 items of
2048 random bases, which is 4096 jobs at w = 1024.  Medians of three after one warm-up each.  One fresh process; nothing more is
started after a failure.

    python scripts/gpu_terminal_repeats_cost.py > profiles/r30_terminal_repeats_cost.json   (needs the GPU)
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
    real = engine.terminal_repeats

    def keep(*args, **kw):
        calls.append((args, kw))
        return real(*args, **kw)

    with tempfile.TemporaryDirectory() as d:
        flag = {'terminal_repeats': os.path.join(d, 't.tsv')}
        for name, more in (('without', {}), ('with', flag)):
            wall = []
            for rep in range(4):   # the first run is the warm-up
                engine.terminal_repeats = keep if more and rep == 0 else real
                t0 = time.perf_counter()
                workflow.self_repeats(A, pairs, os.path.join(d, 'a.tab'), os.path.join(d, 'a.gff3'), prefix='Self_Repeat', label='Self_Repeat', **more)
                wall.append((time.perf_counter() - t0) * 1e3)
            out[name] = {'wall_ms': [round(w, 1) for w in wall[1:]], 'wall_ms_median': round(statistics.median(wall[1:]), 1)}
        rows = [r.split('\t') for r in open(flag['terminal_repeats']).read().splitlines()[1:]]
        out['with'].update({'lines': len(rows), 'ltr_lines': sum(r[4] == 'LTR' for r in rows), 'tir_lines': sum(r[4] == 'TIR' for r in rows),
                            'terminal_repeats_calls': len(calls)})
    (_, iv), kw = calls[0]
    rng = np.random.Generator(np.random.PCG64(30))
    D = engine.Genome(['d'], [np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, 2048 * 2048)]])
    designed = np.zeros(2048, dtype=engine._ffi.INTERVAL)
    designed['start'] = np.arange(2048) * 2048
    designed['end'] = designed['start'] + 2048
    os.environ['MIMEO_TERMINAL_STATS'] = '1'
    for name, fn, n in (('features', lambda: real(A, iv, **kw), len(iv)), ('designed', lambda: real(D, designed), 2048)):
        wall = []
        for rep in range(4):
            sys.stderr.write('MARK %s %d\n' % (name, rep))
            sys.stderr.flush()
            t0 = time.perf_counter()
            recs, _, blocks = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        out[name] = {'items': int(n), 'found': int((recs['score'] > 0).sum()), 'blocks': int(blocks.size), 'wall_ms': [round(w, 3) for w in wall[1:]],
                     'wall_ms_median': round(statistics.median(wall[1:]), 3)}
    D.close()
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
    for l in r.stderr.splitlines():   # the [k17] line of a call lies behind its mark
        if l.startswith('MARK '):
            cur = tuple(l.split()[1:3])
        elif cur and cur[1] != '0' and l.startswith('[k17]'):
            m = re.search(r'(\d+) jobs, (\d+) launches, (\d+) cells, dp ([0-9.]+) ms, walk ([0-9.]+) ms, kernels ([0-9.]+) ms', l)
            out[cur[0]].update({'jobs': int(m.group(1)), 'launches': int(m.group(2)), 'cells': int(m.group(3))})
            for k, g in (('dp_ms', 4), ('walk_ms', 5), ('kernel_ms', 6)):
                ms.setdefault((cur[0], k), []).append(float(m.group(g)))
    for (name, k), v in ms.items():
        out[name].update({k: [round(x, 4) for x in v], k + '_median': round(statistics.median(v), 4)})
    for name in ('features', 'designed'):
        if out[name].get('dp_ms_median'):
            out[name]['gcells_per_s_dp'] = round(out[name]['cells'] / out[name]['dp_ms_median'] / 1e6, 2)
    out = {'what': 'mimeo self --terminalRepeats on the C2-sized synthetic genome (synth_genome(50, 50 Mbp, 10 scaffolds)) through workflow.self_repeats with the '
                   'defaults of mimeo self; one MI355X; medians of three after one warm-up; wall_ms of the whole job without and with the flag; features: the one '
                   'engine.terminal_repeats call of the job alone; designed: 2048 items of 2048 random bases, 4096 jobs at w = 1024; wall and HIP-event time of '
                   'k17_dp and k17_walk apart (MIMEO_TERMINAL_STATS), cells = the sum of w * w over the jobs', 'made_by': 'python scripts/gpu_terminal_repeats_cost.py',
           **out}
    print(json.dumps(out, indent=1))
