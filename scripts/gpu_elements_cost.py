"""Cost of the element structure (DESIGN.md §4 "Element structure"): `mimeo self --elements` on the C2-sized synthetic genome
(the job of scripts/gpu_terminal_repeats_cost.py: synth_genome(50, 50 Mbp, 10 scaffolds)) through workflow.self_repeats — the
whole job's wall time without and with the flag, in one process — and two loads of the two entry points alone, with what
mimeo_flank_repeats (K18) and mimeo_open_frames (K19) say about themselves (MIMEO_ELEMENTS_STATS: the HIP-event time of the
kernels, the bases scanned): `features`, the engine.flank_repeats and engine.open_frames calls that the job makes (their
arguments are taken from a run of the job), and `designed`, 4096 items of 2048 random bases for K18 and the same items plus one
item of 10 Mbp for K19.  Medians of three after one warm-up each, every run listed.  One fresh process; nothing more is started
after a failure.

    python scripts/gpu_elements_cost.py > profiles/r31_elements_cost.json   (needs the GPU)
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
    out, calls = {}, {'flank': [], 'frames': []}
    real = {'flank': engine.flank_repeats, 'frames': engine.open_frames}

    def keep(which):
        def f(*args, **kw):
            calls[which].append((args, kw))
            return real[which](*args, **kw)
        return f

    with tempfile.TemporaryDirectory() as d:
        flag = {'elements': os.path.join(d, 'e.tsv')}
        for name, more in (('without', {}), ('with', flag)):
            wall = []
            for rep in range(4):   # the first run is the warm-up
                first = bool(more) and rep == 0
                engine.flank_repeats, engine.open_frames = (keep('flank'), keep('frames')) if first else (real['flank'], real['frames'])
                t0 = time.perf_counter()
                workflow.self_repeats(A, pairs, os.path.join(d, 'a.tab'), os.path.join(d, 'a.gff3'), prefix='Self_Repeat', label='Self_Repeat', **more)
                wall.append((time.perf_counter() - t0) * 1e3)
            out[name] = {'wall_ms': [round(w, 1) for w in wall[1:]], 'wall_ms_median': round(statistics.median(wall[1:]), 1)}
        rows = [r.split('\t') for r in open(flag['elements']).read().splitlines()[1:]]
        classes = {}
        for r in rows:
            classes[r[-1]] = classes.get(r[-1], 0) + 1
        out['with'].update({'lines': len(rows), 'classes': classes, 'with_tsd': sum(r[12] != '.' for r in rows),
                            'flank_repeats_calls': len(calls['flank']), 'open_frames_calls': len(calls['frames'])})
    (_, fiv), fkw = calls['flank'][0]
    (_, oiv), _ = calls['frames'][0]
    rng = np.random.Generator(np.random.PCG64(31))
    n, ln, big = 4096, 2048, 10_000_000
    D = engine.Genome(['d', 'big'], [np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, n * ln)], np.frombuffer(b'ACGT', dtype=np.uint8)[rng.integers(0, 4, big)]])
    designed = np.zeros(n + 1, dtype=engine._ffi.INTERVAL)
    designed['start'][:n] = np.arange(n) * ln
    designed['end'][:n] = designed['start'][:n] + ln
    designed[n] = (1, 0, big)
    os.environ['MIMEO_ELEMENTS_STATS'] = '1'
    loads = (('features_k18', lambda: real['flank'](A, fiv, **fkw), len(fiv)), ('features_k19', lambda: real['frames'](A, oiv), len(oiv)),
             ('designed_k18', lambda: real['flank'](D, designed[:n]), n), ('designed_k19', lambda: real['frames'](D, designed), n + 1))
    for name, fn, items in loads:
        wall = []
        for rep in range(4):
            sys.stderr.write('MARK %s %d\n' % (name, rep))
            sys.stderr.flush()
            t0 = time.perf_counter()
            res = fn()
            wall.append((time.perf_counter() - t0) * 1e3)
        found = int((res['len'] > 0).sum()) if name.endswith('k18') else int(res['codons'].max()) if res.size else 0
        out[name] = {'items': int(items), 'found' if name.endswith('k18') else 'longest_codons': found, 'wall_ms': [round(w, 3) for w in wall[1:]],
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
    for l in r.stderr.splitlines():   # the [k18] / [k19] line of a call lies behind its mark
        if l.startswith('MARK '):
            cur = tuple(l.split()[1:3])
        elif cur and cur[1] != '0' and l.startswith('[k18] flank repeats'):
            m = re.search(r'(\d+) launches, kernels ([0-9.]+) ms', l)
            out[cur[0]]['launches'] = int(m.group(1))
            ms.setdefault((cur[0], 'kernel_ms'), []).append(float(m.group(2)))
        elif cur and cur[1] != '0' and l.startswith('[k19] open frames'):
            m = re.search(r'(\d+) chunk jobs, (\d+) launches, (\d+) bases scanned, scan ([0-9.]+) ms, kernels ([0-9.]+) ms', l)
            out[cur[0]].update({'chunk_jobs': int(m.group(1)), 'launches': int(m.group(2)), 'bases_scanned': int(m.group(3))})
            ms.setdefault((cur[0], 'scan_ms'), []).append(float(m.group(4)))
            ms.setdefault((cur[0], 'kernel_ms'), []).append(float(m.group(5)))
    for (name, k), v in ms.items():
        out[name].update({k: [round(x, 4) for x in v], k + '_median': round(statistics.median(v), 4)})
    for name in ('features_k19', 'designed_k19'):
        if out[name].get('scan_ms_median'):
            out[name]['gbases_per_s_scan'] = round(out[name]['bases_scanned'] / out[name]['scan_ms_median'] / 1e6, 2)
    out = {'what': 'mimeo self --elements on the C2-sized synthetic genome (synth_genome(50, 50 Mbp, 10 scaffolds)) through workflow.self_repeats with the defaults '
                   'of mimeo self; one MI355X; medians of three after one warm-up; wall_ms of the whole job without and with the flag; features_k18 / features_k19: '
                   'the one engine.flank_repeats and the one engine.open_frames call of the job alone; designed_k18: 4096 items of 2048 random bases; designed_k19: '
                   'the same items and one item of 10 Mbp; wall and HIP-event time of the kernels (MIMEO_ELEMENTS_STATS; scan_ms is k19_scan alone), bases_scanned '
                   '= both strands of every item', 'made_by': 'python scripts/gpu_elements_cost.py', **out}
    print(json.dumps(out, indent=1))
