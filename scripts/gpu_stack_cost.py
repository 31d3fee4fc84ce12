"""Cost of the family seed alignments (DESIGN.md §4 "Pileup and consensus", v3): `mimeo self --familyAlignments` on the C2-sized
synthetic genome (the job of scripts/gpu_pileup_cost.py: synth_genome(50, 50 Mbp, 10 scaffolds)) through workflow.self_repeats,
the whole job's wall time without and with the flag, and of the run with the flag what mimeo_path_stack (K15) says about itself
(MIMEO_PATH_STACK_STATS: the HIP-event time of its kernels and the bytes it wrote, summed over the job's engine.stack calls) —
three runs each after one warm-up run.  --root DIR: import mimeo_amd from another checkout (one that was built), to put a parent
commit's wall time without the flag next to this one's; a tree without the flag measures only that.  One fresh process; nothing
more is started after a failure.

    python scripts/gpu_stack_cost.py [--root DIR] > raw.json   (needs the GPU)
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


def child(root):
    sys.path.insert(0, root)
    import inspect
    from mimeo_amd import engine, workflow
    from mimeo_amd.synth import synth_genome
    os.environ['MIMEO_PATH_STACK_STATS'] = '1'
    engine.init(0)
    names, seqs = synth_genome(50, 50_000_000, 10)
    A = engine.Genome(names, seqs)
    pairs = workflow.all_pairs(len(names))
    has_flag = 'family_alignments' in inspect.signature(workflow.self_repeats).parameters
    out = {'root': os.path.relpath(root, ROOT), 'has_flag': has_flag}
    with tempfile.TemporaryDirectory() as d:
        for name, more in (('without', {}), ('with', {'family_alignments': os.path.join(d, 'fam.sto')})):
            if more and not has_flag:
                continue
            wall = []
            for rep in range(4):   # the first run is the warm-up
                sys.stderr.write('MARK %s %d\n' % (name, rep))
                sys.stderr.flush()
                t0 = time.perf_counter()
                workflow.self_repeats(A, pairs, os.path.join(d, 'a.tab'), os.path.join(d, 'a.gff3'), prefix='Self_Repeat', label='Self_Repeat', **more)
                wall.append((time.perf_counter() - t0) * 1e3)
            out[name] = {'wall_ms': [round(w, 1) for w in wall[1:]], 'wall_ms_median': round(statistics.median(wall[1:]), 1)}
            if more:
                text = open(more['family_alignments']).read()
                out[name].update({'file_bytes': len(text), 'families': text.count('# STOCKHOLM 1.0'),
                                  'sequence_rows': sum(1 for l in text.splitlines() if l and not l.startswith('#') and l != '//')})
    A.close()
    print('OUT ' + json.dumps(out))


if __name__ == '__main__':
    if len(sys.argv) > 2 and sys.argv[1] == '--child':
        child(sys.argv[2])
        sys.exit(0)
    root = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] == '--root' else ROOT
    r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', root], capture_output=True, text=True, timeout=1000)
    if r.returncode != 0:
        print('failed', r.returncode, r.stderr[-3000:], file=sys.stderr)
        sys.exit(1)   # nothing more on the GPU after a failure
    out = json.loads([l for l in r.stdout.splitlines() if l.startswith('OUT ')][0][4:])
    runs, cur = {}, None
    for l in r.stderr.splitlines():   # the [k15] lines of a run lie behind its mark
        if l.startswith('MARK '):
            cur = tuple(l.split()[1:3])
        elif cur and l.startswith('[k15] stack'):
            m = re.search(r'(\d+) items, (\d+) sites, (\d+) bytes, (\d+) jobs, .*kernels ([0-9.]+) ms', l)
            run = runs.setdefault(cur, {'calls': 0, 'items': 0, 'bytes': 0, 'jobs': 0, 'kernel_ms': 0.0})
            run['calls'] += 1
            for k, v in zip(('items', 'bytes', 'jobs'), (m.group(1), m.group(3), m.group(4))):
                run[k] += int(v)
            run['kernel_ms'] += float(m.group(5))
    timed = [v for (name, rep), v in sorted(runs.items()) if name == 'with' and rep != '0']
    if timed:
        ms = statistics.median(v['kernel_ms'] for v in timed)
        out['with']['stack'] = dict(timed[-1], kernel_ms=[round(v['kernel_ms'], 4) for v in timed], kernel_ms_median=round(ms, 4),
                                    bytes_per_second=round(timed[-1]['bytes'] / (ms * 1e-3)) if ms else None)
    print(json.dumps(out, indent=1))
