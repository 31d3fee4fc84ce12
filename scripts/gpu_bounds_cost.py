"""Cost of mimeo_params.bound_extensions (profiles/r06_bounds_cost.json): ms_gapped and the MIMEO_K6_STATS path-rule line of
mimeo_align_pairs under the path anchor rule without and with the bounds, alternated, on C2, the 8-scaffold flanked genome and
the 8 x 150 kbp tandem genome; one fresh process per case, nothing more is started after a case fails.

    python scripts/gpu_bounds_cost.py > raw.json   (needs the GPU)
"""
import json
import os
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def genome(case):
    from mimeo_amd.synth import synth_genome, tandem_genome, flanked_tandem_genome
    if case == 'c2':
        return synth_genome(50, 50_000_000, 10)
    if case == 'tandem':
        return tandem_genome(7, 8, 150_000)
    return flanked_tandem_genome(7, 8)


def child(case):
    import numpy as np
    from mimeo_amd import engine
    engine.init(0)
    names, seqs = genome(case)
    A = engine.Genome(names, seqs)
    n = len(names)
    pairs = [(t, q) for t in range(n) for q in range(n)]
    rows = []
    for rep in range(3):
        for bnd in (0, 1):
            engine.align_pairs(A, None, pairs, engine.default_params(anchor_rule=1, bound_extensions=bnd)) if rep == 0 else None
            al = engine.align_pairs(A, None, pairs, engine.default_params(anchor_rule=1, bound_extensions=bnd))
            st = engine.stats()
            rows.append({'case': case, 'bound_extensions': bnd, 'ms_gapped': round(st['ms_gapped'], 3), 'ms_total': round(st['ms_total'], 3),
                         'alignments': int(al.size), 'aligned_target_bases': int((al['tend'].astype(np.int64) - al['tstart']).sum()),
                         'failed_pairs': len(engine.failed_pairs())})
    os.environ['MIMEO_K6_STATS'] = '1'
    for bnd in (0, 1):
        sys.stderr.write('STATS bnd=%d\n' % bnd)
        sys.stderr.flush()
        engine.align_pairs(A, None, pairs, engine.default_params(anchor_rule=1, bound_extensions=bnd))
    print('ROWS ' + json.dumps(rows))


if __name__ == '__main__':
    if len(sys.argv) > 1:
        child(sys.argv[1])
        sys.exit(0)
    out = {}
    for case in ('flanked', 'tandem', 'c2'):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), case], capture_output=True, text=True, timeout=500)
        if r.returncode != 0:
            print(case, 'failed', r.returncode, r.stderr[-2000:], file=sys.stderr)
            sys.exit(1)   # nothing more on the GPU after a failure
        rows = json.loads([l for l in r.stdout.splitlines() if l.startswith('ROWS ')][0][5:])
        lines, cur = {}, None
        for l in r.stderr.splitlines():
            if l.startswith('STATS bnd='):
                cur = l.split('=')[1]
            elif cur is not None and 'path rule: traceback' in l:
                lines[cur] = l.strip()
        out[case] = {'rows': rows, 'stats_line': lines}
    print(json.dumps(out, indent=1))
