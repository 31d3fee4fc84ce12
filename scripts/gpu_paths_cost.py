"""Cost of asking for alignment paths (profiles/r08_paths_cost.json): ms_gapped of the same call under the box rule without
and with paths (mimeo_align_units against mimeo_align_units_paths), alternated, three times each, medians; on C2, the
8 x 150 kbp tandem genome and one C4 row (target row 0 of the 1 Gbp genome, as bench.py issues it).  One fresh process per
case; nothing more is started after a case fails.

    python scripts/gpu_paths_cost.py [case ...] > raw.json   (needs the GPU; cases: tandem c2 c4row)
"""
import json
import os
import statistics
import subprocess
import sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ('tandem', 'c2', 'c4row')


def child(case):
    import numpy as np
    from mimeo_amd import engine
    from mimeo_amd.dist import units_of_row
    from mimeo_amd.synth import synth_genome, tandem_genome
    engine.init(0)
    if case == 'c2':
        names, seqs = synth_genome(50, 50_000_000, 10)
    elif case == 'tandem':
        names, seqs = tandem_genome(7, 8, 150_000)
    else:
        names, seqs = synth_genome(1000, 1_000_000_000, 100)
    A = engine.Genome(names, seqs)
    n = len(names)
    if case == 'c4row':
        A.build_indexes()
        units = units_of_row(0, n)
    else:
        units = [(t, q, 3) for t in range(n) for q in range(n)]

    def call(paths):
        if case == 'c4row':
            A.drop_indexes([0])
        return engine.align_units(A, None, units, paths=paths)

    call(False)
    call(True)
    rows = []
    for rep in range(3):
        for paths in (False, True):
            res = call(paths)
            st = engine.stats()
            al = res[0] if paths else res
            rows.append({'case': case, 'paths': int(paths), 'ms_gapped': round(st['ms_gapped'], 3), 'ms_total': round(st['ms_total'], 3),
                         'alignments': int(al.size), 'path_blocks': int(res[2].size) if paths else 0,
                         'most_blocks': int(np.diff(res[1].astype(np.int64)).max()) if paths and al.size else 0,
                         'failed_pairs': len(engine.failed_pairs())})
    os.environ['MIMEO_K6_STATS'] = '1'
    call(True)
    print('ROWS ' + json.dumps(rows))


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child(sys.argv[2])
        sys.exit(0)
    out = {}
    for case in (sys.argv[1:] or CASES):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', case], capture_output=True, text=True, timeout=900)
        if r.returncode != 0:
            print(case, 'failed', r.returncode, r.stderr[-2000:], file=sys.stderr)
            sys.exit(1)   # nothing more on the GPU after a failure
        rows = json.loads([l for l in r.stdout.splitlines() if l.startswith('ROWS ')][0][5:])
        med = {str(p): statistics.median(x['ms_gapped'] for x in rows if x['paths'] == p) for p in (0, 1)}
        out[case] = {'ms_gapped_median': {'without': med['0'], 'with_paths': med['1']}, 'rows': rows,
                     'stats_lines': [l.strip() for l in r.stderr.splitlines() if 'paths out: traceback' in l]}
    print(json.dumps(out, indent=1))
