"""Cost of asking for alignment text (profiles/r15_path_text_cost.json): wall time and HIP-event kernel time of mimeo_path_text
(K11) over the kept rows (minLen 100, minIdt 80, as bench.py) of one C4 row, medians of three calls after one warm-up call, and
the bytes written per second (two rows: 2 bytes per column); and the longest single alignment tried, the (0, 0) self diagonal
of a C4 scaffold (one block of 10 Mbp) alone, as one wavefront's work (MIMEO_PATH_TEXT_SPLIT_COLUMNS=0) and cut into jobs (the
default).  One fresh process per case; nothing more is started after a case fails.

    python scripts/gpu_path_text_cost.py [case ...] > raw.json   (needs the GPU; cases: c4row)
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

CASES = ('c4row',)


def mark(name):
    sys.stderr.write('MARK %s\n' % name)
    sys.stderr.flush()


def child(case):
    import numpy as np
    from mimeo_amd import _ffi, engine, formats
    from mimeo_amd.dist import units_of_row
    from mimeo_amd.synth import synth_genome
    os.environ['MIMEO_PATH_TEXT_STATS'] = '1'
    engine.init(0)
    names, seqs = synth_genome(1000, 1_000_000_000, 100)
    A = engine.Genome(names, seqs)
    n = len(names)
    A.build_indexes()
    units = units_of_row(0, n)
    out = {}

    def timed(name, recs, first, blocks, env=None):
        for k, v in (env or {}).items():
            os.environ[k] = v
        mark(name)
        wall = []
        for rep in range(4):   # the first call is the warm-up
            t0 = time.perf_counter()
            rf, tr, qr = engine.path_text(A, None, recs, first, blocks)
            wall.append((time.perf_counter() - t0) * 1e3)
        mark('end')
        for k in (env or {}):
            del os.environ[k]
        out[name] = {'alignments': int(recs.size), 'path_blocks': int(blocks.size), 'columns': int(rf[-1]), 'wall_ms': [round(w, 3) for w in wall[1:]]}
        return rf, tr, qr

    recs, first, blocks = engine.align_units(A, None, units, paths=True)
    rows = []
    formats.tab_blocks(recs, names, names, 100, 80, rows=rows)
    f2, b2 = formats.select_paths(first, blocks, rows[0])
    kept = recs[rows[0]]
    rf, tr, qr = timed('kept_rows', kept, f2, b2)
    # the rows against what the records say: matches, and the two slices' lengths
    st = engine.path_stats(A, None, kept, f2, b2)
    eq = (tr == qr) & (tr != ord('N')) & (tr != ord('-'))
    csum = np.concatenate([[0], np.cumsum(eq)])
    assert ((csum[rf[1:].astype(np.int64)] - csum[rf[:-1].astype(np.int64)]) == st['matches']).all() and (st['matches'] == kept['id_n']).all()
    assert int(np.count_nonzero(tr != ord('-'))) == int((kept['tend'].astype(np.int64) - kept['tstart']).sum())
    out['kept_rows']['alignments_returned'] = int(recs.size)
    d = np.zeros(1, dtype=_ffi.ALIGNMENT)
    L = int(seqs[0].size)
    blk = np.array([(0, 0, L)], dtype=_ffi.PATH_BLOCK)
    one = np.array([0, 1], dtype=np.uint64)
    a = timed('self_diagonal_one_wavefront', d, one, blk, {'MIMEO_PATH_TEXT_SPLIT_COLUMNS': '0'})
    b = timed('self_diagonal_split', d, one, blk)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and (b[1] == b[2]).all() and int(b[0][1]) == L
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
        for l in r.stderr.splitlines():   # the [k11] lines of a measurement lie between its two marks; the first is the warm-up's
            if l.startswith('MARK '):
                name = l[5:].strip() if l[5:].strip() != 'end' else None
            elif name and l.startswith('[k11] path text'):
                out[name].setdefault('stats_lines', []).append(l.strip())
        for name, o in out.items():
            ev = [float(re.search(r'kernels ([0-9.]+) ms', l).group(1)) for l in o['stats_lines'][1:]]
            o['kernel_ms'] = ev
            o['wall_ms_median'], o['kernel_ms_median'] = statistics.median(o['wall_ms']), statistics.median(ev)
            o['bytes_written_per_second_kernel'] = 2 * o['columns'] / (o['kernel_ms_median'] * 1e-3) if o['kernel_ms_median'] else None
            o['bytes_written_per_second_wall'] = 2 * o['columns'] / (o['wall_ms_median'] * 1e-3)
            o['stats_lines'] = o['stats_lines'][-1:]
        res[case] = out
    print(json.dumps(res, indent=1))
