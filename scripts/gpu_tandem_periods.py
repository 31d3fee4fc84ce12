"""Time of engine.tandem_masked (K8) against --tmaxperiod (profiles/r07_tandem_periods.jsonl): a fixed seeded set of
20 000 slices of 100 .. 20 000 bases (log-uniform) of an 8 x 2 Mbp synth genome with 1 % microsatellites and six long-unit
arrays per scaffold; a host clock around the call, which ends in a stream synchronise.  With --parent-lib (a
libmimeo_hip.so built from the parent commit) the two builds run alternately, a fresh process each, five times: the
parent at maxperiod 50 and 64, this build at 50, 64, 128, 200, 500 and 2000; every process warms every period up once
before it times it.  Nothing more is started after a process fails.

    python scripts/gpu_tandem_periods.py [--parent-lib PATH] > raw.jsonl   (needs the GPU)
"""
import json
import os
import subprocess
import sys
import time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

NEW_PERIODS = (50, 64, 128, 200, 500, 2000)
PARENT_PERIODS = (50, 64)
REPEATS = 5


def workload():
    import numpy as np
    from mimeo_amd.synth import add_tandem_arrays, synth_genome
    names, arrs = synth_genome(71, 16_000_000, 8, microsat_frac=0.01)
    arrs = add_tandem_arrays(71, arrs, 6)
    rng = np.random.default_rng(72)
    n = 20_000
    ln = np.exp(rng.uniform(np.log(100), np.log(20_000), n)).astype(np.int64)
    chrom = rng.integers(0, len(arrs), n)
    start = (rng.random(n) * (len(arrs[0]) - ln)).astype(np.int64)
    return names, arrs, np.stack([chrom, start, start + ln], 1).astype(np.uint32)


def child(lib, periods):
    from mimeo_amd import _ffi
    if lib != '-':
        _ffi.LIB_PATH = os.path.abspath(lib)
    from mimeo_amd import engine
    engine.init(0)
    names, arrs, iv = workload()
    A = engine.Genome(names, arrs)
    for mp in periods:
        engine.tandem_masked(A, iv, maxperiod=mp)          # warm-up
        t0 = time.perf_counter()
        m = engine.tandem_masked(A, iv, maxperiod=mp)
        ms = (time.perf_counter() - t0) * 1e3
        print('ROW ' + json.dumps({'maxperiod': mp, 'ms': round(ms, 3), 'masked_bases': int(m.astype('int64').sum()),
                                   'slices': int(iv.shape[0]), 'slice_bases': int((iv[:, 2] - iv[:, 1]).astype('int64').sum())}), flush=True)
    A.close()


if __name__ == '__main__':
    if len(sys.argv) > 1 and sys.argv[1] == '--child':
        child(sys.argv[2], [int(x) for x in sys.argv[3:]])
        sys.exit(0)
    parent = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == '--parent-lib' else None
    for rep in range(REPEATS):
        for build, lib, periods in (('parent', parent, PARENT_PERIODS), ('new', '-', NEW_PERIODS)):
            if lib is None:
                continue
            r = subprocess.run([sys.executable, os.path.abspath(__file__), '--child', lib] + [str(p) for p in periods],
                               capture_output=True, text=True, timeout=240)
            if r.returncode != 0:
                print(build, 'failed', r.returncode, r.stdout[-1000:], r.stderr[-2000:], file=sys.stderr)
                sys.exit(1)   # nothing more on the GPU after a failure
            for l in r.stdout.splitlines():
                if l.startswith('ROW '):
                    print(json.dumps(dict(json.loads(l[4:]), build=build, repeat=rep)), flush=True)
