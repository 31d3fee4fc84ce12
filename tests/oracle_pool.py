"""Oracle jobs on a thread pool, and the per-unit comparison, for the GPU tests that check large units against the C oracle.

The oracle is single-threaded C behind ctypes, which releases the GIL for the whole call, so threads of one process run
its calls side by side (bench.cpu_oracle_times relies on the same).  `start` returns at once: a test can hand the oracle
its sample first and drive the GPU while it runs.  Results come back in job order, whatever order the jobs finish in.
Not a conftest.py: tests import it."""
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# the columns compared with the oracle (test_gpu_segments.ACOLS)
ACOLS = ['tstart', 'tend', 'qstart', 'qend', 'score', 'id_n', 'id_d', 'qstrand']


class Pending:
    """Jobs running on a pool of their own; `results()` waits for all of them and shuts the pool down."""

    def __init__(self, jobs, cap):
        jobs = list(jobs)
        if cap < 1:
            raise ValueError('cap must be at least 1')
        self._ex = ThreadPoolExecutor(max(1, min(cap, len(jobs))))
        self._futs = [self._ex.submit(fn, *args) for fn, *args in jobs]

    def results(self):
        try:
            return [f.result() for f in self._futs]
        finally:
            self._ex.shutdown(wait=True, cancel_futures=True)


def start(jobs, cap):
    """jobs: [(fn, *args)]; at most `cap` of them run at once."""
    return Pending(jobs, cap)


def run(jobs, cap):
    """start(jobs, cap).results(): the jobs' return values in job order."""
    return start(jobs, cap).results()


_load = threading.Lock()


def align_unit(T, Q, minus, **params):
    """An oracle job: lastz(target T, query Q) on one strand (minus 0 / 1), T and Q ASCII bases (uint8 arrays or bytes;
    copied here, inside the job, so that only running jobs hold copies of long scaffolds)."""
    from oracle import oracle as O
    with _load:
        O.lib()
    return O.align_pair(bytes(T), bytes(Q), O.default_params(strand=2 if minus else 1, **params))


def _table(recs):
    """records as an int64 matrix of the ACOLS columns, rows in lexicographic order"""
    m = np.stack([np.asarray(recs[c], dtype=np.int64) for c in ACOLS], axis=1) if recs.size else np.zeros((0, len(ACOLS)), np.int64)
    return m[np.lexsort(m.T[::-1])] if m.shape[0] else m


def assert_unit_matches(got, exp, tid, qid, minus, tag=None):
    """The engine's records of the unit (tid, qid, strand) among `got` (the records of a whole call: tid / qid are scaffold
    indexes) equal `exp`, the oracle's records of lastz(target tid, query qid) run on that strand alone (strand = 1 plus,
    2 minus): the same rows on every column of ACOLS.  Returns the number of rows."""
    exp = np.asarray(exp)
    assert (exp['qstrand'] == minus).all(), (tag, 'the oracle ran another strand')
    sel = (got['tid'] == tid) & (got['qid'] == qid) & (got['qstrand'] == minus)
    a, b = _table(got[sel]), _table(exp)
    assert a.shape == b.shape, (tag, (tid, qid, minus), 'rows', a.shape[0], b.shape[0])
    bad = np.flatnonzero((a != b).any(axis=1))
    assert bad.size == 0, (tag, (tid, qid, minus), 'first differing rows (engine, oracle)', ACOLS, a[bad[:3]].tolist(), b[bad[:3]].tolist())
    return int(a.shape[0])
