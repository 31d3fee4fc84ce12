"""The helpers of the large GPU parity tests (tests/oracle_pool.py) on the host: the per-unit comparison fails on the errors a
subtly wrong kernel would make — a record lost, a coordinate off by one, a mirror unit's rows left untransposed — and the
oracle pool keeps its concurrency cap and returns results in job order.  This is what shows that test_gpu_c4_row and
test_gpu_chromosome can fail, without running a broken kernel on the GPU."""
import threading
import time

import numpy as np
import pytest

from mimeo_amd import _ffi
from oracle import oracle as O
from tests import oracle_pool as OP


def _oracle_rows(rng, n, minus):
    """records as the oracle returns them for one (target, query) strand: tid = qid = 0"""
    e = np.zeros(n, dtype=O.ALN)
    e['tstart'] = rng.integers(0, 9_000_000, n)
    e['tend'] = e['tstart'] + rng.integers(100, 5000, n)
    e['qstart'] = rng.integers(0, 9_000_000, n)
    e['qend'] = e['qstart'] + rng.integers(100, 5000, n)
    e['score'] = rng.integers(3000, 400_000, n)
    e['id_d'] = e['tend'] - e['tstart'] + rng.integers(0, 40, n)
    e['id_n'] = e['id_d'] - rng.integers(0, 200, n)
    e['qstrand'] = minus
    return e


def _engine_rows(exp, tid, qid):
    """the same records as one call of the engine returns them, among other units' rows: scaffold indexes, engine dtype"""
    g = np.zeros(exp.size, dtype=_ffi.ALIGNMENT)
    for c in OP.ACOLS:
        g[c] = exp[c]
    g['tid'], g['qid'] = tid, qid
    return g


def _transposed(exp):
    """the rows of (q, t, +) that (t, q, +) yields: target and query swapped"""
    m = exp.copy()
    m['tstart'], m['tend'], m['qstart'], m['qend'] = exp['qstart'], exp['qend'], exp['tstart'], exp['tend']
    return m


@pytest.fixture
def case():
    """a C4-row-like call: the owned pair (0, 5) on the plus strand with its mirror unit (5, 0, +), and a minus-only unit
    (0, 7, -); `units` maps each unit to the oracle's records of it"""
    rng = np.random.default_rng(11)
    plus = _oracle_rows(rng, 7, 0)
    units = {(0, 5, 0): plus, (5, 0, 0): _transposed(plus), (0, 7, 1): _oracle_rows(rng, 5, 1)}
    got = np.concatenate([_engine_rows(e, t, q) for (t, q, _), e in units.items()])
    return got[np.random.default_rng(1).permutation(got.size)], units


def _check_all(got, units):
    return [OP.assert_unit_matches(got, exp, t, q, minus, 'case') for (t, q, minus), exp in units.items()]


def test_acols_are_the_segment_tests_columns():
    from tests import test_gpu_segments
    assert OP.ACOLS == test_gpu_segments.ACOLS


def test_matching_records_pass_in_any_order(case):
    got, units = case
    assert _check_all(got, units) == [7, 7, 5]


def test_a_dropped_record_fails(case):
    got, units = case
    k = int(np.flatnonzero((got['tid'] == 0) & (got['qid'] == 7))[2])
    with pytest.raises(AssertionError, match='rows'):
        _check_all(np.delete(got, k), units)


def test_an_extra_record_fails(case):
    got, units = case
    with pytest.raises(AssertionError, match='rows'):
        _check_all(np.concatenate([got, got[(got['tid'] == 5)][:1]]), units)


@pytest.mark.parametrize('col', OP.ACOLS[:7])
def test_one_value_off_by_one_fails(case, col):
    got, units = case
    got = got.copy()
    k = int(np.flatnonzero((got['tid'] == 0) & (got['qid'] == 5))[3])
    got[col][k] += 1
    with pytest.raises(AssertionError, match='differing'):
        _check_all(got, units)


def test_a_record_on_the_wrong_strand_fails(case):
    got, units = case
    got = got.copy()
    got['qstrand'][int(np.flatnonzero((got['tid'] == 0) & (got['qid'] == 7))[0])] = 0
    with pytest.raises(AssertionError):
        _check_all(got, units)


def test_a_mirror_unit_left_untransposed_fails(case):
    got, units = case
    got = got.copy()
    src = (got['tid'] == 0) & (got['qid'] == 5)
    mir = np.flatnonzero((got['tid'] == 5) & (got['qid'] == 0))
    assert mir.size == src.sum()
    raw = got[src].copy()
    raw['tid'], raw['qid'] = 5, 0   # the source unit's rows, relabelled but not transposed
    got[mir] = raw
    OP.assert_unit_matches(got, units[(0, 5, 0)], 0, 5, 0)
    with pytest.raises(AssertionError, match='differing'):
        OP.assert_unit_matches(got, units[(5, 0, 0)], 5, 0, 0)


def test_oracle_records_of_another_strand_fail(case):
    got, units = case
    with pytest.raises(AssertionError, match='another strand'):
        OP.assert_unit_matches(got, units[(0, 7, 1)], 0, 7, 0)


def test_pool_keeps_its_cap_and_the_job_order():
    lock, live, peak = threading.Lock(), [0], [0]

    def job(k, delay):
        with lock:
            live[0] += 1
            peak[0] = max(peak[0], live[0])
        time.sleep(delay)
        with lock:
            live[0] -= 1
        return k

    delays = [0.08, 0.01, 0.05, 0.0, 0.03, 0.02, 0.06, 0.0, 0.01]
    assert OP.run([(job, k, d) for k, d in enumerate(delays)], 3) == list(range(len(delays)))
    assert peak[0] == 3
    pending = OP.start([(job, k, 0.01) for k in range(4)], 8)
    assert pending.results() == [0, 1, 2, 3] and peak[0] <= 4
    assert OP.run([], 4) == []
    with pytest.raises(ValueError):
        OP.start([(job, 0, 0.0)], 0)


def test_pool_passes_a_jobs_exception_on():
    def bad():
        raise RuntimeError('oracle job failed')
    with pytest.raises(RuntimeError, match='oracle job failed'):
        OP.run([(time.sleep, 0.0), (bad,)], 2)
