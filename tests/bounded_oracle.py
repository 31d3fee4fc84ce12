"""ctypes binding of tests/bounded_oracle.c, the specification of mimeo_params.bound_extensions (path anchor rule with every
gapped extension bounded by the earlier alignments of its pair and strand; alignment specification v1, rule 7).  PARITY
UNPINNED.  Built on first use into tests/_build/ with the flags of oracle/Makefile."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'bounded_oracle.c')
LIB = os.path.join(HERE, '_build', 'libmimeo_oracle_bounded.so')
CFLAGS = ['-O3', '-fPIC', '-Wall', '-Wextra', '-std=c11', '-ffp-contract=off', '-Wno-unused-function']
_lib = None


def lib():
    global _lib
    if _lib is None:
        deps = [SRC, os.path.join(HERE, '..', 'oracle', 'box_vs_path.c'), os.path.join(HERE, '..', 'oracle', 'mimeo_oracle.c')]
        if not os.path.exists(LIB) or os.path.getmtime(LIB) < max(os.path.getmtime(d) for d in deps):
            os.makedirs(os.path.dirname(LIB), exist_ok=True)
            tmp = '%s.%d.tmp' % (LIB, os.getpid())
            subprocess.check_call([os.environ.get('CC', 'gcc')] + CFLAGS + ['-shared', '-o', tmp, SRC, '-lm'])
            os.replace(tmp, LIB)
        _lib = C.CDLL(LIB)
        u64p, vpp = C.POINTER(C.c_uint64), C.POINTER(C.c_void_p)
        _lib.orc_align_pair_bounded.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(O.Params), C.c_int, vpp,
                                                u64p, u64p, vpp, u64p, vpp, u64p]
        _lib.orc_align_pair_bounded.restype = C.c_int
        _lib.orc_params_default.argtypes = [C.POINTER(O.Params)]
        _lib.orc_free.argtypes = [C.c_void_p]
    return _lib


def _params(params):
    p = O.Params()
    lib().orc_params_default(C.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    return p


def _take(ptr, n, dtype):
    out = np.zeros(0, dtype)
    if n and ptr.value:
        out = np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype=dtype, count=n).copy()
    if ptr.value:
        lib().orc_free(ptr)
    return out


def align_bounded(T, Q, bounded=1, paths=False, counts=None, **params):
    """One `lastz T Q` run under the path rule, extensions bounded (1) or not (0): records as O.ALN.  paths=True: also the
    extended alignments, [(minus, at, aq, score, keys)] in rank order per strand, keys = t << 32 | q of the diagonal steps
    (strand coordinates).  counts: a list that receives [anchors, skipped, alignments kept, live cells clipped]."""
    T, Q = bytes(T), bytes(Q)
    p = _params(params)
    ptr, n = C.c_void_p(), C.c_uint64()
    cnt = (C.c_uint64 * 4)()
    kp, mp, nk, nm = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    rc = lib().orc_align_pair_bounded(T, len(T), Q, len(Q), C.byref(p), int(bounded), C.byref(ptr), C.byref(n), cnt,
                                      C.byref(kp) if paths else None, C.byref(nk) if paths else None,
                                      C.byref(mp) if paths else None, C.byref(nm) if paths else None)
    assert rc == 0
    if counts is not None:
        counts[:] = list(cnt)
    recs = _take(ptr, int(n.value), O.ALN)
    if not paths:
        return recs
    keys = _take(kp, int(nk.value), np.uint64)
    meta = _take(mp, int(nm.value) * 6, np.uint64).reshape(-1, 6)
    return recs, [(int(m[0]), int(m[1]), int(m[2]), int(np.int64(m[5])), keys[int(m[3]):int(m[3] + m[4])]) for m in meta]


def _job(args):
    T, Q, bounded, kw = args
    return align_bounded(T, Q, bounded, **kw)


def many(jobs):
    """[(T bytes, Q bytes, bounded, oracle params)] -> [records], on a pool of fresh processes"""
    import multiprocessing as mp
    lib()   # build once, before the workers look for it
    with mp.get_context('spawn').Pool(min(8, os.cpu_count() or 1)) as pool:
        return pool.map(_job, jobs, chunksize=1)


# The flanked-array cases of tests/test_host_bounds.py and tests/test_gpu_bounds.py (mimeo_amd.synth.flanked_tandem_genome).
# Seeds picked by running this specification: bounded and unbounded path rule give different records on each of them
# (30 of the seeds 1..32 do); test_host_bounds.py asserts it case by case.
FLANKED_PAIR_SEEDS = (1, 2, 3, 5, 13, 14)
FLANKED_RC_SEED = 9          # the pair whose query is handed over reverse-complemented
FLANKED_SELF_SEED = 4        # scaffold 0 against itself
FLANKED_GENOME_SEED = 7      # the 8-scaffold genome, all 64 pairs

_COMP = np.zeros(256, np.uint8)
_COMP[list(b'ACGTN')] = list(b'TGCAN')


def revcomp(a):
    return _COMP[a][::-1].copy()


def flanked_cases():
    """(tag, T, Q, oracle params) of every flanked pair case of the two test files"""
    from mimeo_amd.synth import flanked_tandem_genome
    cases = []
    for seed in FLANKED_PAIR_SEEDS:
        _, s = flanked_tandem_genome(seed, 2)
        cases.append((('pair', seed), s[0], s[1], {}))
    _, s = flanked_tandem_genome(FLANKED_RC_SEED, 2)
    cases.append((('rc', FLANKED_RC_SEED), s[0], revcomp(s[1]), {}))
    _, s = flanked_tandem_genome(FLANKED_SELF_SEED, 1)
    # chained, a self pair has the one anchor of its main diagonal: here every HSP is an anchor
    cases.append((('self', FLANKED_SELF_SEED), s[0], s[0], {'chain': 0}))
    _, s = flanked_tandem_genome(FLANKED_PAIR_SEEDS[1], 2)
    cases.append((('ydrop 90000', FLANKED_PAIR_SEEDS[1]), s[0], s[1], {'ydrop': 90000}))   # bands beyond the register kernels
    return cases
