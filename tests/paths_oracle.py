"""ctypes binding of tests/paths_oracle.c: the paths of the alignments of one `lastz T Q` run under the box rule or the path
rule, what mimeo_align_units_paths is checked against.  PARITY UNPINNED.  Built on first use into tests/_build/ with the
flags of oracle/Makefile, like tests/bounded_oracle.py."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle as O

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, 'paths_oracle.c')
LIB = os.path.join(HERE, '_build', 'libmimeo_oracle_paths.so')
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
        _lib.orc_align_pair_paths.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(O.Params), C.c_int, vpp, u64p,
                                              vpp, u64p, vpp, u64p]
        _lib.orc_align_pair_paths.restype = C.c_int
        _lib.orc_params_default.argtypes = [C.POINTER(O.Params)]
        _lib.orc_free.argtypes = [C.c_void_p]
    return _lib


def _take(ptr, n, dtype):
    out = np.zeros(0, dtype)
    if n and ptr.value:
        out = np.frombuffer((C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr.value), dtype=dtype, count=n).copy()
    if ptr.value:
        lib().orc_free(ptr)
    return out


def align_paths(T, Q, path_rule=0, **params):
    """(records as O.ALN, [(minus, at, aq, score, keys)]): the second lists every EXTENDED alignment, above the threshold or
    not, in rank order per strand; keys = t << 32 | q of its diagonal steps, strand coordinates, in walk order (the layout
    of bounded_oracle.align_bounded(paths=True))."""
    T, Q = bytes(T), bytes(Q)
    p = O.Params()
    lib().orc_params_default(C.byref(p))
    for k, v in params.items():
        setattr(p, k, v)
    ptr, n = C.c_void_p(), C.c_uint64()
    kp, mp, nk, nm = C.c_void_p(), C.c_void_p(), C.c_uint64(), C.c_uint64()
    rc = lib().orc_align_pair_paths(T, len(T), Q, len(Q), C.byref(p), int(path_rule), C.byref(ptr), C.byref(n), C.byref(kp), C.byref(nk),
                                    C.byref(mp), C.byref(nm))
    assert rc == 0
    recs = _take(ptr, int(n.value), O.ALN)
    keys = _take(kp, int(nk.value), np.uint64)
    meta = _take(mp, int(nm.value) * 6, np.uint64).reshape(-1, 6)
    return recs, [(int(m[0]), int(m[1]), int(m[2]), int(np.int64(m[5])), keys[int(m[3]):int(m[3] + m[4])]) for m in meta]


def blocks_to_keys(blocks):
    """gap-free blocks (t, q, len) -> the sorted keys t << 32 | q of their diagonal steps"""
    if len(blocks) == 0:
        return np.zeros(0, np.uint64)
    t = np.concatenate([np.arange(int(b['t']), int(b['t']) + int(b['len']), dtype=np.uint64) for b in blocks])
    q = np.concatenate([np.arange(int(b['q']), int(b['q']) + int(b['len']), dtype=np.uint64) for b in blocks])
    return np.sort(t << np.uint64(32) | q)
