"""ctypes binding of the box-versus-path study oracle (oracle/box_vs_path.c: the CPU oracle plus a gapped stage with a
traceback), the specification of the path anchor rule (mimeo_params.anchor_rule = MIMEO_ANCHOR_PATH).  Built on first
use the way scripts/box_vs_path.py builds it (`make -C oracle study`)."""
import ctypes as C
import os
import subprocess

import numpy as np

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, 'oracle', '_build', 'libmimeo_oracle_study.so')
_lib = None


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB):
            subprocess.check_call(['make', '-s', '-C', os.path.join(ROOT, 'oracle'), 'study'])
        _lib = C.CDLL(LIB)
        _lib.orc_align_pair_rule.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.POINTER(O.Params), C.c_int,
                                             C.POINTER(C.c_void_p), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        _lib.orc_align_pair_rule.restype = C.c_int
        _lib.orc_free.argtypes = [C.c_void_p]
    return _lib


def align_rule(T, Q, rule, **params):
    """One `lastz T Q` run under the box (rule 0: must equal oracle.align_pair) or the path rule (1): records as O.ALN."""
    T, Q = bytes(T), bytes(Q)
    p = O.default_params(**params)
    ptr, n = C.c_void_p(), C.c_uint64()
    counts = (C.c_uint64 * 4)()
    rc = lib().orc_align_pair_rule(T, len(T), Q, len(Q), C.byref(p), int(rule), C.byref(ptr), C.byref(n), counts)
    assert rc == 0
    k = int(n.value)
    out = np.zeros(0, O.ALN)
    if k:
        out = np.frombuffer((C.c_char * (k * O.ALN.itemsize)).from_address(ptr.value), dtype=O.ALN, count=k).copy()
    if ptr.value:
        lib().orc_free(ptr)
    return out
