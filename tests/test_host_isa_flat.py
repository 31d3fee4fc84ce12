"""No flat_* memory access in the extension, chain and gapped kernels (scripts/isa_flat_audit.py): a pointer that a
kernel reads out of a device table (UnitDesc, FusedUnit, Group) has to reach memory in global address space (gptr<T>,
mimeo_amd/csrc/device_util.h), or every access through it is a flat instruction that the compiler keeps in order with
the LDS traffic around it.  Needs hipcc (device code is compiled to assembly, about a minute), no GPU."""
import importlib.util
import io
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _audit():
    spec = importlib.util.spec_from_file_location('isa_flat_audit', os.path.join(ROOT, 'scripts', 'isa_flat_audit.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


ASM = '''
	.protected	_Z3fooPKi
_Z3fooPKi:
; %bb.0:
	global_load_dword v1, v0, s[0:1]
.LBB0_1:                                ; =>This Inner Loop Header: Depth=1
	flat_load_dwordx4 v[2:5], v[6:7]
	; flat_load_dword in a comment does not count
	s_waitcnt vmcnt(0) lgkmcnt(0)
	scratch_load_dword v1, off, off
	global_store_dword v0, v1, s[0:1]
	s_endpgm
.Lfunc_end0:
	.amdhsa_kernel _Z3fooPKi
	.end_amdhsa_kernel
_Z3barv:
	flat_store_dword v[0:1], v2
	s_setpc_b64 s[30:31]
.Lfunc_end1:
'''


def test_the_audit_counts_accesses_per_function():
    res = _audit().audit_asm(ASM)
    foo, bar = res['_Z3fooPKi'], res['_Z3barv']
    assert (foo['flat'], foo['global'], foo['scratch'], foo['kernel']) == (1, 2, 1, True)
    assert dict(foo['flat_ops']) == {'flat_load_dwordx4': 1}
    assert (bar['flat'], bar['global'], bar['scratch'], bar['kernel']) == (1, 0, 0, False)   # an out-of-line device function counts too


def test_no_flat_access_in_the_extension_chain_and_gapped_kernels():
    A = _audit()
    if A.hipcc() is None:
        pytest.skip('no hipcc')
    out = io.StringIO()
    bad = A.audit(A.FILES, out=out)
    print(out.getvalue())
    assert not bad, 'flat_* accesses outside the allow-list of scripts/isa_flat_audit.py: %s\n%s' % (bad, out.getvalue())
    # the allow-list stays short, and every entry names a kernel that exists and still needs it
    assert len(A.ALLOW) <= 2
    for name in A.ALLOW:
        rows = [l for l in out.getvalue().split('\n') if len(l.split()) > 3 and l.split()[3].split('<')[0] == name]
        assert rows and all('allowed:' in l for l in rows), 'stale allow-list entry: %s' % name
