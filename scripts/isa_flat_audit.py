#!/usr/bin/env python3
"""flat_* / global_* / scratch_* accesses per kernel in the gfx950 assembly of the extension, chain and gapped kernels.

    python scripts/isa_flat_audit.py [file.hip ...]      (default: the files below; needs hipcc, no GPU)

A pointer that a kernel loads from a device table (the StrandView / IndexView members of UnitDesc, FusedUnit, Group) is a
generic pointer to the compiler, and every access through it is a flat_* instruction: it may address LDS, so it is not
moved across LDS stores, is waited for on vmcnt and lgkmcnt together, and is issued to both memory paths.  The kernels
hold such pointers in global address space (gptr<T>, mimeo_amd/csrc/device_util.h); this script is the guard that keeps
it so.  It compiles device code only (hipcc -S --cuda-device-only with the Makefile's flags), prints the counts per
kernel and exits non-zero when a kernel outside ALLOW has a flat_* access.
"""
import collections
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'mimeo_amd', 'csrc')
FILES = ['k34_fused.hip', 'k4_extend.hip', 'k5_chain.hip', 'k5_wave.hip', 'k6_gapped.hip', 'k6_dp.hip', 'k6_trace.hip', 'k6_paths.hip', 'k9_path_stats.hip', 'k10_window_stats.hip', 'k11_path_text.hip', 'k12_link_regions.hip', 'k17_terminal.hip', 'k18_flank.hip', 'k19_frames.hip']
FLAGS = ['-O3', '-std=c++17', '--offload-arch=gfx950', '-ffp-contract=off', '-w', '-S', '--cuda-device-only']
# kernels (name without template arguments) that may keep flat_* accesses, each with its reason
ALLOW = {
    'k6_trace': 'the score ring is in LDS for a narrow band and in the device pool for a wide one: one pointer, really either',
}


def hipcc():
    return os.environ.get('HIPCC') or shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def demangle(names):
    filt = shutil.which('llvm-cxxfilt') or shutil.which('c++filt') or next(
        (p for p in ('/opt/rocm/lib/llvm/bin/llvm-cxxfilt', '/opt/rocm/llvm/bin/llvm-cxxfilt') if os.path.exists(p)), None)
    if not filt or not names:
        return {n: n for n in names}
    out = subprocess.run([filt], input='\n'.join(names), capture_output=True, text=True).stdout.split('\n')
    return {n: (out[i].strip() if i < len(out) and out[i].strip() else n) for i, n in enumerate(names)}


def audit_asm(text):
    """{mangled name of a kernel or out-of-line device function: its flat / global / scratch access counts} of one assembly file"""
    kernels = set(re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M))
    res, cur = {}, None
    for line in text.split('\n'):
        m = re.match(r'^([A-Za-z_$][\w$.]*):', line)
        if m:   # a kernel or a device function that was not inlined (block labels start with a dot)
            cur = m.group(1)
            res[cur] = {'flat': 0, 'global': 0, 'scratch': 0, 'flat_ops': collections.Counter(), 'kernel': cur in kernels}
            continue
        if line.startswith('.Lfunc_end'):
            cur = None
            continue
        if cur is None:
            continue
        s = line.strip()
        if not s or s[0] in ';.':
            continue
        op = s.split()[0]
        for kind in ('flat', 'global', 'scratch'):
            if op.startswith(kind + '_'):
                res[cur][kind] += 1
                if kind == 'flat':
                    res[cur]['flat_ops'][op] += 1
    return {k: r for k, r in res.items() if r['kernel'] or r['flat'] or r['global'] or r['scratch']}


def audit(files=FILES, out=sys.stdout):
    cc = hipcc()
    if not cc:
        raise RuntimeError('hipcc not found')
    bad = []
    with tempfile.TemporaryDirectory() as td:
        procs = []
        for f in files:
            asm = os.path.join(td, os.path.basename(f) + '.s')
            procs.append((f, asm, subprocess.Popen([cc] + FLAGS + ['-o', asm, os.path.join(CSRC, f)], stderr=subprocess.PIPE, text=True)))
        for f, asm, p in procs:
            err = p.communicate()[1]
            if p.returncode:
                raise RuntimeError('%s does not compile:\n%s' % (f, err[-2000:]))
            res = audit_asm(open(asm).read())
            names = demangle(sorted(res))
            print('%s' % f, file=out)
            print('  %6s %6s %7s  kernel' % ('flat', 'global', 'scratch'), file=out)
            for k in sorted(res, key=lambda k: names[k]):
                r, name = res[k], re.sub(r'\(.*$', '', names[k]).replace('void ', '').replace('mimeo::', '')
                why = ALLOW.get(re.sub(r'<.*$', '', name))
                mark = ''
                if r['flat']:
                    mark = '   allowed: ' + why if why else '   <-- ' + ', '.join('%s x%d' % kv for kv in sorted(r['flat_ops'].items()))
                    if not why:
                        bad.append((f, name, r['flat']))
                print('  %6d %6d %7d  %s%s' % (r['flat'], r['global'], r['scratch'], name, mark), file=out)
    return bad


def main():
    files = [os.path.basename(a) for a in sys.argv[1:]] or FILES
    bad = audit(files)
    if bad:
        print('\nflat_* accesses outside the allow-list (a pointer read from a device table reaches memory as a generic pointer: '
              'hold it as gptr<T>, device_util.h):', file=sys.stderr)
        for f, name, n in bad:
            print('  %s: %s (%d)' % (f, name, n), file=sys.stderr)
        return 1
    print('\nno flat_* access outside the allow-list')
    return 0


if __name__ == '__main__':
    sys.exit(main())
