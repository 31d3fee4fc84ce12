"""The care-position count of the seed filters (mimeo_amd/csrc/seed_window.h) as a stand-alone program:
tests/sanitize/seed_window_check.cc holds the header's host instantiation — the same carry-save network the kernels compile, with
64-bit shifts and a truth-table loop in the place of v_alignbit_b32 and v_bitop3_b32 — to the serial ones / twos loop it replaced,
bit for bit: the instantiations the kernels use, both `transitions` modes, every single bit, every pair of bits within 19 columns,
full and empty words, 10^6 random word pairs at five densities.  Built once plain and once under the address and
undefined-behaviour sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'sanitize', 'seed_window_check.cc')


@pytest.mark.parametrize('name,flags', [
    ('plain', ['-O2']),
    ('asan_ubsan', ['-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']),
])
def test_seed_window_matches_the_loop_it_replaced(tmp_path, name, flags):
    exe = tmp_path / ('seed_window_check_' + name)
    r = subprocess.run(['g++', '-std=c++17', '-Wall'] + flags + [SRC, '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'seed_window_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
