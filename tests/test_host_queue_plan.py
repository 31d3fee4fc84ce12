"""The sizing policy of the extension batch (mimeo_amd/csrc/queue_plan.h: queue capacities, boosts, arena layout and growth,
budget, follower-key bits) as a stand-alone program: tests/sanitize/queue_plan_check.cc compares it with a frozen restatement
of the arithmetic ExtBatch held before and checks the properties of the layout and of the growth.  Built with the library's
-ffp-contract=off (the capacities are truncated doubles), once plain and once under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'sanitize', 'queue_plan_check.cc')


@pytest.mark.parametrize('name,flags', [
    ('plain', ['-O2', '-ffp-contract=off']),
    ('asan_ubsan', ['-O1', '-g', '-ffp-contract=off', '-fsanitize=address,undefined', '-fno-sanitize-recover=all']),
])
def test_queue_plan_matches_its_restatement(tmp_path, name, flags):
    exe = tmp_path / ('queue_plan_check_' + name)
    r = subprocess.run(['g++', '-std=c++17', '-Wall'] + flags + [SRC, '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'queue_plan_check: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]
