"""Host side of the tandem scorer's wide range (`--tmaxperiod` up to 2000, TRF's own range): the job list
`host_plan::tandem_jobs` (mimeo_amd/csrc/host_plan.h) under ASan + UBSan through the stand-alone program
tests/sanitize/tandem_plan.cc, and the range check of `mimeo map` / `mimeo filter`, which is an argparse error before the
engine is initialised."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, 'tests', 'sanitize', 'tandem_plan.cc')


def test_tandem_jobs_under_sanitizers(tmp_path):
    if shutil.which('g++') is None:
        pytest.skip('no g++')
    exe = tmp_path / 'tandem_plan_asan_ubsan'
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all', SRC, '-o', str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert 'tandem_plan: ok' in r.stdout
    assert 'Sanitizer' not in r.stderr and 'runtime error' not in r.stderr, r.stderr[-4000:]


def _map_args(*extra):
    from mimeo_amd import run_map
    return run_map.mainArgs(['--afasta', 'a.fa', '--bfasta', 'b.fa'] + list(extra))


def _filter_args(*extra):
    from mimeo_amd import run_filter
    return run_filter.mainArgs(['--infile', 'lib.fa'] + list(extra))


@pytest.mark.parametrize('parse', [_map_args, _filter_args])
def test_tmaxperiod_range_is_an_argparse_matter(parse, capsys):
    assert parse().tmaxperiod == 50
    assert parse('--tmaxperiod', '2000').tmaxperiod == 2000
    assert parse('--tmaxperiod', '1').tmaxperiod == 1
    for bad in ('2001', '0', '-1'):
        with pytest.raises(SystemExit) as e:
            parse('--tmaxperiod', bad)
        assert e.value.code == 2
        assert '--tmaxperiod must be in 1..2000' in capsys.readouterr().err


@pytest.mark.parametrize('parse', [_map_args, _filter_args])
def test_help_names_the_range(parse, capsys):
    with pytest.raises(SystemExit):
        parse('--help')
    text = ' '.join(capsys.readouterr().out.split())
    assert "(<= 2000, TRF's own range)" in text and '<= 64' not in text
