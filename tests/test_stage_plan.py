"""The entry points' host half on the CPU (csrc/stage_plan.h): every
DPEMU_E_INVALID / DPEMU_E_NOPROG condition of dpemu_run's config, dpemu_dds,
dpemu_demod_iq, the feedline stages and dpemu_iq_stats that needs no device
pointer, their precedence, and the tables an accepted call uploads, without a
GPU.  tests/stage_plan_test.cpp holds the checks (a stand-alone program, as
tests/qsim_plan_test.cpp is); this builds and runs it."""

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_stage_plan(tmp_path):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'stage_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'stage_plan_test.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    m = re.fullmatch(r'ok (\d+)\n', r.stdout)
    assert m and int(m.group(1)) > 600, r.stdout[-2000:]
