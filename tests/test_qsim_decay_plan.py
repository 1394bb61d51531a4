"""dpemu_qsim_decay's host part on the CPU (csrc/launch_plan.h plan_qsim_decay):
the decay table of an accepted request and the DPEMU_E_INVALID conditions
include/dpemu.h lists for the decay argument, without a GPU.
tests/qsim_decay_plan_test.cpp holds the checks (a stand-alone program, as
tests/qsim_plan_test.cpp is); this builds and runs it."""

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_qsim_decay_plan(tmp_path):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'qsim_decay_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'qsim_decay_plan_test.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    m = re.fullmatch(r'ok (\d+)\n', r.stdout)
    assert m and int(m.group(1)) > 1000, r.stdout[-2000:]
