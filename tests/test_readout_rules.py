"""The readout model's integer rules on the CPU (csrc/readout_rules.h: the
prepared state, the window, the ADC sample index, the noise, the return's table
index, the m_p(n) pick, the discriminator, the strobe predicate) and the pair
descriptor's word names (csrc/uop.h), against values worked out by hand from
include/dpemu.h, without a GPU.  tests/readout_rules_test.cpp holds the checks
(a stand-alone program, as tests/stage_plan_test.cpp is); this builds and runs
it."""

import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_readout_rules(tmp_path):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'readout_rules_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'readout_rules_test.cpp')], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    m = re.fullmatch(r'ok (\d+)\n', r.stdout)
    assert m and int(m.group(1)) >= 80, r.stdout[-2000:]
