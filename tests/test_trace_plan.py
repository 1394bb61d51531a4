"""dpemu_feedline_traces' grid on the CPU (csrc/launch_plan.h plan_traces): the
sort of the pair table, the chunks of one (core, spc_lo) group each, their
growth once the grid would exceed the device, and the sample tiles, without a
GPU.  tests/trace_plan_test.cpp holds the checks (a stand-alone program, as
tests/qsim_plan_test.cpp is); this builds and runs it, on its own tables and
on the pair tables of tests/handbuilt.py's many_pairs cases.  ``trace_plan``
is also what tests/test_handbuilt_inputs.py reads the chunks of those cases
from."""

import os
import re
import shutil
import subprocess
import tempfile

import pytest

from tests import handbuilt as hb

HERE = os.path.dirname(os.path.abspath(__file__))
_built = {}


def driver():
    """the built driver's path (once per process)"""
    if 'exe' not in _built:
        _built['dir'] = tempfile.TemporaryDirectory(prefix='trace_plan_')
        exe = os.path.join(_built['dir'].name, 'trace_plan_test')
        subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'trace_plan_test.cpp')],
                       check=True)
        _built['exe'] = exe
    return _built['exe']


def trace_plan(core, spc_lo, n_samples_lo, ro_cpw, n_bins, bin_clocks, S, wgs_per_cu, n_cu):
    """plan_traces of a pair table through the driver (which checks it too): dict of BLOCK, TRACE_ITEMS,
    TRACE_PAIRS_PER_WG, tiles, chunks [(core, log2 spc_lo, first, end)] and perm"""
    text = '{} {} {} {} {} {} {} {}\n{}\n{}\n'.format(len(core), n_samples_lo, ro_cpw, n_bins, bin_clocks, S, wgs_per_cu,
                                                     n_cu, ' '.join(str(int(v)) for v in core),
                                                     ' '.join(str(int(v)) for v in spc_lo))
    path = os.path.join(os.path.dirname(driver()), 'table_{}.txt'.format(len(os.listdir(os.path.dirname(driver())))))
    with open(path, 'w') as f:
        f.write(text)
    r = subprocess.run([driver(), path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    lines = [ln.split() for ln in r.stdout.splitlines()]
    const = [int(v) for v in lines[0][1:]]
    assert lines[0][0] == 'const' and lines[1][0] == 'tiles' and lines[-1][0] == 'perm'
    return dict(BLOCK=const[0], TRACE_ITEMS=const[1], TRACE_PAIRS_PER_WG=const[2], tiles=int(lines[1][1]),
                chunks=[tuple(int(v) for v in ln[1:]) for ln in lines[2:-1]], perm=[int(v) for v in lines[-1][1:]])


def case_plan(name, n_bins=300, bin_clocks=1, S=1, wgs_per_cu=8, n_cu=4096):
    """the plan of a hand-built case on a device that holds every chunk at once (a large ``resident``: the chunks
    are as small as plan_traces cuts them)"""
    c = hb.case(name)
    return trace_plan(c.pt.cols['core'], c.pt.cols['spc_lo'], c.n_lo, c.cfg.ro_cpw, n_bins, bin_clocks, S, wgs_per_cu,
                      n_cu)


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_trace_plan():
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    r = subprocess.run([driver()], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    m = re.fullmatch(r'ok (\d+)\n', r.stdout)
    assert m and int(m.group(1)) > 100000, r.stdout[-2000:]


@pytest.mark.fresh_process
@pytest.mark.parametrize('name', list(hb.MANY))
def test_trace_plan_of_the_many_pairs_cases(name):
    """the driver's checks on the hand-built table, and its shape: the four groups in core order, the big one cut
    at 64 -- on a device that holds them all and, by slot, on one that holds a single workgroup"""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    c = hb.case(name)
    cores = c.pt.cols['core'].tolist()
    assert cores != sorted(cores)
    pl = case_plan(name)
    assert [(ch[0], ch[3] - ch[2]) for ch in pl['chunks']] == [(0, 33), (1, 5), (2, 64), (2, 8), (3, 32)]
    assert [cores[i] for i in pl['perm']] == sorted(cores) and sorted(pl['perm']) == list(range(c.pt.n_pairs))
    assert pl['tiles'] == (min(300 * int(c.pt.cols['spc_lo'][0]), c.n_lo) + 1023) // 1024
    one = case_plan(name, S=32, wgs_per_cu=1, n_cu=1)
    assert [(ch[0], ch[3] - ch[2]) for ch in one['chunks']] == [(0, 33), (1, 5), (2, 72), (3, 32)]
