"""plan_run's `states` argument (csrc/launch_plan.h) on the CPU: the plan of a
dpemu_run_states call.  With states every program -- pulse-only, branch-free
with registers (the macro kernels' rows) and branching -- runs on branch_kernel
with feature bit 0x80, whatever the exec_flags that pick other families; the
workgroup's programs are staged in LDS by branch.hip's BRANCH_LDS_MAX rule;
without states the plan is the four-argument call's, field for field.
tests/run_states_plan_test.cpp prints the three plans of every request line;
the assertions are here."""

import os
import re
import shutil
import subprocess

import pytest

from distributed_processor_amd import _abi
from tests.test_launch_plan import run_line

HERE = os.path.dirname(os.path.abspath(__file__))
FEAT_FPROC, FEAT_SYNC, FEAT_LUT, FEAT_PROG_LDS, FEAT_REGS, FEAT_DEMOD, FEAT_STATES = 1, 2, 4, 8, 32, 64, 128


@pytest.fixture(scope='module')
def plans(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    d = tmp_path_factory.mktemp('states_plan')
    exe = str(d / 'run_states_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'run_states_plan_test.cpp')],
                   check=True)

    def ask(lines):
        path = str(d / 'requests.txt')
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        out = []
        for ln in r.stdout.strip().splitlines():
            out.append((ln.split()[0], {k: (v if k == 'name' else int(v)) for k, v in re.findall(r'(\w+)=(\S+)', ln)}))
        assert len(out) == 3 * len(lines) + 1, r.stdout[-2000:]
        assert [t for t, _ in out[1:]] == ['four', 'off', 'on'] * len(lines)
        rows = [x for _, x in out[1:]]
        return out[0][1], [tuple(rows[3 * i:3 * i + 3]) for i in range(len(lines))]
    return ask


# the program-facts rows: (keyword arguments of run_line, the feature bits the programs themselves ask for)
ROWS = [
    (dict(straight=1, reg_writes=0, macros=0), 0),                                 # pulse-only
    (dict(straight=1, reg_writes=0, macros=0, max_len=65536, cmd_major=0), 0),    # ... whose ip could wrap
    (dict(), FEAT_REGS),                                                            # branch-free with registers (macro)
    (dict(nr=16, addid=1), FEAT_REGS),
    (dict(linear=0, macros=0, reg_writes=0), 0),                                    # jumps only
    (dict(linear=0, macros=0, fproc=1), FEAT_FPROC | FEAT_REGS),
    (dict(linear=0, macros=0, fproc=1, fproc_mode=1), FEAT_LUT | FEAT_REGS),
    (dict(linear=0, macros=0, fproc=1, sync=1, reg_writes=0), FEAT_FPROC | FEAT_SYNC),
    (dict(linear=0, macros=0, fproc=1, sync=1, fproc_mode=1), FEAT_LUT | FEAT_SYNC | FEAT_REGS),
    (dict(linear=0, macros=0, sync=1), FEAT_SYNC | FEAT_REGS),
]
FLAGS = [0, _abi.X_GENERAL, _abi.X_PROG_LDS, _abi.X_MACRO_DIRECT, _abi.X_GENERAL | _abi.X_PROG_LDS | _abi.X_MACRO_DIRECT,
         _abi.X_PROG_MAJOR, _abi.X_PROG_MAJOR | _abi.X_GENERAL, _abi.X_STREAM_EVENTS]


def grid():
    lines, want = [], []
    for kw, feat in ROWS:
        for flags in FLAGS:
            for C in (1, 2, 8, 16):
                for max_len in (() if 'max_len' in kw else (20, 40, 300, 2000)) or (kw['max_len'],):
                    for order in (0, 1):
                        k = dict(kw, C=C, flags=flags, max_len=max_len, order=order, hist=1)
                        lines.append(run_line(**k))
                        want.append((feat, flags, C, C * (max_len + 1)))
    return lines, want


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_states_plan_is_branch_kernel_with_the_states_bit(plans):
    lines, want = grid()
    caps, got = plans(lines)
    assert caps['feat_states'] == FEAT_STATES == 0x80 and caps['feat_prog_lds'] == FEAT_PROG_LDS
    assert caps['branch'] == 512
    seen_lds = set()
    for ln, (four, off, on), (feat, flags, C, footprint) in zip(lines, got, want):
        assert on['family'] == caps['k_branch'], (ln, on)
        # one group: the workgroup's footprint is the group's commands, each program with its guard
        staged = footprint <= caps['branch'] and not flags & _abi.X_PROG_MAJOR
        bfeat = feat | FEAT_STATES | (FEAT_PROG_LDS if staged else 0)
        assert on['bfeat'] == bfeat and on['bfeat'] & 0x80, (ln, on)
        assert on['name'] == 'branch_kernel<feat=0x{:x}{}>'.format(bfeat, ',c8' if C == 8 else ''), (ln, on)
        if staged:
            assert on['lds'] % 16 == 0 and max(16, footprint) <= on['lds'] <= caps['branch'], (ln, on)
        else:
            assert on['lds'] == 0, (ln, on)
        seen_lds.add((staged, footprint > caps['branch']))
        # the histogram: as for any K_BRANCH run (the reduce launch, never the folded one), and the
        # replica / direct choice that the same request makes without states
        assert on['fold'] == 0, (ln, on)
        for k in ('repl', 'R', 'stride', 'hist_lds', 'bins'):
            assert on[k] == four[k], (ln, k, on, four)
        assert on['rep_words'] == on['R'] * on['stride'], (ln, on)
    assert seen_lds == {(True, False), (False, False), (False, True)}   # staged, kept global by the flag, too long


@pytest.mark.fresh_process
def test_without_states_the_plan_is_the_four_argument_calls(plans):
    lines, _ = grid()
    lines += [run_line(model=2), run_line(model=2, straight=1, reg_writes=0, macros=0),
              run_line(C=2, n_groups=96, spg=10, addid=1, n_shots=960, hist=1),
              run_line(straight=1, reg_writes=0, macros=0, max_len=200, hist=1, n_shots=10 ** 6)]
    _, got = plans(lines)
    families = set()
    for ln, (four, off, on) in zip(lines, got):
        assert off == four, (ln, off, four)
        assert not off['bfeat'] & 0x80, (ln, off)
        families.add(four['family'])
    assert families == {0, 1, 2, 3}             # the grid plans every family without states


@pytest.mark.fresh_process
def test_states_plan_over_groups_and_sizes(plans):
    """more than one program group per workgroup: the staging decision is the plain branch plan's"""
    lines = []
    for ng, spg in ((4, 3), (32, 10), (1000, 1)):
        for max_len in (5, 30, 200):
            for C in (2, 8):
                lines.append(run_line(C=C, n_groups=ng, spg=spg, linear=0, macros=0, fproc=1, sync=1, max_len=max_len,
                                      n_shots=777, hist=1))
    caps, got = plans(lines)
    staged = set()
    for ln, (four, off, on) in zip(lines, got):
        assert four['family'] == on['family'] == caps['k_branch'], (ln, four, on)
        assert on['bfeat'] == four['bfeat'] | 0x80 and on['lds'] == four['lds'] and on['cm'] == four['cm'], (ln, four, on)
        staged.add(bool(on['bfeat'] & FEAT_PROG_LDS))
    assert staged == {True, False}
