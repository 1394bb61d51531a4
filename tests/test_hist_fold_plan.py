"""When a run folds the histogram reduce into straight_kernel
(RunPlan::hist_fold, csrc/launch_plan.h), on the CPU: only straight-family
plans whose histogram goes through LDS-aggregated replicas, never with
DPEMU_X_HIST_DIRECT, never on the macro / branch / general kernels and never
without a histogram; the replica allocation then carries the R + 1 tickets;
and the kernel names tests/test_launch_plan.py pins are what they were,
histogram or not.  tests/hist_fold_plan_test.cpp prints the plans."""

import os
import re
import shutil
import subprocess

import pytest

from distributed_processor_amd import _abi
from tests.test_launch_plan import run_line

HERE = os.path.dirname(os.path.abspath(__file__))
STRAIGHT = dict(straight=1, reg_writes=0, macros=0)
K_STRAIGHT, K_MACRO, K_BRANCH, K_INTERP = range(4)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    d = tmp_path_factory.mktemp('fold_plan')
    exe = str(d / 'hist_fold_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'hist_fold_plan_test.cpp')],
                   check=True)

    def ask(lines):
        path = str(d / 'requests.txt')
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        out = [{k: (v if k == 'name' else int(v)) for k, v in re.findall(r'(\w+)=(\S+)', ln)}
               for ln in r.stdout.strip().splitlines()]
        assert len(out) == len(lines), r.stdout[-2000:]
        return out
    return ask


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_fold_only_for_straight_lds_replicas(plan):
    lines = []
    for C in (1, 2, 4, 8):
        for ng in (1, 2, 3, 100):
            for n_shots in (1, 257, 10 ** 6):
                for flags in (0, _abi.X_HIST_REPL, _abi.X_HIST_DIRECT):
                    for hist in (0, 1):
                        lines.append(run_line(C=C, n_groups=ng, spg=10, max_len=20, flags=flags, n_shots=n_shots,
                                              hist=hist, **STRAIGHT))
    got = plan(lines)
    folded = 0
    for ln, g in zip(lines, got):
        flags, hist = int(ln.split('|')[1].split()[2]), int(ln.split()[-1])
        assert g['family'] == K_STRAIGHT and g['name'].startswith('straight_kernel<'), (ln, g)
        assert g['fold'] == int(bool(g['repl'] and g['hist_lds'])), (ln, g)
        if not hist or flags & _abi.X_HIST_DIRECT:
            assert g['fold'] == 0 and g['repl'] == 0, (ln, g)
        rows = g['R'] * g['stride']
        assert g['words'] == rows + ((g['R'] + 1) * g['pitch'] if g['fold'] else 0), (ln, g)
        if g['fold']:
            # what the kernel's first wave relies on: R <= workgroups, and the sums of at most 64 x 64 words
            C, n_shots = int(ln.split()[1]), int(ln.split('|')[1].split()[5])
            assert 1 <= g['R'] <= min(64, -(-n_shots * C // 256)) and g['bins'] <= 64, (ln, g)
            assert g['pitch'] >= 32
        folded += g['fold']
    assert 0 < folded < len(lines)
    # config 1's shape (one core, one group, 10^6 shots) and the shapes of tests/test_gpu_hist_fold.py:
    # folded by default where a workgroup's 256 / C shots are at least 4 per bin (hist_lds)
    for C, ng, fold in ((1, 1, 1), (2, 1, 1), (2, 2, 1), (2, 3, 1), (4, 1, 1), (4, 2, 0), (4, 3, 0)):
        for n_shots in (1, 255, 256, 257, 64 * 256 + 3, 10 ** 6):
            g = plan([run_line(C=C, n_groups=ng, max_len=20, n_shots=n_shots, hist=1, **STRAIGHT)])[0]
            assert g['fold'] == fold and g['repl'] == 1 and g['bins'] == ng << C, (C, ng, n_shots, g)
    # config 2's (8 cores, 100 groups): direct atomics, no fold
    g = plan([run_line(C=8, n_groups=100, max_len=20, n_shots=10 ** 6, hist=1, **STRAIGHT)])[0]
    assert g['fold'] == 0 and g['repl'] == 0, g


@pytest.mark.fresh_process
def test_other_families_never_fold(plan):
    lines, fam = [], []
    for hist in (0, 1):
        for flags in (0, _abi.X_HIST_REPL):
            for C in (1, 2):
                lines.append(run_line(C=C, hist=hist, flags=flags, n_shots=10 ** 5))                       # macro
                fam.append(K_MACRO)
                lines.append(run_line(C=C, linear=0, macros=0, fproc=1, hist=hist, flags=flags, n_shots=10 ** 5))
                fam.append(K_BRANCH)
                lines.append(run_line(C=C, hist=hist, flags=flags | _abi.X_GENERAL, n_shots=10 ** 5))
                fam.append(K_INTERP)
                lines.append(run_line(C=C, hist=hist, flags=flags | _abi.X_GENERAL, n_shots=10 ** 5, **STRAIGHT))
                fam.append(K_INTERP)                                # pulse-only programs on the general interpreter
                lines.append(run_line(C=C, hist=hist, flags=flags, model=2, n_shots=10 ** 5, **STRAIGHT))
                fam.append(K_BRANCH)                                # ... and with the DEMOD model on branch_kernel
    got = plan(lines)
    lds_repl = 0
    for ln, f, g in zip(lines, fam, got):
        assert g['family'] == f and g['fold'] == 0, (ln, g)
        assert g['words'] == g['R'] * g['stride'], (ln, g)
        lds_repl += bool(g['repl'] and g['hist_lds'])
    assert lds_repl                     # the grid has LDS-aggregated replica plans: they keep the reduce launch


@pytest.mark.fresh_process
def test_pinned_kernel_names_unchanged(plan):
    """the names tests/test_launch_plan.py asserts, with and without a histogram"""
    cases = [
        (dict(max_len=20, **STRAIGHT), 'straight_kernel<rows,fb4>'),
        (dict(max_len=200, **STRAIGHT), 'straight_kernel<lds,fb4>'),
        (dict(max_len=200, cmd_major=0, **STRAIGHT), 'straight_kernel<lds,fb4>'),
        (dict(max_len=5000, n_shots=10 ** 6, **STRAIGHT), 'straight_kernel<rows,fb1>'),
        (dict(flags=_abi.X_GENERAL | _abi.X_PROG_LDS, max_len=30), 'interp_kernel<feat=0x8>'),
        (dict(flags=_abi.X_PROG_LDS, max_len=3000), 'interp_kernel<feat=0x0>'),
        (dict(linear=0, macros=0, fproc=1, sync=1, max_len=30, C=8), 'branch_kernel<feat=0x2b,c8>'),
        (dict(linear=0, macros=0, fproc=1, fproc_mode=1, max_len=2000), 'branch_kernel<feat=0x24>'),
        (dict(linear=0, macros=0, max_len=30, flags=_abi.X_PROG_MAJOR), 'branch_kernel<feat=0x20>'),
        (dict(C=2, n_groups=96, spg=10, addid=1, n_shots=960), 'macro_staged_kernel<2,addid>'),
        (dict(C=2, n_groups=96, spg=10, order=1, addid=1, n_shots=960), 'macro_staged_kernel<2,addid,12>'),
        (dict(C=2, n_groups=3000, spg=4, addid=1, n_shots=12000), 'macro_kernel'),
        (dict(C=2, n_groups=96, spg=10, addid=1, flags=_abi.X_MACRO_DIRECT), 'macro_kernel'),
    ]
    lines = [run_line(hist=h, **kw) for kw, _ in cases for h in (0, 1)]
    got = plan(lines)
    for i, (kw, name) in enumerate(cases):
        for h in (0, 1):
            assert got[2 * i + h]['name'] == name, (kw, h, got[2 * i + h])
