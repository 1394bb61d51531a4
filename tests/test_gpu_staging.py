"""The interpreter kernels at the launch shapes of tests/staging_cases.py, bit
for bit against oracle_fast: workgroup windows of several program groups
staged in LDS (lane.h stage_programs under branch_kernel, interp_kernel and
straight_kernel<lds,*>), pulse-only programs of 64 commands and more, the
dynamic LDS opt-in above 64 KiB and the fall-back past STRAIGHT_LDS_MAX, shot
and group indices past 32 bits, and grids of more than 1,024 workgroups (the
fb1 variants).  Every output array is compared, every execution variant of
test_gpu_parity.run_pair (test_gpu_demod.run_pair for DEMOD) against the base
run, and the kernel name the run reports against the case's.  That each case
reaches what it names is asserted without a GPU in tests/test_staging_cases.py
(which also pins oracle_fast to oracle_rtl at these shapes)."""

import os

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi
from distributed_processor_amd.emulator import Emulator, alloc_device_outputs
from tests import staging_cases as sc
from tests import test_gpu_demod as demod
from tests.test_gpu_parity import ALL_OUT, compare_all, run_pair

pytestmark = pytest.mark.gpu

THREADS = int(os.environ.get('OMP_NUM_THREADS', '0') or 0) or min(16, os.cpu_count() or 1)


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def ids(cases):
    return [c.name for c in cases]


def feat_bits(name):
    return int(name.split('=')[1].split(',')[0].rstrip('>'), 16)


def kernel_of(emu, c, cfg, flags=0):
    """the kernel a run of the case reports under exec_flags `flags` (the programs are loaded)"""
    base = cfg.exec_flags
    cfg.exec_flags = flags
    emu.run(c.n_shots, c.shot0, cfg=cfg, outputs=('summary',))
    cfg.exec_flags = base
    name = emu.last_kernel()
    print('{}: exec_flags {:#x} -> {}'.format(c.name, flags, name))
    return name


def check_case(emu, c):
    """GPU == oracle_fast in every output array, every execution variant == the base run, and the name"""
    ps, cfg = sc.program_set(c), sc.config(c)
    if c.model == 'demod':
        g, f = demod.run_pair(emu, ps, cfg, c.n_shots, c.shot0, sc.demod_tables(c))
        demod.compare(g, f, c.name)
    else:
        g, f = run_pair(emu, ps, cfg, c.n_shots, c.shot0)
        compare_all(g, f, c.name)
    assert kernel_of(emu, c, cfg) == c.kernel
    return cfg


@pytest.mark.parametrize('c', sc.FAMILY_A, ids=ids(sc.FAMILY_A))
def test_staged_windows_branching(emu, c):
    """family A: fuzz programs with jumps, loops, fproc reads and syncs, windows of several groups"""
    cfg = check_case(emu, c)
    assert bool(feat_bits(c.kernel) & 0x8) == c.staged
    # the general interpreter stages the same windows on request (within PROG_LDS_MAX)
    name = kernel_of(emu, c, cfg, _abi.X_GENERAL | _abi.X_PROG_LDS)
    assert name.startswith('interp_kernel<') and feat_bits(name) & 0x8, name
    if not c.staged:
        assert kernel_of(emu, c, cfg, _abi.X_PROG_MAJOR) == c.kernel      # no staging either way


@pytest.mark.parametrize('c', sc.FAMILY_B, ids=ids(sc.FAMILY_B))
def test_long_pulse_programs(emu, c):
    """family B: pulse-only programs of 64 to 1,200 commands"""
    cfg = check_case(emu, c)
    if not c.staged:
        assert kernel_of(emu, c, cfg, _abi.X_PROG_MAJOR) == 'straight_kernel<prog,fb4>'


@pytest.mark.parametrize('c', sc.FAMILY_C, ids=ids(sc.FAMILY_C))
def test_indices_past_32_bits(emu, c):
    """family C: shot 2^32 inside the run, shots above 2^40, and shots_per_group = 2^32 - 16 (the ABI
    takes any nonzero 32-bit value) with shot_begin % spg + sl passing 2^32 inside the run"""
    check_case(emu, c)


D_VARIANTS = (_abi.X_PROG_LDS | _abi.X_HIST_REPL, _abi.X_HIST_DIRECT | _abi.X_PROG_MAJOR,
              _abi.X_GENERAL | _abi.X_PROG_LDS, _abi.X_MACRO_DIRECT, _abi.X_STREAM_EVENTS)


@pytest.mark.parametrize('c', sc.FAMILY_D, ids=ids(sc.FAMILY_D))
def test_large_grids(emu, c):
    """family D: more than 1,024 workgroups, the last one partly filled; the base run against oracle_fast
    (on the job's threads), the execution variants against the base run on the device"""
    import torch
    ps, cfg = sc.program_set(c), sc.config(c)
    emu.load(ps)

    def run(flags):
        out = alloc_device_outputs(cfg, c.n_shots, want=ALL_OUT)
        for t in out.values():
            t.zero_()
        cfg.exec_flags = flags
        emu.run_device(cfg, c.n_shots, c.shot0, out)
        torch.cuda.synchronize()
        cfg.exec_flags = 0
        print('{}: exec_flags {:#x} -> {}'.format(c.name, flags, emu.last_kernel()))
        return out, emu.last_kernel()

    base, name = run(0)
    assert name == c.kernel
    f = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, c.shot0, c.n_shots, threads=THREADS,
                        want=ALL_OUT)
    assert set(f) == set(base)
    for k in f:
        a = base[k].cpu().numpy().view(f[k].dtype).reshape(f[k].shape)
        if not np.array_equal(a, f[k]):
            bad = np.argwhere(a != f[k])
            raise AssertionError('{} {}: {} mismatches, first at {}'.format(c.name, k, len(bad), bad[0].tolist()))
    del f
    names = {}
    for flags in D_VARIANTS:
        out, names[flags] = run(flags)
        for k in base:
            assert torch.equal(out[k], base[k]), '{} execution variant {:#x}: {}'.format(c.name, flags, k)
        del out
    if c.kernel.startswith('straight_kernel<rows'):
        assert names[_abi.X_HIST_DIRECT | _abi.X_PROG_MAJOR] == 'straight_kernel<prog,fb1>'
