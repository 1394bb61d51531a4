"""csrc/macro.hip's wave-uniform fast paths on full-range programs, bit for bit
against oracle_fast: the cases of tests/macro_cases.py, whose runs leave the
register trace off (trace_cap = 0, or the `trace` output not requested), so
lean_chunk_ok, lean_ok and simple_ok are not false at their first term as they
are in every other fuzz run of the macro kernels.  All 8 ALU ops with register
and 32-bit immediate in0, env / phase / freq / amp register-sourced pulse
fields, measurements and cap overflows counted inside lean chunks, late
triggers beside running lanes, partly valid and empty waves, breakers that make
one chunk MIXED, and a stride-1 sweep of max_cycles across the values at which
the lean-chunk bound and the per-macro tests change their verdict.  Every
output array is compared, every execution variant of test_gpu_parity.run_pair
against the base run, and the kernel name the run reports against the case's.
That each case reaches the path it names is asserted without a GPU in
tests/test_macro_cases.py."""

import time

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi
from distributed_processor_amd.emulator import Emulator
from tests import macro_cases as mc
from tests.test_gpu_parity import compare_all, run_pair

pytestmark = pytest.mark.gpu

H_VARIANTS = (_abi.X_MACRO_DIRECT, _abi.X_STREAM_EVENTS, _abi.X_MACRO_DIRECT | _abi.X_STREAM_EVENTS,
              _abi.X_GENERAL | _abi.X_PROG_LDS)


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def ids(cases):
    return [c.name for c in cases]


def kernel_of(emu, c, cfg, flags=0):
    base = cfg.exec_flags
    cfg.exec_flags = flags
    emu.run(c.n_shots, c.shot0, cfg=cfg, outputs=c.outputs)
    cfg.exec_flags = base
    name = emu.last_kernel()
    print('{}: exec_flags {:#x} -> {}'.format(c.name, flags, name))
    return name


def check_case(emu, c):
    """GPU == oracle_fast in every output the case asks for, every execution variant == the base run,
    and the exact kernel name (the per-lane fetch under X_MACRO_DIRECT)"""
    ps, cfg = mc.program_set(c), mc.config(c)
    g, f = run_pair(emu, ps, cfg, c.n_shots, c.shot0, outputs=c.outputs)
    assert ('trace' in g) == c.trace_on
    compare_all(g, f, c.name)
    assert kernel_of(emu, c, cfg) == c.kernel
    assert kernel_of(emu, c, cfg, _abi.X_MACRO_DIRECT) == 'macro_kernel'
    return g


@pytest.mark.parametrize('c', mc.FAMILY_F, ids=ids(mc.FAMILY_F))
def test_simple_programs(emu, c):
    """family F: every macro but the first and the last MACRO_SIMPLE, equal macro counts: the lean chunk
    (2 registers) or the simple macro (3) in every wave; with the trace requested (f_trace_on_*) the
    same programs on the slot paths, every output but `trace` equal to the trace-off run's"""
    g = check_case(emu, c)
    twin = mc.TRACE_TWINS.get(c.name)
    if twin:
        t = mc.BY_NAME[twin]
        assert not t.trace_on and (t.n_shots, t.shot0, t.gen) == (c.n_shots, c.shot0, c.gen)
        emu.load(mc.program_set(t))
        off = emu.run(t.n_shots, t.shot0, cfg=mc.config(t), outputs=t.outputs).arrays
        s_on, s_off = g['summary'].copy(), off['summary'].copy()
        ovf = _abi.unpack_summary(s_on)['n_trace'] > c.caps['trace_cap']
        assert ovf.any()
        s_on[:, 1] &= np.uint32(~(_abi.F_TRACE_OVF << 24) & 0xFFFFFFFF)     # raised only under trace_cap > 0
        assert (s_off[:, 1] >> 24 & _abi.F_TRACE_OVF == 0).all()
        compare_all(dict(g, summary=s_on), dict(off, summary=s_off), c.name + ' trace on / off')


@pytest.mark.parametrize('c', mc.FAMILY_G, ids=ids(mc.FAMILY_G))
def test_mixed_programs(emu, c):
    """family G: one breaker in a wave-uniform run (the MIXED chunk macro by macro through lean_ok /
    simple_ok, lean chunks around it; after inc_qclk by a negative value the no_wrap term), and fuzzed
    sets whose waves drift between all paths as shorter programs end"""
    check_case(emu, c)


def sweep(emu, c, lo, n):
    """one run per max_cycles in [lo, lo + n), stride 1 (0.5 ms a run, the oracle's included)"""
    ps, cfg = mc.program_set(c), mc.config(c)
    emu.load(ps)
    for mcy in range(lo, lo + n):
        cfg.max_cycles = mcy
        g = emu.run(c.n_shots, c.shot0, cfg=cfg, outputs=c.outputs).arrays
        f = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, c.shot0, c.n_shots, want=c.outputs)
        compare_all(g, f, '{} max_cycles {}'.format(c.name, mcy))
    return ps, cfg


@pytest.mark.parametrize('c', mc.FAMILY_H, ids=ids(mc.FAMILY_H))
def test_max_cycles_sweep(emu, c):
    """family H: one run per max_cycles over consecutive values, each against oracle_fast in every
    output: across the lean-chunk bounds of chunks 1 and 2 of both programs (2 registers) and across
    t + SPAN of the macros around macro 30 (lean_ok / simple_ok); every execution variant at the
    bounds and their neighbours"""
    t0 = time.perf_counter()
    lo_m, n_m = mc.h_macro_window(c)
    ps, cfg = sweep(emu, c, lo_m, n_m)
    points = [lo_m + 15, lo_m + 16, lo_m + 17, lo_m + 18]
    if c.n_regs <= 2:
        lo, n = mc.h_window(c)
        sweep(emu, c, lo, n)
        flips = sorted(b for w in mc.fuzz_case(c)['progs'] for _, _, b in mc.lean_bounds(w) if b is not None)
        points = [v for b in flips for v in (b - 1, b)]
    assert len(points) >= 8 or c.n_regs > 2
    for mcy in points:
        cfg.max_cycles = mcy
        cfg.exec_flags = 0
        base = emu.run(c.n_shots, c.shot0, cfg=cfg, outputs=c.outputs).arrays
        for flags in H_VARIANTS:
            cfg.exec_flags = flags
            g2 = emu.run(c.n_shots, c.shot0, cfg=cfg, outputs=c.outputs).arrays
            compare_all(g2, base, '{} max_cycles {} execution variant {:#x}'.format(c.name, mcy, flags))
    cfg.exec_flags = 0
    assert kernel_of(emu, c, cfg) == c.kernel
    print('{}: sweep wall time {:.2f} s'.format(c.name, time.perf_counter() - t0))
