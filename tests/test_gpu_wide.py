"""Shots of 16, 32 and 64 cores on the GPU: every row of tests/wide_cases.py
against oracle_fast, bit for bit, on the kernel the row is there for.

The rows' programs (progfuzz.wide_case) release barriers whose last arrival
sits in each 16-lane row in turn, read fproc_meas across 16-lane rows and the
32-lane half with ids that wrap at C, and run the meas_lut FSM under masks and
table bits up to 31 and 63; tests/test_wide_cases.py checks all that on the
CPU, and pins oracle_fast to the per-clock model on every row.  Here:

* every row: summary, events, trace, meas, regs (and acc under DEMOD) equal the
  oracle's, dpemu_last_kernel is the row's kernel, and the execution variants
  of tests/test_gpu_demod.py::run_pair give the same arrays.  Supplied-states
  rows run by draw equivalence (tests/test_gpu_run_states.py), with the words
  0, 0xFFFFFFFF, 0x80000000 and 0x55555555 planted at cores at or above 16
  wherever they agree with the draws on the bits the lane reads;
* one row per C in two shards with global shot offsets, the boundary inside
  what was one wave;
* the sync_mask / lut_mask words with bits at or above C of include/dpemu.h."""

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi
from distributed_processor_amd.emulator import Emulator, ProgramSet
from tests import feature_cases as fc
from tests import progfuzz
from tests import wide_cases as wc
from tests.wide_cases import ROWS, SEED_A, SEED_B

pytestmark = pytest.mark.gpu

IDS = [wc.row_id(r) for r in ROWS]
VARIANTS = (_abi.X_GENERAL | _abi.X_PROG_LDS, _abi.X_PROG_MAJOR | _abi.X_HIST_DIRECT, _abi.X_PROG_LDS)


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def load(emu, r):
    _, ps = wc.case_of_row(r)
    cfg, tables = wc.config_of_row(r, SEED_A)
    if emu.programs is not ps:
        emu.load(ps)
    if tables is not None:
        emu.load_readout_freqs(cfg.ro_drv_elem, cfg.meas_elem, tables=tables)
    return ps, cfg


@pytest.mark.parametrize('r', ROWS, ids=IDS)
def test_row_equals_the_oracle(emu, r):
    ps, cfg = load(emu, r)
    outs, shot0 = wc.outs_of(cfg), wc.shot0_of(r)
    states = None
    if r.model == 'states':
        want = wc.oracle_of_row(r, SEED_B)
        states, used = wc.planted_states(r)
        assert used == set(wc.PLANTED), [hex(w) for w in used]
    else:
        want = wc.oracle_of_row(r, SEED_A)
    assert set(want) == set(outs) and 'hist' not in outs and ('acc' in outs) == (r.model == 'demod')
    got = fc.device_run(emu, ps, cfg, r.n_shots, shot0, states, outs)
    assert emu.last_kernel() == wc.kernel_name(r)
    fc.compare(got, want, wc.row_id(r))
    if r.model == 'states':
        return                          # dpemu_run_states plans branch_kernel whatever the flags
    for flags in VARIANTS:
        cfg.exec_flags = flags
        fc.compare(fc.device_run(emu, ps, cfg, r.n_shots, shot0, None, outs), got, 'execution variant {:#x}'.format(flags))


def _row(C, backend, model, order):
    return next(r for r in ROWS if (r.C, r.backend, r.model, r.order, r.variant) == (C, backend, model, order, None))


# (row, shots of the first shard): shot-major, a wave holds 4 shots of 16 cores and 2 of 32: the boundary falls inside
# one; a shot of 64 cores is a wave, and the shards' last workgroups are partly filled
SHARDS = [(_row(16, 'lut', 'state', wc.SM), 6), (_row(32, 'meas', 'demod', wc.SM), 5), (_row(64, 'lut', 'state', wc.SM), 3),
          (_row(32, 'lut', 'state', wc.CM), 7)]


@pytest.mark.parametrize('r,first', SHARDS, ids=[wc.row_id(r) for r, _ in SHARDS])
def test_shards_equal_the_unsharded_run(emu, r, first):
    ps, cfg = load(emu, r)
    outs, shot0 = wc.outs_of(cfg), wc.shot0_of(r)
    assert 0 < first < r.n_shots and (r.order == wc.CM or (first * r.C) % 64 or r.C == 64)
    whole = fc.device_run(emu, ps, cfg, r.n_shots, shot0, None, outs)
    fc.compare(whole, wc.oracle_of_row(r, SEED_A), wc.row_id(r))
    parts = [fc.device_run(emu, ps, cfg, n, s0, None, outs) for s0, n in ((shot0, first), (shot0 + first, r.n_shots - first))]
    for k in outs:
        lane_axis = 0 if k == 'summary' else 1
        per = [_abi.by_shot(p[k], r.C, axis=lane_axis, lane_order=r.order) for p in parts]       # (..., core, shot, ...)
        got = np.concatenate(per, axis=lane_axis + 1)
        np.testing.assert_array_equal(got, _abi.by_shot(whole[k], r.C, axis=lane_axis, lane_order=r.order), err_msg=k)


# ---- mask bits that name no core (include/dpemu.h; tests/test_wide_cases.py holds the two oracles to the rule) ----

def mask_cases(C, mode):
    cases = [progfuzz.random_case((60000 if mode == 'meas' else 61000) + 100 * C + seed, ncores=C, mode=mode,
                                  allow_late=False, allow_hang=False) for seed in range(10)]
    if mode == 'lut':
        return cases + [progfuzz.wide_case(79, C, 2, mode='lut', ro_clocks=20, lut_mask=(0x0101 if C == 16 else 3),
                                           quiet=(C - 1,))]
    return cases + [progfuzz.wide_case(77, C, 2, ro_clocks=20)]


@pytest.mark.parametrize('C,kw', [(4, dict(sync_mask=0b10111)), (4, dict(sync_mask=0b11111)), (16, dict(sync_mask=0x1FFFF)),
                                  (16, dict(sync_mask=0x1FF7F)), (4, dict(sync_mask=0b110000)), (16, dict(sync_mask=0x30000)),
                                  (4, dict(fproc_mode=_abi.FPROC_LUT, lut_mask=0b10011)),
                                  (16, dict(fproc_mode=_abi.FPROC_LUT, lut_mask=0x10101))],
                         ids=['c4-sync-0b10111', 'c4-sync-0b11111', 'c16-sync-all-and-bit16', 'c16-sync-hole-and-bit16',
                              'c4-sync-none-below-C', 'c16-sync-none-below-C', 'c4-lut-bit4', 'c16-lut-bit16'])
def test_mask_bits_at_or_above_C(emu, C, kw):
    n_shots = 37
    outs = ('summary', 'events', 'trace', 'meas', 'regs')
    n_wide = 0
    for i, case in enumerate(mask_cases(C, 'lut' if 'lut_mask' in kw else 'meas')):
        groups = [[case['progs'][case['table'][g * C + c]] for c in range(C)] for g in range(case['n_groups'])]
        ps = ProgramSet(groups, cores_per_shot=C)
        cfg = _abi.make_config(C, n_groups=ps.n_groups, shots_per_group=3, max_cycles=6000, event_cap=64, trace_cap=32,
                               meas_cap=8, meas_latency=20, sync_latency=1 + i % 3, seed=SEED_A, lane_order=i % 2, **kw)
        want = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, 100 * i, n_shots, want=outs)
        got = fc.device_run(emu, ps, cfg, n_shots, 100 * i, None, outs)
        name = emu.last_kernel()
        if 'plan' in case:              # the wide case always holds sync and fproc: branch_kernel with both bits
            assert name.startswith('branch_kernel<feat=0x'), name
            feat = int(name.split('feat=0x')[1].split(',')[0].rstrip('>'), 16)
            want_bits = fc.FEAT_SYNC | (fc.FEAT_LUT if 'lut_mask' in kw else fc.FEAT_FPROC)
            assert feat & (fc.FEAT_SYNC | fc.FEAT_LUT | fc.FEAT_FPROC) == want_bits and ',c8' not in name, name
            n_wide += 1
        else:
            assert name.startswith(('branch_kernel<', 'macro', 'straight_kernel<')), name
        fc.compare(got, want, 'case {}'.format(i))
    assert n_wide == 1
