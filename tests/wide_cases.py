"""Shots of 16, 32 and 64 cores whose cores talk to each other: the case table
of the cross-core phases of branch_kernel<FEAT, 0> and interp_kernel (sync
barriers, fproc_meas reads of another lane, the meas_lut FSM) above 16 cores,
where csrc/branch_kernel.h leaves DPP for __shfl_xor steps, csrc/lane.h
group_bits has its C >= 64 case, and sync_mask / lut_table are 64-bit words
shifted by the core index.

Random programs cannot reach this: with 32 or 64 independently drawn programs
some core always strays and the shot deadlocks.  The programs here come from
progfuzz.wide_case, which writes a shot core by core from one plan.

ROWS is the one table.  tests/test_wide_cases.py pins oracle_fast to the
per-clock oracle_rtl on every row, checks on the CPU that every row reaches
what it is there for (oracle_fast and the plan alone, so that seeds can be
chosen without a GPU), that the rows plan the kernel they claim and that the
table covers the axes below; tests/test_gpu_wide.py runs every row on the
device against oracle_fast.

Axes: C in 16, 32, 64; the fproc back end; sync_mask kinds ('all': 0; 'holes':
a hole below 16 and one in the top 16-lane row; 'b63': bit 63 set and bit 31
clear; 'high': only bits at or above 32); lut_mask kinds ('std': 0x00010101,
at C = 16 its 16 low bits, since bit 16 names no core there; 'ends':
0x80000001; 'never': a mask that names a core that never measures);
the measurement model (STATE, READOUT, DEMOD with per-core axes and random
per-program frequency tables, supplied states through dpemu_run_states); the
kernel family and the staging of the programs; the lane order.  Shapes: 257 to
511 lanes, two workgroups, several program groups, shots_per_group below the
shots of a workgroup; C = 64: 5 or 7 shots; C = 32: an odd count in 9..15 (the
last wave holds one shot beside 32 invalid lanes); C = 16: 17..31 shots, no
multiple of 4.  No row has a histogram (C > 12).

Staged rows are `short`: the LDS staging holds 512 (branch_kernel) or 1024
(interp_kernel, on request) commands of the three groups a workgroup can span,
which at 16 cores leaves 9 and at 32 cores (interp_kernel only) 9 commands per
program; at 64 cores nothing with two syncs fits, so no 64-core row is staged.

Seeds: the first of the row's own range (1000 * its index + 0..99) that meets the
reach conditions of tests/test_wide_cases.py; for DEMOD rows the seed also draws
the model parameters (demod_setup)."""

import collections
import functools
import random

import numpy as np

from distributed_processor_amd import _abi
from distributed_processor_amd.emulator import ProgramSet
from tests import feature_cases as fc
from tests.progfuzz import wide_case

CM, SM = _abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR
XG, XL, XM = _abi.X_GENERAL, _abi.X_PROG_LDS, _abi.X_PROG_MAJOR
SEED_A, SEED_B = fc.SEED_A, fc.SEED_B
ROUNDS = 3

# C, backend: 'meas' | 'lut'; model: 'state' | 'readout' | 'demod' | 'states'; family: 'branch' | 'interp';
# exec_flags; order; n_groups, shots_per_group, n_shots; sync: the sync_mask kind; lut: the lut_mask kind (None under
# 'meas'); variant: None | 'skip' (a core of each 16-lane row leaves out a barrier: the other participants end in
# DEADLOCK at the last one) | 'short' (7- to 9-command programs that are staged in LDS); seed
Row = collections.namedtuple('Row', 'C backend model family exec_flags order n_groups shots_per_group n_shots sync lut '
                             'variant seed')

ROWS = [
    # ---- 16 cores ----
    Row(16, 'meas', 'state', 'branch', 0, CM, 3, 5, 19, 'all', None, None, 0),
    Row(16, 'meas', 'readout', 'branch', XM, SM, 2, 7, 23, 'holes', None, None, 1000),
    Row(16, 'meas', 'demod', 'branch', 0, SM, 3, 6, 21, 'all', None, None, 2001),
    Row(16, 'meas', 'states', 'branch', 0, CM, 4, 3, 29, 'holes', None, None, 3000),
    Row(16, 'meas', 'state', 'branch', 0, SM, 3, 8, 17, 'all', None, 'short', 4000),
    Row(16, 'meas', 'demod', 'branch', 0, CM, 3, 9, 22, 'all', None, 'short', 5001),
    Row(16, 'meas', 'state', 'branch', XM, CM, 2, 9, 31, 'all', None, 'skip', 6047),
    Row(16, 'meas', 'state', 'interp', XG, SM, 3, 5, 18, 'holes', None, None, 7000),
    Row(16, 'meas', 'readout', 'interp', XG | XL, CM, 3, 10, 27, 'all', None, 'short', 8000),
    Row(16, 'lut', 'state', 'branch', 0, SM, 3, 5, 19, 'all', 'std', None, 9000),
    Row(16, 'lut', 'readout', 'branch', XM, CM, 2, 7, 26, 'holes', 'std', None, 10002),
    Row(16, 'lut', 'demod', 'branch', 0, CM, 3, 4, 21, 'all', 'std', None, 11010),
    Row(16, 'lut', 'states', 'branch', 0, SM, 4, 3, 30, 'all', 'std', None, 12000),
    Row(16, 'lut', 'state', 'branch', 0, CM, 2, 5, 17, 'all', 'never', None, 13000),
    Row(16, 'lut', 'state', 'interp', XG, CM, 3, 5, 23, 'all', 'std', None, 14000),
    Row(16, 'lut', 'readout', 'interp', XG | XL, SM, 2, 9, 25, 'holes', 'std', None, 15001),
    # ---- 32 cores ----
    Row(32, 'meas', 'state', 'branch', 0, CM, 3, 2, 9, 'all', None, None, 16000),
    Row(32, 'meas', 'readout', 'branch', XM, SM, 2, 3, 11, 'holes', None, None, 17000),
    Row(32, 'meas', 'demod', 'branch', 0, SM, 3, 2, 13, 'all', None, None, 18001),
    Row(32, 'meas', 'states', 'branch', 0, SM, 4, 1, 15, 'holes', None, None, 19000),
    Row(32, 'meas', 'state', 'branch', 0, SM, 2, 5, 13, 'all', None, 'skip', 20005),
    Row(32, 'meas', 'state', 'interp', XG, CM, 3, 3, 11, 'holes', None, None, 21000),
    Row(32, 'meas', 'state', 'interp', XG | XL, SM, 3, 4, 9, 'all', None, 'short', 22000),
    Row(32, 'meas', 'readout', 'interp', XG | XL, CM, 3, 5, 15, 'all', None, 'short', 23000),
    Row(32, 'lut', 'state', 'branch', 0, SM, 3, 2, 11, 'all', 'std', None, 24001),
    Row(32, 'lut', 'state', 'branch', XM, CM, 2, 3, 13, 'all', 'ends', None, 25000),
    Row(32, 'lut', 'readout', 'branch', 0, SM, 2, 5, 9, 'holes', 'ends', None, 26000),
    Row(32, 'lut', 'demod', 'branch', 0, CM, 3, 2, 15, 'all', 'std', None, 27009),
    Row(32, 'lut', 'states', 'branch', XM, CM, 4, 1, 11, 'all', 'ends', None, 28000),
    Row(32, 'lut', 'state', 'branch', 0, SM, 2, 3, 9, 'all', 'never', None, 29000),
    Row(32, 'lut', 'state', 'interp', XG, SM, 3, 2, 13, 'all', 'ends', None, 30000),
    Row(32, 'lut', 'readout', 'interp', XG | XL, CM, 2, 3, 11, 'holes', 'std', None, 31010),
    # ---- 64 cores ----
    Row(64, 'meas', 'state', 'branch', 0, CM, 3, 1, 5, 'all', None, None, 32000),
    Row(64, 'meas', 'readout', 'branch', XM, SM, 2, 2, 7, 'holes', None, None, 33000),
    Row(64, 'meas', 'demod', 'branch', 0, SM, 3, 1, 7, 'b63', None, None, 34000),
    Row(64, 'meas', 'states', 'branch', 0, SM, 2, 3, 5, 'b63', None, None, 35000),
    Row(64, 'meas', 'state', 'branch', 0, CM, 2, 2, 7, 'high', None, None, 36000),
    Row(64, 'meas', 'state', 'branch', XM, SM, 2, 1, 5, 'all', None, 'skip', 37003),
    Row(64, 'meas', 'state', 'interp', XG, SM, 3, 2, 7, 'b63', None, None, 38000),
    Row(64, 'meas', 'readout', 'interp', XG | XL, CM, 2, 1, 5, 'high', None, None, 39000),
    Row(64, 'lut', 'state', 'branch', 0, SM, 3, 1, 7, 'all', 'std', None, 40015),
    Row(64, 'lut', 'readout', 'branch', XM, CM, 2, 2, 5, 'holes', 'ends', None, 41000),
    Row(64, 'lut', 'demod', 'branch', 0, SM, 2, 3, 7, 'all', 'ends', None, 42013),
    Row(64, 'lut', 'states', 'branch', 0, CM, 3, 1, 5, 'b63', 'std', None, 43002),
    Row(64, 'lut', 'state', 'branch', 0, CM, 2, 2, 7, 'all', 'never', None, 44000),
    Row(64, 'lut', 'state', 'interp', XG, CM, 3, 1, 5, 'b63', 'std', None, 45021),
    Row(64, 'lut', 'readout', 'interp', XG | XL, SM, 2, 2, 7, 'all', 'ends', None, 46000),
]


def row_id(r):
    return 'c{}-{}-{}-{}-x{:x}-{}-{}{}{}'.format(r.C, r.backend, r.model, r.family, r.exec_flags, 'sm' if r.order else 'cm',
                                                r.sync, '-' + r.lut if r.lut else '', '-' + r.variant if r.variant else '')


def built_to_deadlock(r):
    """rows in which more than a quarter of the lanes may end other than DONE: the LUT never fires, a core leaves
    out a barrier, or half the cores sit outside sync_mask"""
    return r.lut == 'never' or r.variant == 'skip' or r.sync == 'high'


def sync_mask_of(r):
    C = r.C
    full = (1 << C) - 1
    if r.sync == 'all':
        return 0
    if r.sync == 'holes':           # a hole below 16, a hole in the top 16-lane row
        return full & ~(1 << 5) & ~(1 << (C - 3))
    if r.sync == 'b63':             # bit 63 set, bit 31 clear (and a hole below 16)
        return full & ~(1 << 31) & ~(1 << 9)
    if r.sync == 'high':            # only bits at or above 32
        return full & ~0xFFFFFFFF
    raise ValueError(r.sync)


QUIET = {16: (13,), 32: (13, 29), 64: (13, 29, 45)}     # cores that never strobe a readout, none of them in a mask


def lut_mask_of(r):
    if r.lut is None:
        return _abi.make_config(1).lut_mask
    if r.lut == 'std':
        return 0x00010101 & ((1 << r.C) - 1)
    if r.lut == 'ends':
        return 0x80000001
    if r.lut == 'never':            # core 13 never measures
        return 0x00010101 & ((1 << r.C) - 1) | (1 << 13)
    raise ValueError(r.lut)


def lut_table_of(r):
    rng = random.Random(r.seed ^ 0x7AB1E)
    return [rng.getrandbits(64) for _ in range(256)]


def meas_latency_of(r):
    return 14 + r.seed % 13 if r.backend == 'lut' else 1 + r.seed % 23     # (wide_case: a LUT stretch needs 14)


def p1_of(r):
    """per core, with 1.0 and 0.0 at cores 6 and 7 of every eight: 22 and 23, 30 and 31, 62 and 63"""
    return [(0.5, 0.3, 0.8, 0.05, 0.95, 0.6, 1.0, 0.0)[c % 8] for c in range(r.C)]


def demod_setup(r, n_programs):
    """a DEMOD row's model parameters (per-core axes for all C cores) and per-program frequency tables, drawn as
    tests/test_gpu_demod.py draws them; a delay that leaves the return inside the window"""
    from tests.test_fast_vs_rtl import demod_params
    from tests.test_gpu_demod import random_tables
    rng = random.Random(r.seed + 70000)
    meas_elem = r.seed % 4
    d = demod_params(rng, r.C, meas_elem)
    assert len(d['axis']) == r.C
    return meas_elem, d, random_tables(rng, n_programs)


RO_WORDS = 2        # the envelope length field of the readout strobes: the DEMOD window is RO_WORDS * ro_cpw clocks


@functools.lru_cache(maxsize=None)
def case_of_row(r):
    """-> (wide_case's dict, ProgramSet)"""
    kw = {}
    lat = meas_latency_of(r)
    meas_elem = 2
    if r.model == 'demod':
        meas_elem, d, _ = demod_setup(r, r.n_groups * r.C)
        kw['drv_elem'] = d['drv_elem']
        lat += RO_WORDS * d['cpw']
    if r.variant == 'skip':
        kw['skip'] = {16 * i + 3 + i: 1 + (i + r.seed) % ROUNDS for i in range(r.C // 16)}
    if r.variant == 'short':
        kw.update(short=True, rounds=2)
    if r.lut == 'never':
        kw['lut_rounds'] = (ROUNDS,)
    case = wide_case(r.seed, r.C, r.n_groups, mode=r.backend, meas_elem=meas_elem, ro_words=RO_WORDS, ro_clocks=lat,
                     sync_mask=sync_mask_of(r), lut_mask=lut_mask_of(r) if r.backend == 'lut' else 0, quiet=QUIET[r.C],
                     **{'rounds': ROUNDS, **kw})
    groups = [[case['progs'][g * r.C + c] for c in range(r.C)] for g in range(r.n_groups)]
    return case, ProgramSet(groups, cores_per_shot=r.C)


def config_of_row(r, seed=SEED_A, **over):
    """-> (config, DEMOD frequency tables or None)"""
    case, ps = case_of_row(r)
    kw, tables = {}, None
    lat = meas_latency_of(r)
    if r.model == 'demod':
        kw['meas_elem'], kw['demod'], tables = demod_setup(r, ps.n_programs)
    elif r.model == 'readout':
        # the amplitude words are uniform in [0, 2^16): s = sep A >> 16 spans [0, 3000) against a noise sigma of
        # 0.02 * 37838 = 757, so readouts on both sides of the threshold are common
        kw['readout'] = dict(sep=3000, sigma=0.02, thr=0)
    kw.update(sync_mask=sync_mask_of(r), lut_mask=lut_mask_of(r), lut_table=lut_table_of(r))
    kw.update(over)
    cfg = _abi.make_config(r.C, n_groups=r.n_groups, shots_per_group=r.shots_per_group, max_cycles=6000, event_cap=64,
                           trace_cap=48, meas_cap=8, fproc_mode=_abi.FPROC_LUT if r.backend == 'lut' else _abi.FPROC_MEAS,
                           meas_latency=lat, sync_latency=1 + r.seed % 3, seed=seed, p1=p1_of(r), lane_order=r.order,
                           exec_flags=r.exec_flags, **kw)
    return cfg, tables


def shot0_of(r):
    return (r.seed * 37 + 11) % 100000


def outs_of(cfg):
    return fc.outs_of(cfg)


@functools.lru_cache(maxsize=None)
def oracle_of_row(r, seed=SEED_A, n_shots=None, shot0=None):
    import oracle
    _, ps = case_of_row(r)
    cfg, tables = config_of_row(r, seed)
    return oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, shot0_of(r) if shot0 is None else shot0,
                           n_shots or r.n_shots, want=outs_of(cfg), ro=tables)


def staged(r):
    return r.variant == 'short'


def kernel_name(r):
    """dpemu_last_kernel's name of the kernel the row is there for"""
    case, _ = case_of_row(r)
    facts = fc.program_facts(case['progs'])
    assert facts.has_fproc and facts.has_sync
    feat = (fc.FEAT_LUT if r.backend == 'lut' else fc.FEAT_FPROC) | fc.FEAT_SYNC | (fc.FEAT_PROG_LDS if staged(r) else 0)
    if r.family == 'interp':
        return 'interp_kernel<feat=0x{:x}>'.format(feat)
    feat |= (fc.FEAT_REGS if facts.reg_writes else 0) | {'demod': fc.FEAT_DEMOD, 'states': fc.FEAT_STATES}.get(r.model, 0)
    return 'branch_kernel<feat=0x{:x}>'.format(feat)


PLANTED = (0x80000000, 0x55555555, 0, 0xFFFFFFFF)


def planted_states(r):
    """seed B's draws as words, and at cores at or above 16 (any core at C = 16) one of PLANTED wherever it agrees
    with the draws on the bits the lane reads (readout m reads bit m; a lane without readouts reads none); -> (words,
    the planted values in use)"""
    cfg_b, _ = config_of_row(r, SEED_B)
    shot0 = shot0_of(r)
    want = oracle_of_row(r, SEED_B)
    states = fc.drawn_states(cfg_b, r.n_shots, shot0, 32)
    n_meas = want['summary'].reshape(-1, 8)[:, 5].astype(np.int64)
    assert n_meas.max() <= 31
    _, core = fc.lane_shots_cores(cfg_b, r.n_shots, shot0)
    low = ((np.uint64(1) << n_meas.astype(np.uint64)) - np.uint64(1)).astype(np.uint32)
    used = set()
    for L in np.flatnonzero(core >= (16 if r.C > 16 else 0)):
        for k in range(4):
            w = PLANTED[(L + k) % 4]
            if (int(states[L]) ^ w) & int(low[L]) == 0 and int(states[L]) != w:
                states[L] = w
                used.add(w)
                break
    return states, used
