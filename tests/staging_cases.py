"""The launch shapes at which csrc/launch_plan.h takes another kernel, another
template argument or the LDS staging of csrc/lane.h stage_programs, one case
each.  Not test code of its own: tests/test_staging_cases.py asserts on the CPU
(plain arithmetic, the plan tool of tests/test_launch_plan.py, oracle_fast)
that every case reaches the window, the kernel and the lane endings it was
chosen for; tests/test_gpu_staging.py holds the kernels to oracle_fast on the
same cases.

A case names its generator call (tests/progfuzz.py), the cores per shot C, the
program groups, shots_per_group, the run's shots and first shot, the lane
order, the caps, the fproc back end, the measurement model and the kernel name
a run of it must report (dpemu_last_kernel).

Families:
 A  programs with jumps, loops, fproc reads and syncs whose workgroup windows
    hold several program groups: branch_kernel<...PROG_LDS...> (and, on
    request, interp_kernel) stage the window in LDS
 B  pulse-only programs of 64 commands and more: straight_kernel<lds,fb4>, the
    dynamic LDS opt-in above 64 KiB and the fall-back past STRAIGHT_LDS_MAX
 C  shot and group indices past 32 bits
 D  more than 1,024 workgroups (the fb1 variants), partly filled last one

The window of workgroup b, restated here for the CPU checks: S = 256 / C
shots [b S, (b + 1) S) of the run, shot s in group ((shot0 + s) // spg) %
n_groups; the staged slots are the C programs of every group step from the
window's first shot to its last one."""

import functools
import random

from distributed_processor_amd import _abi
from distributed_processor_amd.emulator import ProgramSet
from tests.progfuzz import random_case, shaped_case

BLOCK = 256
LOOSE = dict(max_cycles=6000, event_cap=256, trace_cap=16, meas_cap=16)


def tight(max_cycles):
    return dict(max_cycles=max_cycles, event_cap=3, trace_cap=16, meas_cap=1)


class Case:
    def __init__(self, name, family, gen, C, n_groups, spg, n_shots, shot0, kernel, order=0, caps=LOOSE,
                 mode='meas', model='state', staged=None, sync_mask=0, seed=1, reach=(), open_end=False):
        self.name, self.family = name, family
        self.gen = gen                      # (generator, keyword arguments): the programs
        self.C, self.n_groups, self.spg = C, n_groups, spg
        self.n_shots, self.shot0, self.order = n_shots, shot0, order
        self.caps = dict(caps)              # max_cycles, event_cap, trace_cap, meas_cap
        self.mode, self.model = mode, model     # 'meas' / 'lut'; 'state' / 'readout' / 'demod'
        self.kernel = kernel                # the name the base run reports
        self.staged = staged                # family A: FEAT_PROG_LDS set in the name; B / D: lds > 0
        self.sync_mask, self.seed = sync_mask, seed
        self.open_end = open_end            # final done / 0000 commands dropped: the lanes run on into the zero guard
        self.reach = tuple(reach)           # what the CPU file asserts of the case's windows (test_staging_cases.py)

    def __repr__(self):
        return self.name


def _random(seed, **kw):
    return (random_case, dict(seed=seed, **kw))


def _shaped(seed, **kw):
    return (shaped_case, dict(seed=seed, **kw))


def _branchy(seed, body, **kw):
    kw.setdefault('allow_late', True)
    kw.setdefault('allow_hang', True)
    return _random(seed, body=body, late_from=kw.pop('late_from', 6), **kw)


def _pulses(seed, body=(64, 200), late_from=150):
    return _random(seed, straight=True, mode='meas', body=body, late_from=late_from)


S32, S40 = 1 << 32, 1 << 40
SPG_BIG = S32 - 16

FAMILY_A = [
    # C = 8, w = (32 - 1) / 31 + 2 = 3: the c8 instantiation; the run starts inside group 1
    Case('a_c8_spg31', 'A', _branchy(116, (5, 8)), C=8, n_groups=3, spg=31, n_shots=32 * 5 + 11, shot0=31 + 17,
         kernel='branch_kernel<feat=0x2b,c8>', staged=True, caps=dict(LOOSE, event_cap=64),
         reach=('partial_last', 'mid_group_start', 'wrap')),
    # C = 2, w = 4: windows of 3 and 4 groups that run from group 4 on to group 0; shot-major lanes; LUT
    Case('a_c2_spg50_lut', 'A', _branchy(105, (6, 12), allow_late=False, allow_hang=False), C=2, n_groups=5,
         spg=50, n_shots=128 * 4 + 37, shot0=50 * 3 + 30, order=1, mode='lut', kernel='branch_kernel<feat=0x2e>',
         staged=True, caps=dict(LOOSE, max_cycles=20000, event_cap=64),
         reach=('three_groups', 'wrap', 'partial_last', 'mid_group_start')),
    # C = 1, w = 4: one program per slot, the READOUT model
    Case('a_c1_spg100_readout', 'A', _branchy(130, (8, 16)), C=1, n_groups=4, spg=100, n_shots=256 * 3 + 90,
         shot0=100 * 2 + 45, model='readout', kernel='branch_kernel<feat=0x2b>', staged=True,
         caps=dict(LOOSE, event_cap=64), reach=('three_groups', 'wrap', 'partial_last', 'mid_group_start')),
    # C = 2, two groups, w = 8: the window laps the ring four times
    Case('a_c2_ring_laps', 'A', _branchy(124, (6, 12)), C=2, n_groups=2, spg=20, n_shots=128 * 3 + 61,
         shot0=20 * 3 + 7, order=1, kernel='branch_kernel<feat=0x2b>', staged=True, caps=dict(LOOSE, event_cap=64),
         reach=('three_groups', 'wrap', 'longer_than_ring', 'partial_last', 'mid_group_start')),
    # DEMOD, C = 4, w = 4, a partial sync mask (core 3 deadlocks at its first sync)
    Case('a_c4_demod', 'A', _branchy(129, (6, 10)), C=4, n_groups=3, spg=25, n_shots=64 * 4 + 29, shot0=25 * 2 + 11,
         model='demod', sync_mask=0b0111, kernel='branch_kernel<feat=0x6b>', staged=True,
         caps=dict(LOOSE, event_cap=64), reach=('three_groups', 'wrap', 'partial_last', 'mid_group_start')),
    # DEMOD through the LUT back end, C = 8
    Case('a_c8_demod_lut', 'A', _branchy(109, (5, 8), allow_late=False, allow_hang=False), C=8, n_groups=2,
         spg=31, n_shots=32 * 4 + 9, shot0=31 + 5, order=1, mode='lut', model='demod',
         kernel='branch_kernel<feat=0x6e,c8>', staged=True, caps=dict(LOOSE, max_cycles=20000, event_cap=64), reach=('wrap', 'partial_last', 'mid_group_start')),
    # the same window shape with a footprint just over BRANCH_LDS_MAX: unstaged, the command-major image
    Case('a_c8_over_512', 'A', _branchy(173, (6, 9)), C=8, n_groups=3, spg=31, n_shots=32 * 5 + 11, shot0=31 + 17,
         kernel='branch_kernel<feat=0x23,c8>', staged=False, caps=dict(LOOSE, event_cap=64),
         reach=('partial_last', 'mid_group_start', 'wrap')),
]

FAMILY_B = [
    Case('b_c1_loose', 'B', _pulses(201), C=1, n_groups=3, spg=100, n_shots=256 * 3 + 50, shot0=100 + 45,
         kernel='straight_kernel<lds,fb4>', staged=True, reach=('three_groups', 'wrap', 'partial_last')),
    Case('b_c2_ring_tight', 'B', _pulses(202), C=2, n_groups=2, spg=20, n_shots=128 * 3 + 61, shot0=20 * 3 + 7,
         order=1, caps=tight(960), kernel='straight_kernel<lds,fb4>', staged=True,
         reach=('three_groups', 'wrap', 'longer_than_ring', 'partial_last')),
    Case('b_c8_shaped_loose', 'B', _shaped(203, ncores=8, n_groups=3, length=100, late_from=90), C=8, n_groups=3,
         spg=31, n_shots=32 * 5 + 11, shot0=31 * 2 + 17, order=1, kernel='straight_kernel<lds,fb4>', staged=True,
         reach=('wrap', 'partial_last')),
    Case('b_c64_tight', 'B', _pulses(204, (64, 68), 64), C=64, n_groups=2, spg=4, n_shots=4 * 5 + 3, shot0=6,
         caps=tight(600), kernel='straight_kernel<lds,fb4>', staged=True, reach=('wrap', 'partial_last')),
    Case('b_c2_spg50_loose', 'B', _pulses(205), C=2, n_groups=5, spg=50, n_shots=128 * 4 + 37, shot0=50 * 3 + 30,
         order=1, kernel='straight_kernel<lds,fb4>', staged=True, open_end=True,
         reach=('three_groups', 'wrap', 'partial_last')),
    Case('b_c8_shaped_tight', 'B', _shaped(206, ncores=8, n_groups=2, length=100, late_from=100), C=8, n_groups=2,
         spg=20, n_shots=32 * 5 + 11, shot0=20 + 9, caps=tight(810), kernel='straight_kernel<lds,fb4>', staged=True,
         reach=('wrap', 'partial_last')),
    # equal-length programs at the LDS budget's edges: 8 x 601 commands need 77,056 B of dynamic LDS (the
    # opt-in above 64 KiB); 8 x 1,200 are past STRAIGHT_LDS_MAX and fetch the command-major rows, where the
    # programs (no final done: open_end) run on into the guard row
    Case('b_lds_opt_in', 'B', _shaped(207, ncores=8, n_groups=1, length=599, late_from=590), C=8, n_groups=1, spg=1,
         n_shots=32 * 3 + 5, shot0=3, caps=dict(LOOSE, max_cycles=40000, event_cap=900),
         kernel='straight_kernel<lds,fb4>', staged=True, reach=('partial_last',)),
    Case('b_past_lds_max', 'B', _shaped(208, ncores=8, n_groups=1, length=1199, late_from=1190, allow_hang=False),
         C=8, n_groups=1, spg=1, n_shots=32 * 3 + 5, shot0=3, caps=dict(LOOSE, max_cycles=80000, event_cap=64),
         kernel='straight_kernel<rows,fb4>', staged=False, open_end=True, reach=('partial_last',)),
]
B_TIGHT = ('b_c2_ring_tight', 'b_c64_tight', 'b_c8_shaped_tight')
B_EDGES = ('b_lds_opt_in', 'b_past_lds_max')


def _index_cases():
    """three program sets through (i) a run that straddles shot 2^32, (ii) shots above 2^40, (iii)
    shots_per_group = 2^32 - 16 from shot 4 spg - 100: the group changes at run shot 100 and
    shot_begin % spg + sl passes 2^32 at run shot 116 (lane.h group_q's 64-bit branch)"""
    sets = [('pulse', _random(301, straight=True, mode='meas'), 'straight_kernel<rows,fb4>', 'meas'),
            ('macro', _random(302, linear=True, mode='meas', regs=[2, 9]), 'macro_staged_kernel<2>', 'meas'),
            ('branch', _branchy(115, (6, 12)), 'branch_kernel<feat=0x2b>', 'meas')]
    runs = [('straddle_2_32', 70, S32 - 100), ('above_2_40', 50, S40 + 123456789),
            ('spg_2_32', SPG_BIG, 4 * SPG_BIG - 100)]
    out = []
    for sname, gen, kernel, mode in sets:
        for rname, spg, shot0 in runs:
            out.append(Case('c_{}_{}'.format(sname, rname), 'C', gen, C=2, n_groups=3, spg=spg, n_shots=700,
                            shot0=shot0, order=len(out) % 2, mode=mode, kernel=kernel,
                            staged=True if sname == 'branch' else None, caps=dict(LOOSE, event_cap=64)))
    return out


FAMILY_C = _index_cases()

BIG = dict(max_cycles=6000, event_cap=12, trace_cap=8, meas_cap=4)
FAMILY_D = [
    Case('d_pulse_rows', 'D', _random(401, straight=True, mode='meas'), C=2, n_groups=3, spg=7, n_shots=132013,
         shot0=12345, caps=BIG, kernel='straight_kernel<rows,fb1>', staged=False),
    Case('d_pulse_lds', 'D', _pulses(402, (64, 70), 66), C=8, n_groups=2, spg=20, n_shots=33005, shot0=29, order=1,
         caps=BIG, kernel='straight_kernel<lds,fb1>', staged=True),
    Case('d_macro', 'D', _random(403, linear=True, mode='meas', regs=[4, 11]), C=2, n_groups=9, spg=10,
         n_shots=132013, shot0=77, caps=BIG, kernel='macro_staged_kernel<2>'),
    Case('d_branch_meas', 'D', _branchy(131, (6, 10)), C=4, n_groups=3, spg=25, n_shots=66003, shot0=25 * 2 + 11,
         caps=BIG, kernel='branch_kernel<feat=0x2b>', staged=True),
    Case('d_branch_lut', 'D', _branchy(109, (5, 8), allow_late=False, allow_hang=False), C=8, n_groups=2, spg=31,
         n_shots=33007, shot0=31 + 5, order=1,
         mode='lut', caps=dict(BIG, max_cycles=20000), kernel='branch_kernel<feat=0x2e,c8>', staged=True),
]
D_LONG = ('d_pulse_lds',)

ALL = FAMILY_A + FAMILY_B + FAMILY_C + FAMILY_D
BY_NAME = {c.name: c for c in ALL}


@functools.lru_cache(maxsize=None)
def _built(name):
    c = BY_NAME[name]
    fn, kw = c.gen
    kw = dict(kw)
    if fn is random_case:
        kw.update(ncores=c.C, n_groups=c.n_groups)
        kw.setdefault('mode', c.mode)
    fz = fn(**kw)
    if c.open_end:
        fz['progs'] = [p[:-1] if (p[-1] >> 124) in (0x0, 0xA) else p for p in fz['progs']]
    assert fz['ncores'] == c.C and fz['n_groups'] == c.n_groups and fz['mode'] == c.mode, name
    groups = [[fz['progs'][fz['table'][g * c.C + k]] for k in range(c.C)] for g in range(c.n_groups)]
    return ProgramSet(groups, cores_per_shot=c.C)


def program_set(c):
    """the case's programs (tests/progfuzz.py), built once"""
    return _built(c.name)


def config(c):
    """a fresh dpemu config of the case (the DEMOD parameters from the case's own seed)"""
    kw = dict(n_groups=c.n_groups, shots_per_group=c.spg,
              fproc_mode=_abi.FPROC_LUT if c.mode == 'lut' else _abi.FPROC_MEAS,
              meas_latency=3 + c.seed % 20, sync_latency=1 + c.seed % 3, sync_mask=c.sync_mask, seed=c.seed,
              lane_order=c.order, **c.caps)
    if c.model == 'readout':
        kw['readout'] = dict(sep=25000, sigma=0.7, thr=-1500, win=40)
    if c.model == 'demod':
        from tests.test_fast_vs_rtl import demod_params
        kw['demod'] = demod_params(random.Random(c.name), c.C)
    return _abi.make_config(c.C, **kw)


def demod_tables(c):
    """the DEMOD frequency tables of the case (test_gpu_demod.random_tables), None for the other models"""
    if c.model != 'demod':
        return None
    from tests.test_gpu_demod import random_tables
    return random_tables(random.Random(c.name + ' tables'), program_set(c).n_programs)


def windows(c):
    """per workgroup of the run: the groups of its shots' group steps, first to last (the staged slots are
    these groups x C cores), from the arithmetic of the module docstring alone"""
    S = BLOCK // c.C
    out = []
    for b in range(-(-c.n_shots // S)):
        first, last = b * S, min((b + 1) * S, c.n_shots) - 1
        q0, q1 = (c.shot0 + first) // c.spg, (c.shot0 + last) // c.spg
        out.append([q % c.n_groups for q in range(q0, q1 + 1)] if c.n_groups > 1 else [0])
    return out
