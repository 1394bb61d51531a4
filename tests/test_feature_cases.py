"""tests/feature_cases.py's INSTANTIATIONS on the CPU: every row plans exactly
the branch_kernel / interp_kernel instantiation it claims (the plan of
csrc/launch_plan.h over the image of csrc/program_image.h, run by
tests/instantiation_plan_test.cpp), the rows are exactly the instantiations
libdpemu.so holds, and every row's programs reach the code its feature bits
switch (oracle_fast alone, so that seeds can be chosen without a GPU).
tests/test_gpu_instantiations.py then runs every row on the device."""

import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from distributed_processor_amd import _abi, isa
from tests import feature_cases as fc
from tests.feature_cases import INSTANTIATIONS, SEED_A, SEED_B
from tests.test_kernel_resources import LLVM, code_objects, kernel_meta  # noqa: F401  (code_objects: a fixture)
from tests.test_program_image import case_words

HERE = os.path.dirname(os.path.abspath(__file__))
IDS = [fc.row_id(r) for r in INSTANTIATIONS]
XS = (0, fc.FEAT_FPROC, fc.FEAT_SYNC, fc.FEAT_FPROC | fc.FEAT_SYNC, fc.FEAT_LUT, fc.FEAT_LUT | fc.FEAT_SYNC)


def expected_instantiations():
    """what the dispatch tables of branch.hip, branch_demod.hip, branch_states.hip and interp.hip list"""
    want = {('branch', m | x | r | l, ct) for m in (0, fc.FEAT_DEMOD, fc.FEAT_STATES) for x in XS
            for r in (0, fc.FEAT_REGS) for l in (0, fc.FEAT_PROG_LDS) for ct in (0, 8)}
    want |= {('interp', x | l) for x in XS for l in (0, fc.FEAT_PROG_LDS)}
    want |= {('interp', fc.FEAT_STRAIGHT), ('interp', fc.FEAT_STRAIGHT | fc.FEAT_PROG_LDS)}
    return want


# ---- the shape of the table ----

def test_table_covers_every_instantiation_once():
    got = [fc.instantiation(r) for r in INSTANTIATIONS]
    assert len(got) == len(set(got)) == 158
    assert set(got) == expected_instantiations()


def test_table_shapes():
    by_c, orders, globals_ = set(), set(), {}
    for r in INSTANTIATIONS:
        lanes = r.n_shots * r.C
        assert 257 <= lanes <= 511 and lanes % 64, fc.row_id(r)         # two workgroups, a partly filled last wave
        assert r.n_groups >= 2 and r.shots_per_group < 256 // r.C, fc.row_id(r)     # a workgroup spans > 1 group
        assert (r.C == 8) == r.c8 or r.family == 'interp', fc.row_id(r)
        # the groups a workgroup can span have at most 256 programs: the staging rule looks at their length alone
        assert ((256 // r.C - 1) // r.shots_per_group + 2) * r.C <= 256, fc.row_id(r)
        assert not r.feat & fc.FEAT_SYNC or r.C >= 2, fc.row_id(r)
        if r.family == 'branch':
            assert not r.exec_flags & ~_abi.X_PROG_MAJOR, fc.row_id(r)
            if not r.c8:
                by_c.add(r.C)
            if not r.feat & fc.FEAT_PROG_LDS:
                globals_.setdefault(r.model, set()).add(bool(r.exec_flags & _abi.X_PROG_MAJOR))
        else:
            want = _abi.X_GENERAL | (_abi.X_PROG_LDS if r.feat & fc.FEAT_PROG_LDS else 0)
            assert r.exec_flags == want and r.model == 'state', fc.row_id(r)
        orders.add(r.order)
    assert by_c == {1, 2, 4, 16} and orders == {fc.CM, fc.SM}
    # both reasons for a global fetch, in every model: kept global by the flag, and too long to stage
    assert globals_ == {m: {True, False} for m in ('state', 'demod', 'states')}


# ---- (a) the plan ----

MODEL = {'state': _abi.MEAS_STATE, 'demod': _abi.MEAS_DEMOD, 'states': _abi.MEAS_STATE}


def plan_case(r):
    ps = fc.programs_of_row(r)
    parts = case_words(r.C, ps.n_groups, ps.words, ps.offsets, ps.n_instr, ps.table)
    fproc_mode = _abi.FPROC_LUT if r.feat & fc.FEAT_LUT else _abi.FPROC_MEAS
    parts[0] = np.concatenate([parts[0], np.array([r.shots_per_group, r.order, r.exec_flags, MODEL[r.model], fproc_mode,
                                                   r.n_shots], np.uint32)])
    return parts


def run_plans(tmp_path, cases):
    """-> per case (facts, plan of dpemu_run, plan of dpemu_run_states), as dicts"""
    exe = str(tmp_path / 'instantiation_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'instantiation_plan_test.cpp')],
                   check=True)
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for parts in cases:
            for a in parts:
                fh.write(np.ascontiguousarray(a, np.uint32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'OK' and lines[0].startswith('caps ') and len(lines) == 3 * len(cases) + 2, r.stdout[-2000:]
    rows = [(ln.split()[0], {k: (v if k == 'name' else int(v)) for k, v in re.findall(r'(\w+)=(\S+)', ln)})
            for ln in lines[1:-1]]
    assert [t for t, _ in rows] == ['facts', 'off', 'on'] * len(cases)
    assert all(d['case'] == i // 3 for i, (_, d) in enumerate(rows))
    caps = dict((k, int(v)) for k, v in re.findall(r'(\w+)=(\S+)', lines[0]))
    return caps, [tuple(d for _, d in rows[3 * i:3 * i + 3]) for i in range(len(cases))]


def plan_problems(rows, plans, caps):
    """the rows whose plan is not the instantiation they claim"""
    bad = []
    for r, (facts, off, on) in zip(rows, plans):
        f = fc.program_facts(_progs_of(r))
        if tuple(bool(facts[k]) for k in fc.Facts._fields) != tuple(f):
            bad.append((fc.row_id(r), 'facts', facts, f))
        plan = on if r.model == 'states' else off
        feat = r.feat | fc.MODEL_BIT[r.model]
        want_family = caps['k_interp'] if r.family == 'interp' else caps['k_branch']
        if plan['name'] != fc.kernel_name(r) or plan['family'] != want_family or \
                plan['feat' if r.family == 'interp' else 'bfeat'] != feat:
            bad.append((fc.row_id(r), 'plan', plan['name'], fc.kernel_name(r)))
        # staged programs have their LDS words.  A row without them and without DPEMU_X_PROG_MAJOR is too long to
        # stage: test_table_shapes rules out the other reason, a workgroup that spans too many groups
        if bool(plan['lds']) != bool(r.feat & fc.FEAT_PROG_LDS):
            bad.append((fc.row_id(r), 'lds', plan['lds']))
        # dpemu_run_states of a row of another model: the same bits and the states bit, on branch_kernel
        if r.family == 'branch' and r.model == 'state' and on['bfeat'] != (off['bfeat'] | fc.FEAT_STATES):
            bad.append((fc.row_id(r), 'states plan', on['name']))
    return bad


@functools.lru_cache(maxsize=None)
def _progs_of(r):
    ps = fc.programs_of_row(r)
    return [[int(w[0]) | int(w[1]) << 32 | int(w[2]) << 64 | int(w[3]) << 96
             for w in ps.words[int(o):int(o) + int(n)]] for o, n in zip(ps.offsets, ps.n_instr)]


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_every_row_plans_the_instantiation_it_claims(tmp_path):
    caps, plans = run_plans(tmp_path, [plan_case(r) for r in INSTANTIATIONS])
    assert caps['branch'] == 512 and caps['prog'] == 1024
    assert not plan_problems(INSTANTIATIONS, plans, caps)
    # and the kernels the plans name are all of them, each once: a row moved to another feature set, whose programs
    # follow it there, leaves its own instantiation unplanned
    planned = []
    for r, (_, off, on) in zip(INSTANTIATIONS, plans):
        pl = on if r.model == 'states' else off
        planned.append(('interp', pl['feat']) if pl['family'] == caps['k_interp'] else
                       ('branch', pl['bfeat'], 8 if pl['name'].endswith(',c8>') else 0))
    assert sorted(planned) == sorted(expected_instantiations())


# ---- (b) the census ----

def test_census_can_fail():
    sym = lambda inst: ('_ZN5dpemu13branch_kernelILi{}ELi{}EEEvNS_7KParamsE'.format(*inst[1:]) if inst[0] == 'branch'
                        else '_ZN5dpemu13interp_kernelILi{}EEEvNS_7KParamsE'.format(inst[1]))
    symbols = [sym(fc.instantiation(r)) for r in INSTANTIATIONS]
    other = ['_ZN5dpemu15straight_kernelILi0ELi1EEEvNS_7KParamsE', '_ZN5dpemu12macro_kernelILi2EEEvNS_7KParamsE']
    assert fc.census(symbols + other, INSTANTIATIONS) == ([], [])
    gone = fc.instantiation(INSTANTIATIONS[5])
    assert fc.census(symbols[:5] + symbols[6:] + other, INSTANTIATIONS) == ([], [gone])
    extra = ('branch', fc.FEAT_STATES | fc.FEAT_DEMOD | 3, 8)
    assert fc.census(symbols + [sym(extra)] + other, INSTANTIATIONS) == ([extra], [])
    assert fc.census(symbols + [sym(('interp', 7))], INSTANTIATIONS[:-1]) == \
        (sorted([('interp', 7), fc.instantiation(INSTANTIATIONS[-1])]), [])


@pytest.mark.fresh_process        # runs llvm tools: before any test touches the GPU
@pytest.mark.skipif(not os.path.exists(os.path.join(LLVM, 'llvm-objdump')), reason='ROCm llvm tools not available')
def test_rows_are_exactly_the_built_instantiations(code_objects):
    symbols = [k for co in code_objects for k in kernel_meta(co)]
    no_row, not_built = fc.census(symbols, INSTANTIATIONS)
    assert not no_row, 'built without a row in INSTANTIATIONS: {}'.format(no_row)
    assert not not_built, 'rows whose kernel libdpemu.so does not hold: {}'.format(not_built)
    assert len(fc.built_instantiations(symbols)) == 158


# ---- (c) reach conditions ----

@functools.lru_cache(maxsize=None)
def oracle_pair(r):
    return fc.oracle_of_row(r, SEED_A), fc.oracle_of_row(r, SEED_B)


def lane_programs(r, ps, cfg):
    """the program of every lane"""
    shot, core = fc.lane_shots_cores(cfg, r.n_shots, fc.shot0_of(r))
    group = (shot // r.shots_per_group) % ps.n_groups
    return ps.table[group * r.C + core]


def reach_problems(r):
    """why the row does not reach what its feature bits switch (empty: it does)"""
    bad = []
    ps = fc.programs_of_row(r)
    cfg, _ = fc.config_of_row(r, ps)
    fa, fb = oracle_pair(r)
    xmeas, sync, regs = fc.requested(r)
    sa, sb = fa['summary'].reshape(-1, 8), fb['summary'].reshape(-1, 8)
    if xmeas != 'none' and not fc.paths_differ(fa, fb).any():
        bad.append('no lane takes another path under the second seed')
    if sync:
        progs = _progs_of(r)
        first_sync = np.array([min([i for i, w in enumerate(p) if isa.decode(w)['op'] == 'sync'], default=1 << 20)
                               for p in progs])
        if not ((sa[:, 1] & 0xFFFF) > first_sync[lane_programs(r, ps, cfg)]).any():
            bad.append('no lane gets past a sync')
    if regs is False and not fc.names_source_register(_progs_of(r)):
        bad.append('no command reads a register')
    if r.model == 'states':
        if max(sa[:, 5].max(), sb[:, 5].max()) > 32:
            bad.append('a lane measures more than 32 times')
        if not (sa[:, 6] != sb[:, 6]).any():
            bad.append('the second seed draws the same states')
    if not ((((sa[:, 1] >> 16) & 0xFF) == _abi.ST_DONE) & (sa[:, 2] > 0)).any():
        bad.append('no lane ends DONE with an event')
    return bad


@pytest.mark.parametrize('r', INSTANTIATIONS, ids=IDS)
def test_row_reaches_its_features(r):
    assert not reach_problems(r)


def test_table_reaches_every_status_and_flag():
    """over the table every stop status occurs, and every flag the oracle can raise: F_GUARD is the device
    interpreters' own iteration guard (an internal error), which no program asks for"""
    status, flags = set(), 0
    for r in INSTANTIATIONS:
        s = oracle_pair(r)[0]['summary'].reshape(-1, 8)
        status |= set(((s[:, 1] >> 16) & 0xFF).tolist())
        flags |= int(np.bitwise_or.reduce(s[:, 1] >> 24))
    assert status == {_abi.ST_DONE, _abi.ST_MAX_CYCLES, _abi.ST_HUNG_OPCODE, _abi.ST_DEADLOCK}
    assert flags == _abi.F_LATE | _abi.F_EVENT_OVF | _abi.F_TRACE_OVF | _abi.F_MEAS_OVF | _abi.F_DOUBLE_STROBE
