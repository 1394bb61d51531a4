"""The case table of tests/staging_cases.py on the CPU: what
tests/test_gpu_staging.py relies on, asserted from the references and plain
arithmetic alone -- that each case's workgroup windows reach the group steps,
ring laps and partial workgroups it was chosen for, that csrc/launch_plan.h
picks the kernel the case names, that the lanes end the way the case needs
(oracle_fast), and that oracle_fast equals the per-clock oracle_rtl at the new
shapes (shots_per_group > 1, runs that start inside a group, indices past 32
bits), where tests/test_fast_vs_rtl.py holds shots_per_group at 1."""

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, isa
from tests import staging_cases as sc
from tests.progfuzz import pack_programs
from tests.test_fast_vs_rtl import EV_CAP, HORIZON, MEAS_CAP, TR_CAP, compare
from tests.test_launch_plan import plan, run_line        # noqa: F401  (plan: the fixture)

BRANCH_LDS_MAX, PROG_LDS_MAX, STRAIGHT_LDS_MAX = 512, 1024, 9216      # csrc/uop.h


def ids(cases):
    return [c.name for c in cases]


def facts(ps):
    """csrc/program_image.h's ProgramFacts of a ProgramSet, as far as plan_run reads them"""
    op = ps.words[:, 3] >> 28
    used = np.zeros(len(op), bool)
    for o, n in zip(ps.offsets, ps.n_instr):
        used[int(o):int(o) + int(n)] = True
    op = op[used]
    straight = not ((op >= 1) & (op <= 7)).any()
    linear = not (((op >= 2) & (op <= 5)) | (op == 7)).any()
    max_len = int(ps.n_instr.max())
    tot = int((ps.n_instr.astype(np.int64) + 1).sum())
    C = ps.cores_per_shot
    group_len = [int(sum(int(ps.n_instr[p]) + 1 for p in ps.table[g * C:(g + 1) * C])) for g in range(ps.n_groups)]
    return dict(straight=int(straight), linear=int(linear), fproc=int(((op == 4) | (op == 5)).any()),
                sync=int((op == 7).any()), reg_writes=int(((op == 1) | (op == 4)).any()),
                macros=int(linear and not straight), max_len=max_len, group_len=group_len,
                cmd_major=int((max_len + 1) * ps.n_programs <= max(4 * tot, 4096)), n_programs=ps.n_programs)


def footprint(c, group_len):
    """commands of the largest staged window (guards included): launch_plan.h's w consecutive groups"""
    S = sc.BLOCK // c.C
    w = 1 if c.n_groups == 1 else (S - 1) // c.spg + 2
    if w * c.C > sc.BLOCK:
        return None
    return max(sum(group_len[(g + i) % c.n_groups] for i in range(w)) for g in range(c.n_groups))


def plan_line(c, flags=0):
    f = facts(sc.program_set(c))
    return run_line(C=c.C, n_groups=c.n_groups, n_programs=f['n_programs'], straight=f['straight'], linear=f['linear'],
                    fproc=f['fproc'], sync=f['sync'], reg_writes=f['reg_writes'], macros=f['macros'],
                    cmd_major=f['cmd_major'], nr=2, addid=0, max_len=f['max_len'], group_len=max(f['group_len']),
                    spg=c.spg, order=c.order, flags=flags, model={'state': 0, 'readout': 1, 'demod': 2}[c.model],
                    fproc_mode=int(c.mode == 'lut'), n_shots=c.n_shots)


@pytest.fixture(scope='module')
def fast():
    """oracle_fast's summary of a case, by name, computed once"""
    cache = {}

    def get(c):
        if c.name not in cache:
            ps = sc.program_set(c)
            out = oracle.fast_run(sc.config(c), ps.words, ps.offsets, ps.n_instr, ps.table, c.shot0, c.n_shots,
                                  want=('summary',), ro=sc.demod_tables(c))
            cache[c.name] = _abi.unpack_summary(out['summary'])
        return cache[c.name]
    return get


# ---------------------------------------------------------------- reach
@pytest.mark.parametrize('c', sc.ALL, ids=ids(sc.ALL))
def test_windows_reach(c):
    S = sc.BLOCK // c.C
    win = sc.windows(c)
    assert all(len(w) * c.C <= sc.BLOCK for w in win)                # no window exceeds 256 slots
    hit = {
        'three_groups': any(len(w) >= 3 for w in win),
        'wrap': any(a == c.n_groups - 1 and b == 0 for w in win for a, b in zip(w, w[1:])) and c.n_groups > 1,
        'longer_than_ring': any(len(w) > c.n_groups for w in win),
        'partial_last': c.n_shots % S != 0,
        'mid_group_start': c.shot0 % c.spg != 0 and (c.shot0 // c.spg) % c.n_groups != 0,
    }
    for r in c.reach:
        assert hit[r], (c.name, r)
    if c.family in 'AB':
        assert c.n_shots < 2000 and 2 <= len(win) <= 8           # a few workgroups
    if c.family == 'D':
        assert len(win) > 1024 and c.n_shots % S != 0       # past the fb1 threshold, last workgroup partly filled
        for k in ('event_cap', 'trace_cap'):
            assert c.caps[k] * c.n_shots * c.C * 16 <= 100e6


def test_family_a_reach():
    """between them the family-A cases reach every window shape, both lane orders, the c8 instantiation and
    two other C, every feature bit, READOUT once and DEMOD twice"""
    A = sc.FAMILY_A
    for r in ('three_groups', 'wrap', 'longer_than_ring', 'partial_last', 'mid_group_start'):
        assert any(r in c.reach for c in A if c.staged), r
    assert {c.order for c in A} == {0, 1}
    Cs = {c.C for c in A if c.staged}
    assert 8 in Cs and len(Cs) >= 3
    feats = [int(c.kernel.split('=')[1].split(',')[0].rstrip('>'), 16) for c in A]
    for bit in (0x1, 0x2, 0x4):                                     # FEAT_FPROC, FEAT_SYNC, FEAT_LUT
        assert any(f & bit and f & 0x8 for f in feats), bit
    assert sum(c.model == 'readout' for c in A) == 1 and sum(c.model == 'demod' for c in A) == 2
    over = [c for c in A if not c.staged]
    assert len(over) == 1 and not feats[A.index(over[0])] & 0x8
    for c in A:
        fp = footprint(c, facts(sc.program_set(c))['group_len'])
        if c.staged:
            assert fp is not None and fp <= BRANCH_LDS_MAX, (c.name, fp)
        else:
            assert BRANCH_LDS_MAX < fp <= BRANCH_LDS_MAX + 48, (c.name, fp)      # just over


def test_family_b_and_c_shapes():
    B = sc.FAMILY_B
    assert {c.C for c in B} == {1, 2, 8, 64}
    tight = [c for c in B if c.name in sc.B_TIGHT]
    assert len(tight) == 3 and all(c.caps['event_cap'] == 3 and c.caps['meas_cap'] == 1 for c in tight)
    assert len([c for c in B if c.name not in sc.B_TIGHT + sc.B_EDGES]) == 3
    fps = {c.name: footprint(c, facts(sc.program_set(c))['group_len']) for c in B}
    assert 4097 <= fps['b_lds_opt_in'] <= STRAIGHT_LDS_MAX and fps['b_lds_opt_in'] * 16 > 64 * 1024
    assert STRAIGHT_LDS_MAX < fps['b_past_lds_max'] <= STRAIGHT_LDS_MAX + 512
    for name in sc.B_EDGES:                             # equal-length programs: the plan tool decides exactly
        assert len(set(sc.program_set(sc.BY_NAME[name]).n_instr.tolist())) == 1
    for c in sc.FAMILY_C:
        assert c.n_shots == 700
    runs = {c.name.split('_', 2)[2]: c for c in sc.FAMILY_C}
    c = runs['straddle_2_32']
    assert c.shot0 < 2 ** 32 < c.shot0 + c.n_shots
    assert runs['above_2_40'].shot0 > 2 ** 40
    c = runs['spg_2_32']
    assert c.spg == 2 ** 32 - 16 and (c.shot0 + 99) // c.spg != (c.shot0 + 100) // c.spg
    assert c.shot0 % c.spg + 115 < 2 ** 32 <= c.shot0 % c.spg + 116
    for kind in ('pulse', 'macro', 'branch'):
        assert sum(c.name.startswith('c_' + kind) for c in sc.FAMILY_C) == 3


# ---------------------------------------------------------------- kernel names
@pytest.mark.fresh_process
def test_kernel_names(plan):
    """the plan names each case's kernel (the largest group's length as every group's: an upper bound for
    cases with unequal programs, exact for the budget-edge cases of B), PROG_LDS under X_GENERAL | X_PROG_LDS
    for family A, and prog under X_PROG_MAJOR where the case fetches rows"""
    lines = [plan_line(c) for c in sc.ALL]
    _, got = plan(lines)
    for c, g in zip(sc.ALL, got):
        name = g['name']
        if name.startswith('macro_staged_kernel'):
            # the tool is told nr = 2, addid = 0: the case's programs name 2 registers and use other ALU ops
            ps = sc.program_set(c)
            alu = ps.words[(ps.words[:, 3] >> 28 == 1) | (ps.words[:, 3] >> 28 == 6)]
            assert (((alu[:, 3] >> 24) & 7) > 1).any(), c.name
        assert name == c.kernel, (c.name, g)
        if c.staged is not None:
            assert (g['lds'] > 0) == c.staged, (c.name, g)
    A = sc.FAMILY_A
    _, got = plan([plan_line(c, _abi.X_GENERAL | _abi.X_PROG_LDS) for c in A])
    for c, g in zip(A, got):
        assert g['name'].startswith('interp_kernel<') and g['feat'] & 0x8 and 0 < g['lds'] <= PROG_LDS_MAX, (c.name, g)
    over = sc.BY_NAME['a_c8_over_512']
    _, (g,) = plan([plan_line(over)])
    assert g['cm'] == 1 and g['lds'] == 0                            # unstaged: the command-major image
    rows = [c for c in sc.ALL if c.kernel.startswith('straight_kernel<rows')]
    _, got = plan([plan_line(c, _abi.X_PROG_MAJOR) for c in rows])
    for c, g in zip(rows, got):
        assert g['name'] == c.kernel.replace('rows', 'prog'), (c.name, g)


# ---------------------------------------------------------------- the cases run what they are for
LONG = [c for c in sc.FAMILY_B] + [c for c in sc.FAMILY_D if c.name in sc.D_LONG]


@pytest.mark.parametrize('c', LONG, ids=ids(LONG))
def test_long_programs_run_long(c, fast):
    """at least half the lanes retire 64 commands and more and end DONE (the tight-cap cases too: their
    max_cycles cuts the slower lanes only)"""
    s = fast(c)
    assert ((s['n_instr'] >= 64) & (s['status'] == _abi.ST_DONE)).mean() >= 0.5, c.name


def test_tight_caps_and_endings(fast):
    hung = late = False
    for c in sc.FAMILY_B:
        s = fast(c)
        hung |= bool((s['status'] == _abi.ST_HUNG_OPCODE).any())
        late |= bool((s['flags'] & _abi.F_LATE).any())
        if c.name in sc.B_TIGHT:
            assert (s['flags'] & _abi.F_EVENT_OVF).any() and (s['flags'] & _abi.F_MEAS_OVF).any(), c.name
            cut = s['ip'][s['status'] == _abi.ST_MAX_CYCLES]
            assert len(cut), c.name
            # straight_kernel<*,fb4> fetches commands k = 1 + 4 j .. 4 + 4 j together: lanes cut at the first
            # command of a batch (at the fetch) and at the last of the batch before it
            assert (cut % 4 == 1).any() and (cut % 4 == 0).any(), (c.name, np.bincount(cut % 4))
    assert hung and late


def program_lengths(c):
    """per output lane: the commands of the lane's program"""
    ps = sc.program_set(c)
    grp = [((c.shot0 + s) // c.spg) % c.n_groups for s in range(c.n_shots)]
    lens = np.array([[int(ps.n_instr[ps.table[g * c.C + k]]) for g in grp] for k in range(c.C)])     # [core, shot]
    return (lens.T if c.order == _abi.LANES_SHOT_MAJOR else lens).reshape(-1)


def test_guards_are_retired(fast):
    """lanes end DONE on the zero guard behind their program (ip = the program's length) -- what dropping the
    guard from the staged length would change: in the open-ended cases of B (staged in LDS, and in the
    command-major image's guard row behind the longest programs), and in family A, whose jumps point past
    the end, under staging and without it"""
    seen = {}
    for c in sc.FAMILY_A + [c for c in sc.FAMILY_B if c.open_end]:
        s = fast(c)
        seen[c.name] = int(((s['status'] == _abi.ST_DONE) & (s['ip'] >= program_lengths(c))).sum())
    for c in sc.FAMILY_B:
        if c.open_end:
            assert seen[c.name] >= c.n_shots * c.C // 2, (c.name, seen)
    assert {c.name for c in sc.FAMILY_B if c.open_end} == {'b_c2_spg50_loose', 'b_past_lds_max'}
    ps = sc.program_set(sc.BY_NAME['b_past_lds_max'])
    assert (ps.n_instr == ps.n_instr.max()).all()                    # every program runs into the guard row
    assert sum(seen[c.name] > 0 for c in sc.FAMILY_A if c.staged) >= 2 and seen['a_c8_over_512'] > 0, seen


def test_family_a_endings(fast):
    st = np.concatenate([fast(c)['status'] for c in sc.FAMILY_A])
    assert (st == _abi.ST_DONE).mean() >= 0.2
    for want in (_abi.ST_DONE, _abi.ST_MAX_CYCLES, _abi.ST_DEADLOCK):
        assert (st == want).any(), want


# ---------------------------------------------------------------- oracle_fast against oracle_rtl
def fast_vs_rtl(c, fz, n_shots, shot0):
    """tests/test_fast_vs_rtl.py's run_both for a case's shots_per_group (its caps and horizon)"""
    C = c.C
    cfg = sc.config(c)
    cfg.max_cycles, cfg.event_cap, cfg.trace_cap, cfg.meas_cap = HORIZON, EV_CAP, TR_CAP, MEAS_CAP
    cfg.lane_order = _abi.LANES_CORE_MAJOR
    words, offs, ni = pack_programs(fz['progs'])
    fastr = oracle.fast_run(cfg, words, offs, ni, fz['table'], shot0, n_shots)
    scfg = oracle.shot_cfg_from_config(cfg)
    rtl = []
    for s in range(n_shots):
        g = ((shot0 + s) // c.spg) % c.n_groups
        progs = [np.asarray(isa.words_to_u32(fz['progs'][int(fz['table'][g * C + k])])) for k in range(C)]
        rtl.append(oracle.rtl_run_shot(scfg, progs, shot0 + s, HORIZON + 16, EV_CAP, TR_CAP, MEAS_CAP)[1])
    return compare(cfg, fastr, rtl, n_shots)


RTL_CASES = ['b_c2_spg50_loose', 'a_c2_ring_laps', 'c_branch_straddle_2_32', 'c_branch_above_2_40',
             'c_branch_spg_2_32']


@pytest.mark.parametrize('name', RTL_CASES)
@pytest.mark.parametrize('k', range(3))
def test_fast_vs_rtl_at_the_new_shapes(name, k):
    """a long pulse-only case, a family-A case with spg > 1 that starts inside a group, and the three index
    cases, each with three program seeds, on the handful of shots around the case's first group change"""
    c = sc.BY_NAME[name]
    fn, kw = c.gen
    kw = dict(kw, seed=kw['seed'] + 1000 * k, ncores=c.C, n_groups=c.n_groups)
    kw.setdefault('mode', c.mode)
    fz = fn(**kw)
    assert c.spg > 1 and c.shot0 % c.spg != 0
    first = c.spg - c.shot0 % c.spg                  # run shot of the first group change
    if name == 'c_branch_straddle_2_32':
        first = 2 ** 32 - c.shot0                    # ... or of shot 2^32
    st = fast_vs_rtl(c, fz, 6, c.shot0 + first - 3)
    assert st['done'] + st['other'] == 6 * c.C
