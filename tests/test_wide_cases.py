"""tests/wide_cases.py's ROWS on the CPU (tests/test_gpu_wide.py runs them on
the device):

(a) oracle_fast is pinned to the per-clock oracle_rtl on every row's programs,
    masks, tables and measurement model (run_both / compare of
    tests/test_fast_vs_rtl.py), and lanes that end in DEADLOCK are compared
    exactly: the per-clock model still waits at the same command at its
    horizon, and every event agrees;
(b) every row reaches what it is there for, by oracle_fast and the plan of
    progfuzz.wide_case alone; the plan itself is checked against the oracle
    (every read's outcome, as the plan predicts it from the measurement
    records, gives the lane's event count and the read's register);
(c) the rows plan the kernel they claim (tests/instantiation_plan_test.cpp), at
    run-time C;
(d) the table covers the axes its docstring names, so that no row can be
    deleted unnoticed;
(e) sync_mask bits at or above C are ignored, a mask with no bit below C
    leaves no participant, lut_mask bits at or above C keep the LUT from firing
    (include/dpemu.h): both oracles, at C = 4 and C = 16;
(f) the draws of random_case, shaped_case and macro_shape_case are what they
    were before wide_case joined tests/progfuzz.py."""

import functools
import hashlib
import shutil

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, isa
from tests import feature_cases as fc
from tests import progfuzz
from tests import wide_cases as wc
from tests.test_fast_vs_rtl import EV_CAP, HORIZON, MEAS_CAP, TR_CAP, compare, run_both
from tests.test_feature_cases import run_plans
from tests.test_program_image import case_words
from tests.wide_cases import ROWS, SEED_A, SEED_B

IDS = [wc.row_id(r) for r in ROWS]
RST = _abi.TRACE_QCLK_RST


def alu(op, in0, in1):
    return int(oracle.lib().oracle_alu(op, in0 & 0xFFFFFFFF, in1 & 0xFFFFFFFF))


# ---- (a) the two oracles ----

def model_kw(r, cfg, n_programs):
    kw = dict(meas_latency=cfg.meas_latency, sync_latency=cfg.sync_latency, sync_mask=cfg.sync_mask, p1=wc.p1_of(r),
              lut_mask=cfg.lut_mask, lut_table=wc.lut_table_of(r))
    if r.model == 'demod':              # the row's own frequency tables, the ones the device run loads
        kw['meas_elem'], kw['demod'], kw['tables'] = wc.demod_setup(r, n_programs)
    elif r.model == 'readout':
        kw['readout'] = dict(sep=3000, sigma=0.02, thr=0)
    return kw


def compare_deadlocks(cfg, fast, rtl, n_shots):
    """lanes that oracle_fast ends in DEADLOCK: the per-clock model still runs at its horizon, at the same command,
    and every event, trace and measurement record is the same (none can follow: the lane waits); -> their number"""
    C = cfg.cores_per_shot
    summ = _abi.unpack_summary(fast['summary'])
    n = 0
    for s in range(n_shots):
        for c in range(C):
            L, r = c * n_shots + s, rtl[s][c]
            ctx = 'shot {} core {}'.format(s, c)
            assert (r['status'] == 0) == (summ['status'][L] != _abi.ST_DONE), ctx
            if summ['status'][L] != _abi.ST_DEADLOCK:
                continue
            n += 1
            assert summ['t_end'][L] < HORIZON - 16, ctx
            assert summ['ip'][L] == r['ip'] and summ['n_instr'][L] == r['n_instr'], ctx
            assert summ['n_events'][L] == r['n_events'] and summ['n_trace'][L] == r['n_trace'], ctx
            assert summ['n_meas'][L] == r['n_meas'] and summ['meas_bits'][L] == r['meas_bits'], ctx
            np.testing.assert_array_equal(fast['events'][:min(int(summ['n_events'][L]), EV_CAP), L], r['events'], err_msg=ctx)
            np.testing.assert_array_equal(fast['trace'][:min(int(summ['n_trace'][L]), TR_CAP), L], r['trace'], err_msg=ctx)
            np.testing.assert_array_equal(fast['meas'][:min(int(summ['n_meas'][L]), MEAS_CAP), L], r['meas'], err_msg=ctx)
            if 'acc' in fast:
                np.testing.assert_array_equal(fast['acc'][:min(int(summ['n_meas'][L]), MEAS_CAP), L], r['acc'], err_msg=ctx)
            np.testing.assert_array_equal(fast['regs'][:, L], r['regs'], err_msg=ctx)
    return n


@pytest.mark.parametrize('r', ROWS, ids=IDS)
def test_fast_equals_rtl_on_the_row(r):
    case, ps = wc.case_of_row(r)
    cfg, _ = wc.config_of_row(r)
    n_shots = 3 if r.C < 64 else 2
    cfg2, fast, rtl = run_both(case, n_shots=n_shots, seed=SEED_A, shot0=wc.shot0_of(r),
                               **model_kw(r, cfg, ps.n_programs))
    st = compare(cfg2, fast, rtl, n_shots)
    assert st['done'] > 0 and st['events'] > 0
    n_dead = compare_deadlocks(cfg2, fast, rtl, n_shots)
    assert n_dead == st['other']                        # nothing ends in another way
    assert (n_dead > 0) == (wc.built_to_deadlock(r) or r.sync != 'all')


# ---- (b) reach ----

class View:
    """a row's oracle run under one seed, by (local shot, core)"""

    def __init__(self, r, seed=SEED_A, **over):
        self.r = r
        self.case, self.ps = wc.case_of_row(r)
        self.plan = self.case['plan']
        self.cfg, tables = wc.config_of_row(r, seed, **over)
        if over:
            f = oracle.fast_run(self.cfg, self.ps.words, self.ps.offsets, self.ps.n_instr, self.ps.table, wc.shot0_of(r),
                                r.n_shots, want=wc.outs_of(self.cfg), ro=tables)
        else:
            f = wc.oracle_of_row(r, seed)
        self.f = f
        self.s = _abi.unpack_summary(f['summary'])
        shot, core = fc.lane_shots_cores(self.cfg, r.n_shots, wc.shot0_of(r))
        self.lane = np.zeros((r.n_shots, r.C), np.int64)
        self.lane[shot - wc.shot0_of(r), core] = np.arange(r.n_shots * r.C)
        self.group = ((wc.shot0_of(r) + np.arange(r.n_shots)) // r.shots_per_group) % r.n_groups
        self.status = self.s['status'][self.lane]
        tr = f['trace']
        nt = np.minimum(self.s['n_trace'], self.cfg.trace_cap)
        is_rst = (tr[:, :, 1] == RST) & (np.arange(tr.shape[0])[:, None] < nt[None, :])
        self.n_rst = is_rst.sum(axis=0)[self.lane]
        self.rst_t = [[tr[is_rst[:, self.lane[s, c]], self.lane[s, c], 0] for c in range(r.C)] for s in range(r.n_shots)]

    def bit(self, s, c, m):
        """outcome m of core c in shot s"""
        assert m < self.s['n_meas'][self.lane[s, c]]
        return int(self.f['meas'][m, self.lane[s, c], 1])

    def strobed(self, c, k):
        """readouts core c has strobed by the end of stretch k"""
        return sum(c in self.plan['strobes'][j] for j in range(k + 1))

    def data(self, s, rd):
        """what the read sees in shot s, as the plan has it; None: not planned"""
        if rd.get('fire') is not None:
            k = rd['fire']
            addr = sum(self.bit(s, c, self.strobed(c, k) - 1) << c for c in self.plan['strobes'][k] if c < 8)
            return (self.cfg.lut_table[addr] >> rd['core']) & 1
        if rd['m'] is None:
            return None
        return self.bit(s, rd['target'], rd['m'])

    def reads(self, s, c=None):
        return [rd for rd in self.plan['reads'] if rd['group'] == self.group[s] and (c is None or rd['core'] == c)]


@functools.lru_cache(maxsize=None)
def view(r, seed=SEED_A):
    return View(r, seed)


def check_plan_against_oracle(v):
    """every DONE lane whose reads are all planned: the event count is the plan's, less the pulses its taken jumps
    skip, and every alu_fproc left its register as the planned outcome gives it; -> (lanes checked, jump reads taken,
    jump reads not taken)"""
    r, checked, taken, kept = v.r, 0, 0, 0
    for s in range(r.n_shots):
        for c in range(r.C):
            L = v.lane[s, c]
            rds = v.reads(s, c)
            if v.status[s, c] != _abi.ST_DONE or any(v.data(s, rd) is None for rd in rds):
                continue
            n_ev = v.plan['base_events'][v.group[s]][c]
            for rd in rds:
                out = alu(rd['op'], rd['imm'], v.data(s, rd))
                if rd['kind'] == 'jump':
                    n_ev -= rd['skips'] * (out & 1)
                    taken, kept = taken + (out & 1), kept + 1 - (out & 1)
                else:
                    assert v.f['regs'][rd['rd'], L] == out, (wc.row_id(r), s, rd)
            assert v.s['n_events'][L] == n_ev, (wc.row_id(r), s, c)
            checked += 1
    return checked, taken, kept


def both_outcomes(v, pick):
    """a read among pick(read) whose planned outcome is 1 in some shots and 0 in others, the reader DONE in both"""
    seen = {}
    for s in range(v.r.n_shots):
        for rd in v.reads(s):
            if pick(rd) and v.status[s, rd['core']] == _abi.ST_DONE and v.data(s, rd) is not None:
                seen.setdefault((rd['core'], rd['round'], rd['fid'], rd['kind']), set()).add(v.data(s, rd))
    return any(len(x) == 2 for x in seen.values())


def reach_problems(r):
    bad = []
    v = view(r)
    plan, C = v.plan, r.C
    rows = C // 16
    part, outside = plan['part'], plan['outside']
    done = v.status == _abi.ST_DONE
    # barriers: at least two released in every shot, seen in every 16-lane row that holds a participant
    for s in range(r.n_shots):
        for row in range(rows):
            cs = [c for c in part if c // 16 == row and c not in plan['skip']]
            if cs and not all(v.n_rst[s, c] >= 2 for c in cs):
                bad.append('shot {}: fewer than two barriers released in row {}'.format(s, row))
    # ... and the planned core was the last to arrive: the release follows its idle, T + 5 + sync_latency after
    # the last one (qclk = 0 at the release record), T + 6 + sync_latency after cycle 0
    if not plan['skip']:
        for s in range(r.n_shots):
            t = v.rst_t[s][part[0]]
            for k in range(1, len(t) + 1):
                T = plan['last_T'][v.group[s]][k]
                want = T + 5 + v.cfg.sync_latency + (int(t[k - 2]) if k > 1 else 1)
                if int(t[k - 1]) != want:
                    bad.append('shot {} barrier {}: released at {}, not {}'.format(s, k, t[k - 1], want))
    if r.sync != 'all':
        if not any(done[s, part].all() and (v.status[s, outside] == _abi.ST_DEADLOCK).all() for s in range(r.n_shots)):
            bad.append('no shot whose participants end DONE and whose other cores end in DEADLOCK')
        if not (v.status[:, outside] == _abi.ST_DEADLOCK).all():
            bad.append('a core outside sync_mask does not end in DEADLOCK')
        if C == 64 and not (v.n_rst[:, [c for c in part if c >= 32]] >= 1).any():
            bad.append('no released barrier with a participant at or above 32')
    checked, taken, kept = check_plan_against_oracle(v)
    if not checked or not taken or not kept:
        bad.append('no lane checked against the plan, or no jump_fproc taken / not taken')
    planned = [rd for rd in plan['reads'] if rd['m'] is not None or rd.get('fire') is not None]
    if r.backend == 'meas':
        if rows > 1 and not any(rd['target'] // 16 != rd['core'] // 16 for rd in planned):
            bad.append('no read of a core in another 16-lane row')
        if C == 64 and not any(rd['target'] // 32 != rd['core'] // 32 for rd in planned):
            bad.append('no read of a core in the other 32-lane half')
        if not any(rd['fid'] >= C for rd in planned):
            bad.append('no read with an id at or above C')
        if not both_outcomes(v, lambda rd: rd['kind'] == 'jump' and (rows == 1 or rd['target'] // 16 != rd['core'] // 16)):
            bad.append('no cross-row jump_fproc that sees 1 in some shots and 0 in others')
        if not both_outcomes(v, lambda rd: rd['fid'] >= C):
            bad.append('no read with an id at or above C that sees 1 in some shots and 0 in others')
    else:
        waits = [(s, rd) for s in range(r.n_shots) for rd in v.reads(s) if rd.get('fire') is not None]
        own = [rd for rd in plan['reads'] if rd['fid'] == 0]
        if not waits or not own:
            bad.append('no read with a nonzero id, or none with id 0')
        high = 32 if C == 64 else 16 if C == 32 else 8
        if r.lut == 'never':
            if not all(v.status[s, rd['core']] == _abi.ST_DEADLOCK for s, rd in waits):
                bad.append('a LUT wait does not end in DEADLOCK though the LUT never fires')
        else:
            if not all(done[s, rd['core']] for s, rd in waits if rd['core'] in part):
                bad.append('a LUT wait is not released')
            if not any(rd['core'] >= high and done[s, rd['core']] for s, rd in waits):
                bad.append('no lane at core >= {} released by a fire'.format(high))
            if not both_outcomes(v, lambda rd: rd.get('fire') is not None and rd['kind'] == 'jump' and rd['core'] >= high // 2 * 2
                                 and rd['core'] >= min(16, high)):
                bad.append('no lut_table bit at or above {} that decides a branch both ways'.format(min(16, high)))
            # the fires are what releases them: with a core that never measures in the mask, each of the waits
            # ends in DEADLOCK; and with any one bit of the mask cleared, the run is another
            dead = View(r, SEED_A, lut_mask=v.cfg.lut_mask | (1 << wc.QUIET[C][0]))
            if not all(dead.status[s, rd['core']] == _abi.ST_DEADLOCK for s, rd in waits):
                bad.append('a LUT wait survives a mask that cannot fire')
            for b in range(32):
                if (v.cfg.lut_mask >> b) & 1 and v.cfg.lut_mask != 1 << b:
                    other = View(r, SEED_A, lut_mask=v.cfg.lut_mask & ~(1 << b))
                    if np.array_equal(other.f['summary'], v.f['summary']):
                        bad.append('clearing bit {} of lut_mask changes nothing'.format(b))
    if not wc.built_to_deadlock(r) and 4 * int((~done).sum()) > done.size:
        bad.append('more than a quarter of the lanes end other than DONE')
    if r.model == 'states':
        b = view(r, SEED_B)
        if max(v.s['n_meas'].max(), b.s['n_meas'].max()) > 31:
            bad.append('a lane measures more than 31 times')
        if not fc.paths_differ(v.f, b.f).any():
            bad.append('no lane takes another path under the second seed')
    if int(np.bitwise_or.reduce(v.s['flags'])):
        bad.append('a flag is raised (late trigger, overflow): the plan does not hold')
    return bad


@pytest.mark.parametrize('r', ROWS, ids=IDS)
def test_row_reaches_what_it_is_there_for(r):
    assert not reach_problems(r)


def test_last_arrivals_cover_every_row_and_half():
    """over the table the last-arriving participant of some barrier lies in each 16-lane row (at C = 64: in each
    32-lane half), in both lane orders; at C = 32, shot-major, the C-wide reduction spans rows 0-1 of a wave for even
    local shots and rows 2-3 for odd ones, and the table has barriers in both"""
    seen = {}
    for r in ROWS:
        case, _ = wc.case_of_row(r)
        if r.variant != 'skip':
            seen.setdefault((r.C, r.order), set()).update(c // 16 for c in case['plan']['last'][1:])
    for C in (16, 32, 64):
        for order in (wc.CM, wc.SM):
            assert seen[(C, order)] == set(range(C // 16)), (C, order)
    for r in ROWS:
        if r.C == 32 and r.order == wc.SM:
            assert r.n_shots >= 2 and view(r).n_rst[0].max() >= 2 and view(r).n_rst[1].max() >= 2


def test_states_rows_plant_every_full_range_word():
    """the supplied-states rows' buffers hold 0, 0xFFFFFFFF, 0x80000000 and 0x55555555 at cores at or above 16 (C = 16:
    at any core), each on a lane whose readouts agree with seed B's draws on every bit the lane reads"""
    for r in ROWS:
        if r.model == 'states':
            states, used = wc.planted_states(r)
            assert used == set(wc.PLANTED), (wc.row_id(r), [hex(w) for w in used])
            assert len(states) == r.n_shots * r.C


# ---- (c) the plan ----

MODEL = {'state': _abi.MEAS_STATE, 'readout': _abi.MEAS_READOUT, 'demod': _abi.MEAS_DEMOD, 'states': _abi.MEAS_STATE}


def plan_case(r):
    _, ps = wc.case_of_row(r)
    parts = case_words(r.C, ps.n_groups, ps.words, ps.offsets, ps.n_instr, ps.table)
    fproc_mode = _abi.FPROC_LUT if r.backend == 'lut' else _abi.FPROC_MEAS
    parts[0] = np.concatenate([parts[0], np.array([r.shots_per_group, r.order, r.exec_flags, MODEL[r.model], fproc_mode,
                                                   r.n_shots], np.uint32)])
    return parts


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_every_row_plans_the_kernel_it_claims(tmp_path):
    caps, plans = run_plans(tmp_path, [plan_case(r) for r in ROWS])
    for r, (facts, off, on) in zip(ROWS, plans):
        pl = on if r.model == 'states' else off
        assert pl['name'] == wc.kernel_name(r), wc.row_id(r)
        assert ',c8' not in pl['name'] and ',c8' not in on['name'], wc.row_id(r)
        assert pl['family'] == (caps['k_interp'] if r.family == 'interp' else caps['k_branch']), wc.row_id(r)
        assert bool(pl['lds']) == wc.staged(r), wc.row_id(r)
        assert facts['has_fproc'] and facts['has_sync'] and not facts['linear'], wc.row_id(r)


# ---- (d) the table ----

def test_table_shapes():
    for r in ROWS:
        lanes = r.n_shots * r.C
        assert 257 <= lanes <= 511 and r.n_groups >= 2 and r.shots_per_group < 256 // r.C, wc.row_id(r)
        assert r.n_shots > r.shots_per_group * (r.n_groups - 1), wc.row_id(r)       # every group runs
        if r.C == 64:
            assert r.n_shots in (5, 7)
        elif r.C == 32:
            assert r.n_shots % 2 == 1 and 9 <= r.n_shots <= 15
        else:
            assert r.C == 16 and 17 <= r.n_shots <= 31 and r.n_shots % 4
        cfg, _ = wc.config_of_row(r)
        assert 'hist' not in wc.outs_of(cfg)
        p1 = wc.p1_of(r)
        assert r.C == 16 or (0.0 in p1[16:] and 1.0 in p1[16:])
        m = wc.sync_mask_of(r)
        if r.sync == 'holes':
            assert [c for c in range(16) if not (m >> c) & 1] and [c for c in range(r.C - 16, r.C) if not (m >> c) & 1]
        if r.sync == 'b63':
            assert r.C == 64 and (m >> 63) & 1 and not (m >> 31) & 1
        if r.sync == 'high':
            assert r.C == 64 and m and not m & 0xFFFFFFFF
        assert cfg.lut_mask < 2 ** 32 and (r.lut != 'ends' or r.C >= 32)
        if r.lut == 'never':
            assert cfg.lut_mask & sum(1 << c for c in wc.QUIET[r.C])
        elif r.lut:
            assert not cfg.lut_mask & sum(1 << c for c in wc.QUIET[r.C]) and cfg.lut_mask < 1 << r.C
    assert 40 <= len(ROWS) <= 60 and len(set(IDS)) == len(ROWS)


def test_table_covers_its_axes():
    have = lambda *f: {tuple(getattr(r, k) for k in f) for r in ROWS}
    Cs, backs, fams = (16, 32, 64), ('meas', 'lut'), ('branch', 'interp')
    assert have('C', 'backend', 'family') == {(c, b, f) for c in Cs for b in backs for f in fams}
    assert have('C', 'model') == {(c, m) for c in Cs for m in ('state', 'readout', 'demod', 'states')}
    assert have('C', 'sync') == {(c, k) for c in Cs for k in ('all', 'holes')} | {(64, 'b63'), (64, 'high')}
    assert have('C', 'lut') == {(c, k) for c in Cs for k in (None, 'std', 'never')} | {(32, 'ends'), (64, 'ends')}
    assert have('C', 'order') == {(c, o) for c in Cs for o in (wc.CM, wc.SM)}
    assert have('C', 'backend', 'order') == {(c, b, o) for c in Cs for b in backs for o in (wc.CM, wc.SM)}
    assert have('C', 'variant') >= {(c, 'skip') for c in Cs} | {(16, 'short'), (32, 'short')}
    # staged and global fetches in both families; DPEMU_X_PROG_MAJOR and its absence on branch_kernel at every C
    assert {(r.family, wc.staged(r)) for r in ROWS} == {(f, s) for f in fams for s in (True, False)}
    assert {(r.C, bool(r.exec_flags & wc.XM)) for r in ROWS if r.family == 'branch'} == {(c, x) for c in Cs for x in (True, False)}
    assert {(r.C, bool(r.exec_flags & wc.XL)) for r in ROWS if r.family == 'interp'} == {(c, x) for c in Cs for x in (True, False)}
    assert all(r.exec_flags == (wc.XG | (r.exec_flags & wc.XL)) for r in ROWS if r.family == 'interp')
    assert all(not r.exec_flags & ~wc.XM for r in ROWS if r.family == 'branch')
    assert all(r.model in ('state', 'readout') for r in ROWS if r.family == 'interp')


# ---- (e) mask bits that name no core ----

def mask_case(C, seed):
    return progfuzz.random_case(60000 + 100 * C + seed, ncores=C, mode='meas', allow_late=False, allow_hang=False)


@pytest.mark.parametrize('C,mask', [(4, 0b10111), (4, 0b11111), (16, 0x1FFFF), (16, 0x1FF7F)],
                         ids=['c4-0b10111', 'c4-0b11111', 'c16-all-and-bit16', 'c16-hole-and-bit16'])
def test_sync_mask_bits_at_or_above_C_are_ignored(C, mask):
    """both oracles, on random programs and on a wide case: the run under the mask equals the run under its bits
    below C"""
    cases = [mask_case(C, seed) for seed in range(10)]
    if C == 16:
        low = mask & 0xFFFF
        cases.append(progfuzz.wide_case(77, 16, 2, ro_clocks=20, sync_mask=0 if low == 0xFFFF else low))
    n_rst = 0
    for case in cases:
        cfg, fast, rtl = run_both(case, n_shots=2, sync_mask=mask)
        compare(cfg, fast, rtl, 2)
        compare_deadlocks(cfg, fast, rtl, 2)
        cfg_low, fast_low, _ = run_both(case, n_shots=2, sync_mask=mask & ((1 << C) - 1))
        for k in fast:
            np.testing.assert_array_equal(fast[k], fast_low[k], err_msg=k)
        n_rst += int((fast['trace'][:, :, 1] == RST).sum())
    assert n_rst > 0                                    # barriers were released


@pytest.mark.parametrize('C,mask', [(4, 0b110000), (16, 0x30000)])
def test_sync_mask_without_a_bit_below_C_leaves_no_participant(C, mask):
    n_sync = 0
    for case in [mask_case(C, seed) for seed in range(10)] + [progfuzz.wide_case(78, 16, 2, ro_clocks=20)] * (C == 16):
        cfg, fast, rtl = run_both(case, n_shots=2, sync_mask=mask)
        compare(cfg, fast, rtl, 2)
        compare_deadlocks(cfg, fast, rtl, 2)
        assert not (fast['trace'][:, :, 1] == RST).any()
        s = _abi.unpack_summary(fast['summary'])
        for L in range(2 * C):                          # core-major lanes, one group per shot
            prog = case['progs'][case['table'][((L % 2) % case['n_groups']) * C + L // 2]]
            at = int(s['ip'][L])
            if s['status'][L] == _abi.ST_DEADLOCK and at < len(prog) and isa.decode(prog[at])['op'] == 'sync':
                n_sync += 1
    assert n_sync > 0


@pytest.mark.parametrize('C,mask', [(4, 0b10011), (16, 0x10101)])
def test_lut_mask_bits_at_or_above_C_keep_the_lut_from_firing(C, mask):
    """no core at or above C ever measures, so the FSM never sees its mask complete: in both oracles the run does not
    depend on lut_table (under the bits below C it does), and reads with a nonzero id end in DEADLOCK"""
    ones = [2 ** 64 - 1] * 256
    stuck, table_matters = 0, False
    cases = [progfuzz.random_case(61000 + 100 * C + seed, ncores=C, mode='lut', allow_late=False, allow_hang=False)
             for seed in range(10)]
    # (random LUT programs seldom take a branch on a fire: the wide case does, at run_both's meas_latency of 20)
    cases.append(progfuzz.wide_case(79, C, 2, mode='lut', ro_clocks=20, lut_mask=mask & ((1 << C) - 1), quiet=(C - 1,)))
    for case in cases:
        runs = {}
        for m in (mask, mask & ((1 << C) - 1)):
            for name, kw in (('default', {}), ('ones', dict(lut_table=ones))):
                cfg, fast, rtl = run_both(case, n_shots=2, lut_mask=m, **kw)
                compare(cfg, fast, rtl, 2)
                compare_deadlocks(cfg, fast, rtl, 2)
                runs[m, name] = fast
        for k in runs[mask, 'default']:
            np.testing.assert_array_equal(runs[mask, 'default'][k], runs[mask, 'ones'][k], err_msg=k)
        low = mask & ((1 << C) - 1)
        table_matters |= any(not np.array_equal(runs[low, 'default'][k], runs[low, 'ones'][k]) for k in fast)
        s = _abi.unpack_summary(runs[mask, 'default']['summary'])
        for L in range(2 * C):                          # core-major lanes, one group per shot
            prog = case['progs'][case['table'][((L % 2) % case['n_groups']) * C + L // 2]]
            at = int(s['ip'][L])
            d = isa.decode(prog[at]) if at < len(prog) else {'op': 'done'}
            stuck += s['status'][L] == _abi.ST_DEADLOCK and d['op'] in ('alu_fproc', 'jump_fproc') and d['fproc_id'] != 0
    assert stuck > 0 and table_matters


# ---- (f) the earlier generators draw what they drew ----

def _digest(cases):
    h = hashlib.sha256()
    for case in cases:
        h.update(repr((case['ncores'], case['mode'], case['n_groups'], case['progs'], case['table'].tolist())).encode())
    return h.hexdigest()[:16]


def test_earlier_generators_draw_what_they_drew():
    """progfuzz.wide_case shares Gen with random_case, shaped_case and macro_shape_case: their outputs over the seed
    ranges the suite uses, hashed before wide_case was added"""
    rc = _digest([progfuzz.random_case(s) for s in range(0, 70000, 97)] +
                 [progfuzz.random_case(s, ncores=c, mode=m, allow_late=False, allow_hang=False)
                  for s in range(1000, 6000, 53) for c, m in ((4, 'meas'), (8, 'lut'), (16, 'meas'))] +
                 [progfuzz.random_case(s, ncores=64, mode='meas', linear=True, body=(3, 6)) for s in range(500, 600)])
    sc = _digest([progfuzz.shaped_case(s, c, n_groups=1 + s % 3, linear=bool(s & 1)) for s in range(71000, 71100)
                  for c in (1, 8)])
    mc = _digest([progfuzz.macro_shape_case(s, 2, 3, regs, 6, breaks={2: progfuzz.BREAKERS[s % 5]}, late_at=(4,))
                  for s in range(300) for regs in ((1, 2), (0, 3, 5, 9))])
    assert (rc, sc, mc) == EARLIER_DRAWS


EARLIER_DRAWS = ('4ca823d383790555', '0762fe6276c9ba17', '36ccea6e7bd9b78a')
