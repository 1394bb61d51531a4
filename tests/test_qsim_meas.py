"""CPU tests of the measuring qubit-state stage (dpemu_qsim_meas, include/dpemu.h)
and of the states it hands to the readout stages: the specification, through
its Python-integer restatement tests/qsim_meas_ref.py, on event records written
by hand (tests/test_qsim.py's helpers), and the injected readout references
against their base references.  tests/test_gpu_qsim_meas.py holds the kernels
to the same references bit for bit."""

import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from distributed_processor_amd import _abi, qsim, workloads
from tests import feedline_ref, iq_stats_ref, qsim_meas_ref as mref, qsim_ref, resonator_ref, traces_ref
from tests.test_demod import ro_program
from tests.test_demod_iq import SQUARE
from tests.test_feedline import fl_cfg, synth_cores
from tests.test_qsim import HAND_KEYS, hand_events, hand_gateset, strobe

HERE = os.path.dirname(os.path.abspath(__file__))
ONE = 1 << 30
FULL = 1 << 60
RDLO = workloads.RDLO
X0, CR, X1 = (HAND_KEYS[k] for k in ('x0', 'cr', 'x1'))
SEED = 0x5EED0C0FFEE


def ro(t):
    """a readout (rdlo) strobe: what it carries besides its element does not matter"""
    return strobe(t, 3, 0x0FA000, 0xFFFF, 0x155, elem=RDLO)


def cfg_of(C_, cap, **kw):
    return _abi.make_config(C_, event_cap=cap, seed=SEED, **kw)


def per_shot(lanes_of_shot, n_shots, C_):
    """core-major lane lists from one shot's per-core record lists, the same in every shot"""
    return [list(lanes_of_shot[c]) for c in range(C_) for _ in range(n_shots)]


def run(cfg, gs, lanes, n_shots, cap=None, **kw):
    summary, ev = hand_events(lanes, cap)
    return mref.qsim_meas_gateset(cfg, gs, summary, ev, n_shots, event_cap=cap, **kw) + (summary, ev)


# ---- 1. without readout strobes the stage is dpemu_qsim ----

def test_no_readout_is_qsim():
    cfg = cfg_of(2, 8)
    shots = [([strobe(42, *CR, 0)], [strobe(58, *X1, 0x10000)]),
             ([strobe(10, *X0, 0), strobe(26, *X0, 0), strobe(42, *CR, 0)], [strobe(58, *X1, 0x10000)]),
             ([strobe(10, *X0, 0x8000), strobe(7, 1, 2, 3, 4, elem=1)], [strobe(10, 9, 9, 9, 9)])]
    lanes = [s[0] for s in shots] + [s[1] for s in shots]
    pops, res, states, summary, ev = run(cfg, hand_gateset(), lanes, len(shots))
    want = qsim_ref.qsim_gateset(cfg, hand_gateset(), summary, ev, len(shots))
    np.testing.assert_array_equal(pops, want[0])
    np.testing.assert_array_equal(res, want[1])
    assert states.shape == (6,) and not states.any() and res[0, 2, 2] == 1


# ---- 2. outcomes ----

def test_x180_reads_one():
    n = 64
    cfg = cfg_of(2, 8)
    lanes = per_shot([[strobe(10, *X0, 0), strobe(26, *X0, 0), ro(60)], [ro(60)]], n, 2)
    pops, res, states, _, _ = run(cfg, hand_gateset(), lanes, n)
    assert (states[:n] == 1).all() and (states[n:] == 0).all()       # the first core's X180; the second never driven
    assert (res[0, :, 0] == 1).all() and (res[0, :, 1] == 2).all() and (res[0, :, 2:] == 0).all()
    assert (pops[0, :, 2] >= 1 << 58).all() and (pops[0, :, [0, 1, 3]] == 0).all()


def test_x90_reads_half_and_repeats():
    """X90, then two readouts: k of N first readouts read 1 with |k / N - 1/2| <= 5 / (2 sqrt N), five standard
    deviations of the binomial; the second readout repeats the first; the collapsed state is renormalised"""
    n = 400
    cfg = cfg_of(1, 4)
    gs = qsim.GateSet().add_rotation(0, *X0, np.pi / 2).registers([0])
    shifts, amps = [], []
    pops, res, states, _, _ = run(cfg, gs, per_shot([[strobe(10, *X0, 0), ro(60), ro(90)]], n, 1), n, shifts=shifts,
                                  amps=amps)
    first, second = states & 1, (states >> 1) & 1
    k = int(first.sum())
    assert abs(k / n - 0.5) <= 5 / (2 * np.sqrt(n)), k
    assert 0 < k < n and (first == second).all() and (states >> 2 == 0).all()
    tot = pops[0].astype(object).sum(axis=1)
    assert all((1 << 58) <= int(t) < (1 << 60) for t in tot)          # after a 50/50 collapse: sum of pops in [2^58, 2^60)
    assert (res[0, :, 0] == first).all()                              # the final sample of a basis state is that state
    # T ~ 2^60 before the first readout, so T' ~ 2^59 and s = 0 there; the second readout finds T = T' and s = 0
    assert {s for _, _, _, _, s in shifts} == {0}
    assert all(x[1] == (0, 0) and x[3] == (0, 0) and ((x[0] == (0, 0)) != (x[2] == (0, 0))) for x in amps)


def bell_lanes(gs):
    """X90 on the control, then the CNOT of workloads.rb2q_gateset's pulses (clifford2q's native one: the ZX90 on
    the control's drive at phase 0, then X-90 on the target), then a readout of each core"""
    x90_c, zx, x90_t = (tuple(gs.entries[i][k] for k in ('freq', 'env', 'amp')) for i in range(3))
    assert [gs.entries[i]['core'] for i in range(3)] == [0, 0, 1] and gs.entries[1]['kind'] == 1
    return [[strobe(10, *x90_c, 0), strobe(42, *zx, 0), ro(120)], [strobe(58, *x90_t, 0x10000), ro(100)]]


def test_bell_pair_agrees():
    n = 128
    cfg = cfg_of(2, 4)
    gs = workloads.rb2q_gateset(2)
    pops, res, states, _, _ = run(cfg, gs, per_shot(bell_lanes(gs), n, 2), n)
    a, b = states[:n], states[n:]
    assert (a == b).all() and set(a.tolist()) == {0, 1}
    assert (res[0, :, 1] == 3).all() and (res[0, :, 0] == 3 * a).all()    # |00> or |11>


# ---- 3. edges of the rule ----

def test_tie_takes_the_first_cores_record():
    """a readout at the other lane's drive strobe's t.  The second core's readout against the control's ZX90:
    the gate goes first (t_first <= t_second), so the target is measured in a superposition; were the readout
    first it would read 0 in every shot.  The first core's readout against the second core's pulse: the readout
    goes first, as with the pulse one clock later"""
    n = 96
    cfg = cfg_of(2, 4)
    drive_first = per_shot([[strobe(10, *X0, 0), strobe(26, *X0, 0), strobe(50, *CR, 0)], [ro(50)]], n, 2)
    pops, res, states, _, _ = run(cfg, hand_gateset(), drive_first, n)
    assert set(states[n:].tolist()) == {0, 1} and not states[:n].any()
    late = per_shot([[strobe(10, *X0, 0), strobe(26, *X0, 0), strobe(50, *CR, 0)], [ro(51)]], n, 2)
    same = run(cfg, hand_gateset(), late, n)
    np.testing.assert_array_equal(pops, same[0])
    np.testing.assert_array_equal(states, same[2])
    early = per_shot([[strobe(10, *X0, 0), strobe(26, *X0, 0), strobe(50, *CR, 0)], [ro(49)]], n, 2)
    assert not run(cfg, hand_gateset(), early, n)[2].any()
    # the other way round
    tie = per_shot([[strobe(10, *X0, 0), ro(50)], [strobe(50, *X1, 0)]], n, 2)
    after = per_shot([[strobe(10, *X0, 0), ro(50)], [strobe(51, *X1, 0)]], n, 2)
    got, want = run(cfg, hand_gateset(), tie, n), run(cfg, hand_gateset(), after, n)
    for g, w in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(g, w)
    assert set(got[2][:n].tolist()) == {0, 1}


def test_registers_of_one_and_cores_of_none():
    """C = 4: register (0, 1), the one-qubit register 2 and core 3 in no register, whose readouts leave 0"""
    n = 32
    cfg = cfg_of(4, 4)
    key2 = (2, 0x040000, 5000)
    gs = hand_gateset()
    gs.add_rotation(2, *key2, np.pi)
    gs.registers([(0, 1), 2])
    lanes = per_shot([[ro(20)], [strobe(10, *X1, 0), strobe(26, *X1, 0), ro(40)], [strobe(10, *key2, 0), ro(30), ro(31)],
                      [strobe(10, *key2, 0), ro(30)]], n, 4)
    pops, res, states, _, _ = run(cfg, gs, lanes, n)
    st = states.reshape(4, n)
    assert not st[0].any() and (st[1] == 1).all() and (st[2] == 3).all() and not st[3].any()
    assert (res[1, :, 0] == 1).all() and (pops[1, :, [1, 3]] == 0).all() and (res[0, :, 0] == 2).all()


def test_forty_readouts():
    """bits stop at 32, collapse does not: an X90 after readout 31 makes readouts 32..39 random again -- they
    still collapse (the final state is a basis state, both values occur) and leave no bit"""
    n = 48
    cfg = cfg_of(1, 64)
    gs = qsim.GateSet().add_rotation(0, *X0, np.pi / 2).registers([0])
    recs = [strobe(10, *X0, 0)] + [ro(20 + i) for i in range(32)] + [strobe(60, *X0, 0)] + [ro(70 + i) for i in range(8)]
    shifts = []
    pops, res, states, _, _ = run(cfg, gs, per_shot([recs], n, 1), n, shifts=shifts)
    assert set(states.tolist()) == {0, 0xFFFFFFFF}
    assert max(m for _, _, m, _, _ in shifts) == 39 and len(shifts) == 40 * n
    assert ((pops[0] != 0).sum(axis=1) == 1).all() and (res[0, :, 1] == 2).all()
    flipped = res[0, :, 0] != (states & 1)
    assert 0 < flipped.sum() < n                          # readout 32 was a fresh 50/50 draw
    late = {(row, m): b for row, _, m, b, _ in shifts if m >= 32}
    assert all(late[(row, 32)] == late[(row, 39)] == int(res[0, row, 0]) for row in range(n))


def test_readouts_beyond_event_cap():
    n, cap = 16, 3
    cfg = cfg_of(1, cap)
    gs = qsim.GateSet().add_rotation(0, *X0, np.pi / 2).registers([0])
    recs = [strobe(10, *X0, 0), strobe(26, *X0, 0), ro(40), strobe(50, *X0, 0), strobe(66, *X0, 0), ro(80)]
    pops, res, states, summary, _ = run(cfg, gs, per_shot([recs], n, 1), n, cap=cap)
    assert (summary[:, 2] == 6).all()
    assert (states == 1).all() and (res[0, :, 1] == 2).all() and (res[0, :, 3] == 1 << 31).all()
    assert (res[0, :, 0] == 1).all()                      # the X180 and readout past the cap never act


def test_small_state_is_shifted_up():
    """a dictionary entry scaled by 2^-6 (not unitary): T ~ 2^48 at the readout, so s >= 5 on either outcome,
    asserted from the reference; the shifted state's populations sum to [2^58, 2^60)"""
    n = 64
    cfg = cfg_of(1, 4)
    gs = qsim.GateSet().add_matrix(0, *X0, qsim.rotation(np.pi / 2) / 64).registers([0])
    shifts = []
    pops, res, states, _, _ = run(cfg, gs, per_shot([[strobe(10, *X0, 0), ro(40)]], n, 1), n, shifts=shifts)
    assert len(shifts) == n and {b for _, _, _, b, _ in shifts} == {0, 1}
    assert all(s >= 5 for _, _, _, _, s in shifts)
    tot = pops[0].astype(object).sum(axis=1)
    assert all((1 << 58) <= int(t) < (1 << 60) for t in tot)
    assert mref.shift_of(0) == 0 and mref.shift_of(1) == 29 and mref.shift_of(1 << 57) == 1
    assert mref.shift_of((1 << 58) - 1) == 1 and mref.shift_of(1 << 58) == 0 and mref.shift_of((1 << 64) - 1) == 0


def test_rebatched():
    """counter-based draws: two half batches from their own shot_begin reproduce one batch"""
    n = 40
    cfg = cfg_of(2, 4)
    gs = workloads.rb2q_gateset(2)
    lanes = per_shot(bell_lanes(gs), n, 2)
    pops, res, states, _, _ = run(cfg, gs, lanes, n, shot_begin=2 ** 32 - 7)
    for b, e in ((0, n // 2), (n // 2, n)):
        p2, r2, s2, _, _ = run(cfg, gs, per_shot(bell_lanes(gs), e - b, 2), e - b, shot_begin=2 ** 32 - 7 + b)
        np.testing.assert_array_equal(p2[0], pops[0, b:e])
        np.testing.assert_array_equal(r2[0], res[0, b:e])
        np.testing.assert_array_equal(s2.reshape(2, -1), states.reshape(2, n)[:, b:e])


# ---- 4. injected readout references ----

def readout_case():
    """4 cores x 2 shots, two readouts per lane at 1:1, lines of three members and of one"""
    env = np.full(4 * 40, SQUARE, np.uint32)
    reads = [[dict(A=20000 + 3000 * c + 500 * k, ph_d=777 * k + c, ph_lo=99 * c, L_d=20, L_lo=16, lo_at=4 + c,
                   gap=100 + 3 * c) for k in range(2)] for c in range(4)]
    cfg = fl_cfg(4, delay=2, theta=(0.4, 2.5), gain=(0.9, 0.6), p1=[0.3, 0.5, 0.7, 0.5], sigma=30.0, meas_cap=2, seed=SEED)
    f_d = [0x01234567 + 0x111111 * c for c in range(4)]
    out, pairs, iq_d, iq_l = synth_cores([ro_program(r) for r in reads], cfg, f_d, [f - 40 for f in f_d], (1, 1), (1, 1),
                                         env, 256, n_shots=2, shot0=5)
    lines = [[0, 1, 2], [3], [6, 4, 5], [7]]
    return cfg, out, pairs, iq_d, iq_l, lines


def test_injected_references_reproduce_the_draws():
    cfg, out, pairs, iq_d, iq_l, lines = readout_case()
    n = len(pairs['lane'])
    summary, ev = out['summary'], out['events']
    words = mref.draw_words(cfg, pairs['shot'], pairs['core'])
    states = np.zeros(n, np.uint32)
    states[np.asarray(pairs['lane'])] = words
    assert len(set((words & 3).tolist())) >= 3            # the draws differ between the lanes and the slots
    n_lo = iq_l.shape[1]
    adc = feedline_ref.feedline_adc(cfg, pairs, lines, summary, ev, iq_d, n_lo, 2)
    np.testing.assert_array_equal(mref.feedline_adc_st(states, cfg, pairs, lines, summary, ev, iq_d, n_lo, 2), adc)
    assert not np.array_equal(mref.feedline_adc_st(states ^ 3, cfg, pairs, lines, summary, ev, iq_d, n_lo, 2), adc)
    rng = np.random.default_rng(3)
    ang = rng.uniform(0, 2 * np.pi, (n, 2, 2))
    coef = np.rint(np.stack([0.8 * np.cos(ang[..., 0]), 0.8 * np.sin(ang[..., 0]), 0.7 * np.cos(ang[..., 1]),
                             0.7 * np.sin(ang[..., 1])], axis=-1) * ONE).astype(np.int64)
    res = resonator_ref.feedline_adc_res(cfg, pairs, lines, coef, 300, summary, ev, iq_d, n_lo, 2)
    np.testing.assert_array_equal(mref.feedline_adc_res_st(states, cfg, pairs, lines, coef, 300, summary, ev, iq_d, n_lo, 2),
                                  res)
    assert not np.array_equal(mref.feedline_adc_res_st(states ^ 3, cfg, pairs, lines, coef, 300, summary, ev, iq_d, n_lo, 2),
                              res)
    tr = traces_ref.feedline_traces(cfg, pairs, lines, summary, ev, adc, iq_l, 2, 8, 4, True)
    np.testing.assert_array_equal(mref.feedline_traces_st(states, cfg, pairs, lines, summary, ev, adc, iq_l, 2, 8, 4, True),
                                  tr)
    assert not np.array_equal(mref.feedline_traces_st(states ^ 3, cfg, pairs, lines, summary, ev, adc, iq_l, 2, 8, 4, True),
                              tr)
    _, acc, result = feedline_ref.feedline(cfg, pairs, lines, summary, ev, iq_d, iq_l, 2)
    # the run layout (columns = lanes: the pairs' columns brought to lane order, the per-lane words as they
    # are) and explicit columns (the words gathered to the pairs' lanes)
    lane = np.asarray(pairs['lane'])
    acc_l, cnt_l = np.zeros_like(acc), np.zeros(n, np.int64)
    acc_l[:, lane], cnt_l[lane] = acc, result[:, 0]
    for a, cnt, st, kw in ((acc_l, cnt_l, states, dict(shot_begin=5)),
                           (acc, result[:, 0], states[lane], dict(core=pairs['core'], shot=pairs['shot']))):
        want = iq_stats_ref.iq_stats(cfg, a, cnt, by_slot=True, **kw)
        got = mref.iq_stats_st(st, cfg, a, cnt, by_slot=True, **kw)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[1], want[1])
        other = mref.iq_stats_st(st ^ 3, cfg, a, cnt, by_slot=True, **kw)
        assert not np.array_equal(other[0], want[0]) and np.array_equal(other[1], want[1])
    # the wrappers leave the base references as they found them
    assert feedline_ref.state(cfg, 5, 0, 0) == int(words[0] & 1)


# ---- 5. the Python helpers ----

def test_state_bits_and_readout_survival():
    words = np.arange(12, dtype=np.uint32)
    cm = _abi.make_config(4, lane_order=_abi.LANES_CORE_MAJOR)
    sm = _abi.make_config(4, lane_order=_abi.LANES_SHOT_MAJOR)
    assert qsim.state_bits(words, cm, 3).tolist() == [[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 10, 11]]
    assert qsim.state_bits(words.view(np.int32), sm, 3).tolist() == [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7, 11]]
    with pytest.raises(ValueError):
        qsim.state_bits(words, cm, 4)
    bits = np.array([[0, 0, 1, 0], [0, 2, 0, 0], [1, 1, 1, 1], [0, 0, 0, 2]], np.uint32)
    reg = np.array([[0, 1], [3, _abi.QSIM_NO_CORE]], np.uint32)
    assert qsim.readout_survival(bits, reg, 2).tolist() == [1.0, 0.5]
    assert qsim.readout_survival(bits, reg, 4, slot=1).tolist() == [0.5]
    res = np.stack([np.full_like(bits, 2), bits], axis=2).astype(np.int32)          # a result table: {count, bits}
    assert qsim.readout_survival(res, reg, 2).tolist() == [1.0, 0.5]
    with pytest.raises(ValueError):
        qsim.readout_survival(bits, reg, 3)


# ---- 6. the C ABI's refusals that need no device work ----

@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_meas_plan(tmp_path):
    """the two conditions dpemu_qsim_meas adds are decided by the host plan: its stand-alone CPU driver"""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    exe = str(tmp_path / 'qsim_meas_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'qsim_meas_plan_test.cpp')],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    m = re.fullmatch(r'ok (\d+)\n', r.stdout)
    assert m and int(m.group(1)) > 50, r.stdout[-2000:]


def test_refusals_before_any_device_work():
    """a context cannot be made without a GPU, and every argument check follows the context check: with the
    library alone, what can be refused is the NULL context (the states == NULL refusal and the plan's through
    the C ABI are in tests/test_gpu_qsim_meas.py)"""
    from distributed_processor_amd._native import load_library
    L = load_library()
    assert L.dpemu_qsim_meas(None, None, None, None, None, None, None, None, None) == -22
    assert L.dpemu_feedline_adc_st(None, *([None] * 9)) == -22
    assert L.dpemu_feedline_adc_res_st(None, *([None] * 10)) == -22
    assert L.dpemu_feedline_traces_st(None, *([None] * 11)) == -22
    assert L.dpemu_iq_stats_st(None, *([None] * 8)) == -22
    assert C.sizeof(C.c_void_p) == 8


# ---- the measuring 64-register inputs of tests/test_gpu_qsim_meas.py ----------------------------------------------

@pytest.mark.parametrize('n_shots', [1, 5, 37])
@pytest.mark.parametrize('which', ['1q', '2q'])
def test_wide_cases_reach_every_slot_window(which, n_shots):
    from tests.test_gpu_qsim import ORDERS, wide_seed
    from tests.test_gpu_qsim_meas import wide_meas_reference
    from tests.test_qsim import check_wide_reach
    for lane_order in ORDERS:
        pops, res, states = wide_meas_reference(which, n_shots, lane_order, wide_seed(which, n_shots) + 1000)
        check_wide_reach(which, n_shots, res[:, :, 1])
        assert states.shape == (64 * n_shots,) and (states != 0).sum() >= 10 * min(n_shots, 5)
