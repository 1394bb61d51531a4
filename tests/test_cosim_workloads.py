"""CPU tests of the co-simulation workloads (workloads.cosim_active_reset,
workloads.cosim_bell_feedback): the qubit half of what tests/test_gpu_cosim.py
asserts on the GPU, through the Python-integer reference tests/qsim_meas_ref.py
on event records written by hand from the workloads' own pulse commands -- no
interpreter runs here.

* a qubit collapsed to |1> and driven by the gate set's X90 X90 is left with a
  |1> population below 2^-40 of the total, so a readout of it reads 1 only when
  its 32-bit draw u satisfies floor(u T / 2^32) >= T - A, i.e. never (u < 2^32
  and A < T / 2^40): "the second readout is 0 in every shot" cannot fail by chance;
* the Bell workload's pulses make the two first readouts agree, and with the
  conditional X180 played where the control read 1 the target's second readout
  is 0 and the control's repeats;
* the builders leave config3_active_reset's bytes as they were."""

import hashlib

import numpy as np

from distributed_processor_amd import _abi, isa, workloads
from tests import qsim_meas_ref as mref
from tests.test_qsim import hand_events, strobe

SEED = 0xC051
RDLO = workloads.RDLO


def cfg_of(C_, cap):
    return _abi.make_config(C_, event_cap=cap, seed=SEED, meas_elem=RDLO)


def segments(cmd_buf):
    """the pulse strobes of one core's program as hand records, cut where the control flow is: [before the
    branch (jump_i)], [the conditional block: between jump_i and the second sync], [after that sync]; a program
    without a branch has the first and the last.
    t = cmd_time: every segment starts from a qclk reset common to the shot's cores"""
    segs, cur, n_sync = [], [], 0
    for w in isa.bytes_to_words(cmd_buf):
        d = isa.decode(w)
        n_sync += d['op'] == 'sync'
        if d['op'] == 'jump_i' or (d['op'] == 'sync' and n_sync == 2):
            segs.append(cur)
            cur = []
        elif d['op'] == 'pulse_write_trig':
            cur.append(strobe(d['cmd_time'], d['freq'], d['env_word'], d['amp'], d['phase'], elem=d['cfg'] & 3))
    segs.append(cur)
    return segs


def ref(cfg, gs, lanes, n_shots):
    summary, ev = hand_events(lanes, cfg.event_cap)
    return mref.qsim_meas_gateset(cfg, gs, summary, ev, n_shots, event_cap=cfg.event_cap)


def later(recs, dt):
    return [(r[0] + dt,) + r[1:] for r in recs]


def test_x180_after_collapse_to_one_leaves_no_one_population():
    prog, gs = workloads.cosim_active_reset(8, prep=2)
    assert gs.n_regs == 8 and len(gs.entries) == 8 and all(e['kind'] == 0 for e in gs.entries)
    cfg = cfg_of(8, 16)
    lanes = []
    for c in range(8):
        first, cond, second = segments(prog[str(c)]['cmd_buf'])
        assert [r[1] >> 24 for r in first] == [0, 0, 1, 2] and [r[1] >> 24 for r in cond] == [0, 0]
        assert [r[1] >> 24 for r in second] == [1, 2]
        # prep = 2 is an X180: the first readout collapses to |1>; then the conditional X90 X90; no second readout,
        # so the final populations are the state the second readout would measure
        lanes.append(first + later(cond, 10000))
    pops, res, states = ref(cfg, gs, lanes, 1)
    assert (states == 1).all() and (res[:, 0, 1] == 4).all() and (res[:, 0, 2:] == 0).all()
    for c in range(8):
        P = [int(v) for v in pops[c, 0]]
        one, tot = P[2] + P[3], sum(P)          # a one-qubit register: the first core's bit is the high one
        assert tot >= 1 << 58 and one << 40 < tot, (c, P)
        assert res[c, 0, 0] == 0


def test_active_reset_prep_one_is_a_fair_coin_and_resets():
    """prep = 1 by hand: X90, readout, then X90 X90 in the shots that read 1, readout: bit 0 fair, bit 1 zero"""
    n = 256
    prog, gs = workloads.cosim_active_reset(2, prep=1)
    cfg = cfg_of(2, 16)
    segs = [segments(prog[str(c)]['cmd_buf']) for c in range(2)]
    lanes = [segs[c][0] for c in range(2) for _ in range(n)]
    bit0 = ref(cfg, gs, lanes, n)[2] & 1
    k = int(bit0.sum())
    assert abs(k / (2 * n) - 0.5) <= 5 / (2 * np.sqrt(2 * n)), k          # five standard deviations of the binomial
    lanes = [segs[c][0] + (later(segs[c][1], 10000) if bit0[c * n + s] else []) + later(segs[c][2], 20000)
             for c in range(2) for s in range(n)]
    states = ref(cfg, gs, lanes, n)[2]
    assert ((states & 1) == bit0).all() and (states >> 1 == 0).all()


def test_bell_feedback_pulses_correlate_the_pair():
    n = 128
    prog, gs = workloads.cosim_bell_feedback()
    assert [tuple(int(v) for v in r) for r in gs.reg_core] == [(0, 1)]
    cfg = cfg_of(2, 16)
    segs = [segments(prog[str(c)]['cmd_buf']) for c in range(2)]
    assert [len(s) for s in segs[0]] == [4, 2] and [len(s) for s in segs[1]] == [3, 2, 2]   # the control has no branch
    keys = gs.keys()
    for c in range(2):
        for s in segs[c]:
            assert all((c, r[2] >> 17, r[1] & 0xFFFFFF, r[3]) in keys for r in s if r[1] >> 24 == 0), (c, s)
    lanes = [segs[c][0] for c in range(2) for _ in range(n)]
    _, res, states = ref(cfg, gs, lanes, n)
    a, b = states[:n], states[n:]
    assert (a == b).all() and set(a.tolist()) == {0, 1}                 # the two first readouts agree
    assert (res[0, :, 1] == 3).all() and (res[0, :, 2] == 0).all()      # three gates, every pulse in the dictionary
    # the feedback by hand: the target plays its conditional X90 X90 where the CONTROL read 1
    lanes = [segs[0][0] + later(segs[0][1], 20000) for _ in range(n)]
    lanes += [segs[1][0] + (later(segs[1][1], 10000) if a[s] else []) + later(segs[1][2], 20000) for s in range(n)]
    pops, res, states = ref(cfg, gs, lanes, n)
    c0, c1 = states[:n], states[n:]
    assert ((c0 & 1) == a).all() and ((c0 >> 1) == a).all()             # the control's second repeats its first
    assert ((c1 & 1) == a).all() and (c1 >> 1 == 0).all()               # the target is reset
    for s in range(n):
        P = [int(v) for v in pops[0, s]]
        assert (P[1] + P[3]) << 40 < sum(P), (s, P)                      # the target's |1> population


def test_builders_leave_config3_alone():
    """config3_active_reset's machine code and buffers, pinned by digest, before and after the new builders ran"""
    def digest():
        h = hashlib.sha256()
        for kw in (dict(), dict(n_cores=4, extra_pulses=3), dict(read_shift=1)):
            p = workloads.config3_active_reset(**kw)
            for c in sorted(p, key=int):
                h.update(p[c]['cmd_buf'])
                for k in ('env_buffers', 'freq_buffers'):
                    for b in p[c][k]:
                        h.update(b)
        return h.hexdigest()
    before = digest()
    workloads.cosim_active_reset(8, prep=1, read_shift=3)
    workloads.cosim_bell_feedback()
    assert digest() == before
    # prep = 0 differs from config 3 only in nothing: the same commands (the builder is config 3 with a preparation)
    p0, _ = workloads.cosim_active_reset(8, prep=0, read_shift=1)
    want = workloads.config3_active_reset(8, read_shift=1)
    assert {c: p0[c]['cmd_buf'] for c in p0} == {c: want[c]['cmd_buf'] for c in want}
