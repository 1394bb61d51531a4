"""GPU tests of the qubit-state stage (dpemu_qsim, include/dpemu.h; qsim.hip):
qsim_kernel against tests/qsim_ref.py on every word of pops and result --
behind dpemu_run on config 4, and on hand-built event records the pipeline
never produces (tests/handbuilt.py's style: explicit records, explicit
reach-conditions checked on the reference)."""

import ctypes as C
import functools

import numpy as np
import pytest

from distributed_processor_amd import _abi, qsim, workloads
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.emulator import Emulator, alloc_device_outputs
from tests import qsim_ref
from tests.handbuilt import random_words
from tests.test_qsim import NEAR_ONE, ONE

pytestmark = pytest.mark.gpu

ORDERS = [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR]
LIM = (1 << 31) - 1


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.array(a, order='C')                          # a writable copy: the cached records are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(pops, result):
    import torch
    torch.cuda.synchronize()
    return pops.cpu().numpy().view(np.uint64), result.cpu().numpy().view(np.uint32)


def assert_same(got, want):
    for g, w, name in zip(got, want, ('pops', 'result')):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(g, w, err_msg=name)


# ---- behind dpemu_run ----

@pytest.mark.parametrize('lane_order', ORDERS, ids=['core_major', 'shot_major'])
def test_pipeline_config4(emu, lane_order):
    """config 4, 8 sequences x 3 shots from shot 5 on 4 cores (two registers): errors, over-rotation and a
    detuning per core; then the ideal gate set, where every row returns to |00>"""
    n_seq, depth, n_cores, n_shots, shot0 = 8, 12, 4, 24, 5
    ps = workloads.config4_rb2q_set(n_seq=n_seq, depth=depth, n_cores=n_cores)
    cfg = _abi.make_config(n_cores, n_groups=n_seq, shots_per_group=3, max_cycles=1 << 22, event_cap=8 * depth + 16,
                           meas_cap=2, lane_order=lane_order, seed=0xA5EED)
    emu.load(ps)
    outs = alloc_device_outputs(cfg, n_shots, want=('summary', 'events'))
    emu.run_device(cfg, n_shots, shot0, outs)
    gs = workloads.rb2q_gateset(n_cores, over_rotation=0.02, err_1q=2.0 ** -5, err_2q=2.0 ** -4)
    for c in range(n_cores):
        gs.set_detune(c, (3 + c) * 2.0 ** -14)
    got = host(*emu.simulate_gates(cfg, gs, outs, n_shots, shot_begin=shot0))
    assert emu.last_kernel() == 'qsim_kernel'
    summary, ev = outs['summary'].cpu().numpy(), outs['events'].cpu().numpy()
    want = qsim_ref.qsim_gateset(cfg, gs, summary, ev, n_shots, shot0)
    assert_same(got, want)
    assert (want[1][:, :, 1] > 50).all() and (want[1][:, :, 2] == 0).all() and (want[1][:, :, 3] > 0).sum() > 10
    ideal = workloads.rb2q_gateset(n_cores)
    got = host(*emu.simulate_gates(cfg, ideal, outs, n_shots, shot_begin=shot0))
    assert_same(got, qsim_ref.qsim_gateset(cfg, ideal, summary, ev, n_shots, shot0))
    assert (got[0][:, :, 0] >= NEAR_ONE).all() and (got[1][:, :, 0] == 0).all() and (got[1][:, :, 2:] == 0).all()


# ---- hand-built records ----

C_HAND, CAP_HAND = 8, 24
REGS_HAND = [(0, 1), 3, (5, 2), 6]                      # two two-qubit registers (one with first > second), two of one
PHASES = (0, 1, 255, 256, 0x7FFF, 0x8000, 0x1FFFF)
ENV = 0x040000


def hand_entries(core):
    """dictionary entries of a core in hand_gateset (the non-unitary one of core 3 apart)"""
    return 8 if core == 0 else 3


def hand_gateset(always_err=False, regs=None, entries=hand_entries, drv_elem=0):
    """up to 8 entries per core; keys (freq, ENV, amp); the non-unitary entry sits on core 3.  ``regs``: other
    registers than REGS_HAND -- ``entries(core)`` rotations for each of their cores, a ZX in place of the second on
    the first core of every two-qubit register, a detuning word per core"""
    gs = qsim.GateSet(drv_elem=drv_elem)
    thr = (lambda k: 0xFFFFFFFF) if always_err else (lambda k: (0, 1 << 30, 0xFFFFFFFF, 1 << 28)[k % 4])
    rng = np.random.default_rng(77)
    second = {0: 1, 5: 2} if regs is None else {r[0]: r[1] for r in regs if isinstance(r, tuple)}
    cores = (0, 1, 2, 3, 5, 6) if regs is None else sorted(c for r in regs for c in (r if isinstance(r, tuple) else (r,)))
    for core in cores:
        for k in range(entries(core)):
            if k == 1 and core in second:
                gs.add_zx(core, second[core], k, ENV, 100 + core, 1.3 + core)
                gs.entries[-1]['err_thr'] = thr(k + core)
            else:
                gs.add_matrix(core, k, ENV, 100 + core, qsim.rotation(rng.uniform(0, 6.0), rng.uniform(0, 1.0)),
                              err_thr=thr(k + core))
    s = ONE
    gs.add_matrix(3, 9, ENV, 103, np.array([s, -s, s, s, -s, s, s, -s]),      # |row| = 2: the state grows
                  err_thr=0xFFFFFFFF if always_err else 0)
    for c, d in ((0, 0x00012345), (1, 0xFFF00001), (2, 0x80000001), (3, 0x7FFFFFFF), (5, 0x0000BEEF), (6, 0xDEADBEEF)):
        gs.detune[c] = d
    if regs is not None:
        for c in cores:
            gs.detune.setdefault(c, int(rng.integers(0, 2 ** 32)))
    return gs.registers(REGS_HAND if regs is None else list(regs))


@functools.lru_cache(maxsize=None)
def hand_records(n_shots, lane_order, t0, seed, n_cores=C_HAND, entries=hand_entries):
    """summary / events of n_shots x n_cores lanes: per lane 0 .. CAP_HAND + 3 records (so empty lanes, and lanes
    over event_cap) in nondecreasing time from t0 with steps of 0..3 clocks (ties between the lanes of a register
    are common) -- drive strobes with a dictionary key (one of the core's ``entries(core)``), an unmatched key or
    the non-unitary entry, strobes of other elements, pulse_resets and records of kind >= 2; every slot past the
    count holds garbage"""
    rng = np.random.default_rng(seed)
    n_lanes = n_shots * n_cores
    summary = random_words(rng, (n_lanes, 8))
    ev = random_words(rng, (CAP_HAND, n_lanes, 4))
    for sl in range(n_shots):
        for core in range(n_cores):
            lane = sl * n_cores + core if lane_order == _abi.LANES_SHOT_MAJOR else core * n_shots + sl
            n = int(rng.choice([0, CAP_HAND + 3, rng.integers(1, CAP_HAND + 1)], p=[0.1, 0.15, 0.75]))
            summary[lane, 2] = n
            t = t0
            for k in range(min(n, CAP_HAND)):
                t += int(rng.integers(0, 4))
                what = rng.random()
                phase = int(PHASES[rng.integers(0, len(PHASES))] if rng.random() < 0.7 else rng.integers(0, 1 << 17))
                freq, cfgw, kind = int(rng.integers(0, entries(core))), int(rng.integers(0, 4)) << 2, 0
                if what < 0.08:
                    freq = 11                            # no such key
                elif what < 0.2 and core == 3:
                    freq = 9                             # the non-unitary entry
                elif what < 0.3:
                    cfgw |= int(rng.integers(1, 4))      # another element
                elif what < 0.4:
                    kind = int(rng.choice([1, 1, 2, 9, 15]))
                ev[k, lane] = (t & 0xFFFFFFFF, ENV | (cfgw << 24) | (kind << 28), phase | (freq << 17),
                               (100 + core) | (int(rng.integers(0, 1 << 16)) << 16))
    summary.setflags(write=False)
    ev.setflags(write=False)
    return summary, ev


def hand_cfg(lane_order, seed=0x51C0FFEE12345678, n_cores=C_HAND):
    return _abi.make_config(n_cores, event_cap=CAP_HAND, lane_order=lane_order, seed=seed)


@functools.lru_cache(maxsize=None)
def hand_reference(n_shots, lane_order, t0, seed, always_err=False, shot0=2 ** 32 - 30):
    summary, ev = hand_records(n_shots, lane_order, t0, seed)
    states = []
    pops, res = qsim_ref.qsim_gateset(hand_cfg(lane_order), hand_gateset(always_err), summary, ev, n_shots, shot0,
                                      states=states)
    return pops, res, states


@pytest.mark.parametrize('lane_order', ORDERS, ids=['core_major', 'shot_major'])
def test_handbuilt_records(emu, lane_order):
    """70 shots x 4 registers = 280 rows: two workgroups, a partly filled last wave; shots across 2^32"""
    n_shots, shot0 = 70, 2 ** 32 - 30
    summary, ev = hand_records(n_shots, lane_order, 5, 11)
    pops, res, states = hand_reference(n_shots, lane_order, 5, 11)
    # what the records were built to reach, on the reference
    assert (res[:, :, 3] >> 31).any() and not (res[:, :, 3] >> 31).all()              # a lane over event_cap
    assert (res[:, :, 2] > 0).any() and (res[:, :, 1] == 0).any()                     # unmatched pulses; rows without a gate
    assert ((res[:, :, 3] & 0xFFFF) > 0).any() and (res[[1, 3], :, 0] <= 1).all()     # errors; one-qubit outcomes
    assert max(abs(v) for x in states for c in x for v in c) == LIM                   # the clamp acted
    assert len(np.unique(res[:, :, 0])) == 4
    times = [[{r[0] for r in qsim_ref.drive_strobes(summary, ev, qsim_ref.lane_of(hand_cfg(lane_order), s, c, n_shots),
                                                     CAP_HAND, 0)} for s in range(n_shots)] for c in (0, 1)]
    assert sum(1 for a, b in zip(*times) if a & b) > 10                               # equal-t ties between the lanes
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    got = host(*emu.simulate_gates(hand_cfg(lane_order), hand_gateset(), outs, n_shots, shot_begin=shot0))
    assert_same(got, (pops, res))


def test_handbuilt_edges(emu):
    """one shot; t around 2^31 under the detunings (the 64-bit phase product, the unsigned merge); an error after
    every gate"""
    import torch
    for n_shots, t0, seed, always in ((1, 5, 21, False), (9, 2 ** 31 - 40, 22, False), (9, 2 ** 32 - 30, 23, False),
                                      (33, 5, 24, True)):
        order = _abi.LANES_CORE_MAJOR
        summary, ev = hand_records(n_shots, order, t0, seed)
        pops, res, _ = hand_reference(n_shots, order, t0, seed, always, shot0=7)
        if always:
            assert ((res[:, :, 3] & 0xFFFF) == res[:, :, 1]).all() and (res[:, :, 1] > 0).any()
        assert (res[:, :, 1] > 0).any()
        outs = dict(summary=to_dev(summary), events=to_dev(ev))
        # caller-made outputs, full of garbage
        p_buf = torch.full((4, n_shots, 4), 0x5A5A5A5A5A5A, dtype=torch.int64, device='cuda')
        r_buf = torch.full((4, n_shots, 4), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
        p2, r2 = emu.simulate_gates(hand_cfg(order), hand_gateset(always), outs, n_shots, shot_begin=7, pops=p_buf,
                                    result=r_buf)
        assert p2 is p_buf and r2 is r_buf
        assert_same(host(p2, r2), (pops, res))


# ---- 64 registers: the dictionary slots of every register in one workgroup's LDS ----

C_WIDE = 64
WIDE_SHOTS = (1, 5, 37)                                 # 256 rows span all 64, 52 and 7..8 registers


def wide_entries(core):
    """1 .. 8 dictionary entries per core"""
    return 1 + (5 * core + 3) % 8


@functools.lru_cache(maxsize=None)
def wide_regs(which):
    """'1q': 64 one-qubit registers; '2q': 32 two-qubit registers, about half with first core > second -- the 64
    cores in shuffled order"""
    order = np.random.default_rng(640).permutation(C_WIDE).tolist()
    return tuple(order) if which == '1q' else tuple((order[2 * r], order[2 * r + 1]) for r in range(C_WIDE // 2))


def wide_gateset(which, always_err=False, drv_elem=0):
    return hand_gateset(always_err, wide_regs(which), wide_entries, drv_elem)


def wide_records(n_shots, lane_order, seed):
    return hand_records(n_shots, lane_order, 5, seed, C_WIDE, wide_entries)


@functools.lru_cache(maxsize=None)
def wide_reference(which, n_shots, lane_order, seed, shot0=2 ** 32 - 30):
    summary, ev = wide_records(n_shots, lane_order, seed)
    return qsim_ref.qsim_gateset(hand_cfg(lane_order, n_cores=C_WIDE), wide_gateset(which), summary, ev, n_shots, shot0)


def wide_seed(which, n_shots):
    return 6400 + 100 * (which == '2q') + n_shots


def wide_windows(which, n_shots):
    """per workgroup of 256 rows (first register, last register, first slot, end slot) as qsim_kernel finds them,
    the slots of every register, and the dynamic LDS bytes plan_qsim grants (restated from its comment)"""
    regs = wide_regs(which)
    slot_first = np.concatenate([[0], np.cumsum([2 if isinstance(r, tuple) else 1 for r in regs])]).tolist()
    n_rows = len(regs) * n_shots
    wgs = []
    for row0 in range(0, n_rows, 256):
        r_lo, r_hi = row0 // n_shots, (min(row0 + 256, n_rows) - 1) // n_shots
        wgs.append((r_lo, r_hi, slot_first[r_lo], slot_first[r_hi + 1]))
    span = min(len(regs), 255 // n_shots + 2)
    most = max(slot_first[r + span] - slot_first[r] for r in range(len(regs) - span + 1))
    return wgs, slot_first, (1536 + most * 176) * 4


@pytest.mark.parametrize('n_shots', WIDE_SHOTS)
@pytest.mark.parametrize('lane_order', ORDERS, ids=['core_major', 'shot_major'])
@pytest.mark.parametrize('which', ['1q', '2q'])
def test_64_registers(emu, which, lane_order, n_shots):
    """cores_per_shot 64 in 64 one-qubit or 32 two-qubit registers, 1 .. 8 entries per core: a workgroup stages up
    to all 64 dictionary slots (51,200 B of LDS) from a window of the table that starts at its own first
    register's.  Reach: tests/test_qsim.py test_wide_cases_reach_every_slot_window"""
    seed, shot0 = wide_seed(which, n_shots), 2 ** 32 - 30
    summary, ev = wide_records(n_shots, lane_order, seed)
    want = wide_reference(which, n_shots, lane_order, seed)
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    got = host(*emu.simulate_gates(hand_cfg(lane_order, n_cores=C_WIDE), wide_gateset(which), outs, n_shots,
                                   shot_begin=shot0))
    assert emu.last_kernel() == 'qsim_kernel'
    assert_same(got, want)


# ---- the C ABI's checks, n_shots = 0, naming, timing, streams ----

def test_refusals_at_the_c_abi(emu):
    """every argument check: -22 and a message, before any launch"""
    import torch
    n_shots, order = 4, _abi.LANES_CORE_MAJOR
    cfg = hand_cfg(order)
    summary, ev = hand_records(n_shots, order, 5, 31)
    d_sum, d_ev = to_dev(summary), to_dev(ev)
    pops = torch.zeros((4, n_shots, 4), dtype=torch.int64, device='cuda')
    res = torch.zeros((4, n_shots, 4), dtype=torch.int32, device='cuda')

    def call(gs=None, cfg_=cfg, qs=True, ptrs=None, **f):
        st, keep = (gs or hand_gateset()).struct(cfg, n_shots, 0)
        for k, v in f.items():
            setattr(st, k, v)
        p = dict(summary=d_sum.data_ptr(), events=d_ev.data_ptr(), pops=pops.data_ptr(), result=res.data_ptr())
        p.update(ptrs or {})
        rc = emu._L.dpemu_qsim(emu._h, C.addressof(cfg_) if cfg_ is not None else None, C.addressof(st) if qs else None,
                               p['summary'], p['events'], p['pops'], p['result'], None)
        return rc, emu._L.dpemu_last_error(emu._h)

    def edited(fn):
        gs = hand_gateset()
        fn(gs)
        return gs

    def entry(gs, core, k):
        return [e for e in gs.entries if e['core'] == core][k]

    def set_m(gs):
        entry(gs, 2, 0)['m'][1, 5] = ONE + 1

    def set_m_neg(gs):
        entry(gs, 2, 0)['m'][0, 0] = -ONE - 1

    assert call()[0] == 0
    torch.cuda.synchronize()
    pops.zero_()
    res.zero_()
    bad_c = hand_cfg(order)
    bad_c.cores_per_shot = 6
    cases = [
        (dict(cfg_=None), b'cfg'), (dict(qs=False), b'qs'), (dict(ptrs=dict(summary=None)), b'summary'),
        (dict(ptrs=dict(events=None)), b'events'), (dict(ptrs=dict(pops=None)), b'pops'),
        (dict(ptrs=dict(result=None)), b'result'), (dict(reg_core=None), b'reg_core'), (dict(gates=None), b'gates'),
        (dict(n_regs=0), b'n_regs'),
        (dict(gs=hand_gateset().registers([(0, 1), 3, (5, 2), 8])), b'core 8'),
        (dict(gs=hand_gateset().registers([(0, 1), 3, (5, 2), 6, 1])), b'two registers'),
        (dict(gs=hand_gateset().registers([(0, 1), 3, (5, 2), 6, (4, 4)])), b'two registers'),
        (dict(gs=edited(lambda g: g.add_rotation(0, 50, ENV, 1, 1.0))), b'entries for core 0'),
        (dict(gs=edited(lambda g: g.add_rotation(1, 2, ENV, 101, 1.0))), b'key'),
        (dict(gs=edited(lambda g: entry(g, 1, 0).update(kind=2))), b'kind'),
        (dict(gs=edited(lambda g: entry(g, 1, 0).update(kind=1))), b'kind 1'),       # the second core of (0, 1)
        (dict(gs=edited(lambda g: entry(g, 3, 0).update(kind=1))), b'kind 1'),       # a one-qubit register
        (dict(gs=edited(lambda g: g.add_rotation(4, 0, ENV, 1, 1.0))), b'no register'),
        (dict(gs=edited(lambda g: g.add_rotation(8, 0, ENV, 1, 1.0))), b'no register'),
        (dict(gs=edited(set_m)), b'2^30'), (dict(gs=edited(set_m_neg)), b'2^30'),
        (dict(drv_elem=4), b'drv_elem'), (dict(event_cap=_abi.MAX_EVENT_CAP + 1), b'event_cap'),
        (dict(n_lanes=n_shots * C_HAND + 1), b'n_lanes'), (dict(n_shots=n_shots + 1), b'n_lanes'),
        (dict(cfg_=bad_c), b'cores_per_shot'), (dict(ptrs=dict(result=res.data_ptr() + 4)), b'aligned'),
    ]
    for kw, field in cases:
        rc, msg = call(**kw)
        assert rc == -22 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert not pops.any().item() and not res.any().item()             # nothing was launched
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, hand_gateset(), dict(summary=d_sum, events=d_ev), n_shots + 1)
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, hand_gateset(), dict(summary=d_sum, events=d_ev), n_shots, result=res[:3])
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, hand_gateset(), dict(summary=d_sum), n_shots)


def test_no_shots_name_and_timing(emu):
    import torch
    n_shots, order = 5, _abi.LANES_SHOT_MAJOR
    cfg = hand_cfg(order)
    summary, ev = hand_records(n_shots, order, 5, 41)
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        # no shots: accepted, nothing launched, nothing timed -- the tables are still checked
        pops, res = emu.simulate_gates(cfg, hand_gateset(), {}, 0)
        assert tuple(pops.shape) == (4, 0, 4) and tuple(res.shape) == (4, 0, 4)
        assert emu.kernel_times() == []
        with pytest.raises(DpemuError):
            emu.simulate_gates(cfg, hand_gateset().registers([(0, 1), 3, (5, 2), 6, 1]), {}, 0)
        got = host(*emu.simulate_gates(cfg, hand_gateset(), outs, n_shots, shot_begin=3))
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 1 and 0 < ms[0] < 100
    assert emu.last_kernel() == 'qsim_kernel'
    assert_same(got, qsim_ref.qsim_gateset(cfg, hand_gateset(), summary, ev, n_shots, 3))
    torch.cuda.synchronize()


def test_ordered_across_streams(emu):
    """a run on one stream, simulate_gates on another with nothing between them: the context orders its calls"""
    import torch
    n_seq, depth, n_shots = 6, 12, 12
    ps = workloads.config4_rb2q_set(n_seq=n_seq, depth=depth, n_cores=2)
    cfg = _abi.make_config(2, n_groups=n_seq, shots_per_group=2, max_cycles=1 << 22, event_cap=8 * depth + 16, meas_cap=2,
                           seed=0xBEE5)
    emu.load(ps)
    outs = alloc_device_outputs(cfg, n_shots, want=('summary', 'events'))
    for t in outs.values():
        t.zero_()
    torch.cuda.synchronize()
    a, b = torch.cuda.Stream(), torch.cuda.Stream()
    gs = workloads.rb2q_gateset(2, over_rotation=0.05, err_1q=2.0 ** -6, err_2q=2.0 ** -4)
    emu.run_device(cfg, n_shots, 0, outs, stream=a)
    pops, res = emu.simulate_gates(cfg, gs, outs, n_shots, stream=b)
    b.synchronize()
    got = host(pops, res)
    want = qsim_ref.qsim_gateset(cfg, gs, outs['summary'].cpu().numpy(), outs['events'].cpu().numpy(), n_shots)
    assert_same(got, want)
    assert (want[1][:, :, 1] > 50).all()
