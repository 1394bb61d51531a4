"""GPU tests of the decaying qubit-state stage (dpemu_qsim_decay, include/dpemu.h):
qsim_kernel<decay> and qsim_kernel<meas,decay> against tests/qsim_decay_ref.py on
every word of pops, result, states and counts over hand-built records -- one- and
two-qubit registers over two workgroups, both lane orders, event times up to
2^32 - 1, 64 cores with a table per core -- the identity tables against the base
calls on the device, the Ramsey workload behind dpemu_run against its
exponential, and the co-simulation loop with decaying qubits."""

import ctypes as C
import functools

import numpy as np
import pytest

from distributed_processor_amd import _abi, qsim, workloads
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from tests import qsim_decay_ref as dref
from tests import test_gpu_qsim as tq
from tests import test_gpu_qsim_meas as tm

pytestmark = pytest.mark.gpu

CM, SM = _abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR
ORDERS = [CM, SM]
ORDER_IDS = ['core_major', 'shot_major']
ONE = 1 << 30
SHOT0 = 2 ** 32 - 30                                    # the shots of every bit-exact case run across 2^32
T_MAX = 2 ** 32 - 1


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.array(a, order='C')
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def u32(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy().view(np.uint32)


def stretched(ev, mult):
    """the records with every time t replaced by min(t mult, 2^32 - 1): order and ties stay, the gaps reach bit 16
    and above"""
    ev = np.array(ev)
    ev[:, :, 0] = np.minimum(ev[:, :, 0].astype(np.uint64) * np.uint64(mult), np.uint64(T_MAX)).astype(np.uint32)
    ev.setflags(write=False)
    return ev


def kept_t_max(summary, ev, cap):
    """the largest time among the records below their lane's count and ``cap``"""
    n = np.minimum(np.asarray(summary).view(np.uint32).reshape(-1, 8)[:, 2], cap)
    kept = np.arange(ev.shape[0])[:, None] < n[None, :]
    return int(ev[:, :, 0][kept].max())


def with_decay(gs, times):
    """``gs`` with the decay of {core: (t1, t2)}"""
    for c, (t1, t2) in times.items():
        gs.set_decay(c, t1, t2)
    return gs


def run_decay(emu, cfg, gs, summary, ev, n_shots, measure, t_final, want_counts=True, shot0=SHOT0):
    """simulate_gates through dpemu_qsim_decay on caller-made buffers full of garbage -> (pops, result, states,
    counts) on the host, states / counts None where they are not asked for"""
    import torch
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    counts = torch.full((gs.n_regs, n_shots, 4), 0x5A5A5A5A, dtype=torch.int32, device='cuda') if want_counts else None
    states = torch.full((n_shots * cfg.cores_per_shot,), 0x5A5A5A5A, dtype=torch.int32, device='cuda') if measure else None
    got = emu.simulate_gates(cfg, gs, outs, n_shots, shot_begin=shot0, measure=measure, states=states, t_final=t_final,
                             decay_counts=counts)
    assert len(got) == (3 if measure else 2) and (not measure or got[2] is states)
    assert emu.last_kernel() == ('qsim_kernel<meas,decay>' if measure else 'qsim_kernel<decay>')
    torch.cuda.synchronize()
    return (got[0].cpu().numpy().view(np.uint64), u32(got[1]), u32(states) if measure else None,
            u32(counts) if want_counts else None)


def assert_same(got, want):
    for g, w, name in zip(got, want, ('pops', 'result', 'states', 'counts')):
        if g is None:
            continue
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(g, w, err_msg=name)


# ---- 1. with readouts: a two- and a one-qubit register of 4 cores, 260 rows over two workgroups ----

FUZZ_SHOTS = 130
FUZZ_TIMES = {0: (2.0 ** 31, 2.0 ** 30), 1: (3e8, 2e8), 2: (5e7, 2e7)}     # core 3 is in no register


@functools.lru_cache(maxsize=None)
def fuzz_case(lane_order):
    summary, ev = tm.fuzz_records(FUZZ_SHOTS, lane_order, 500 + lane_order)
    ev = stretched(ev, T_MAX // kept_t_max(summary, ev, tm.CAP_FUZZ) + 1)      # the last kept record lands on 2^32 - 1
    cfg, gs = tm.fuzz_cfg(lane_order), with_decay(tm.fuzz_gateset(), FUZZ_TIMES)
    advances = []
    want = dref.qsim_decay_gateset(cfg, gs, summary, ev, FUZZ_SHOTS, SHOT0, measure_readouts=True, t_final=T_MAX,
                                   advances=advances)
    return cfg, gs, summary, ev, want, advances


def check_fuzz_reach(lane_order):
    cfg, gs, summary, ev, (pops, res, states, counts), advances = fuzz_case(lane_order)
    assert all((counts[r, :, k] > 0).any() for r, k in ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1)))
    assert not counts[1, :, 2:].any()                                                 # a one-qubit register has one qubit
    assert {tag for _, _, tag, _, _, _, _ in advances} == {dref.OWN_CTR, dref.TARGET_CTR, dref.FINAL_CTR}
    assert max(dt for _, _, _, _, dt, _, _ in advances) >= 1 << 31 and any((dt >> 16) & 0xFF for _, _, _, _, dt, _, _ in advances)
    per_row = {}
    for row, core, tag, n, _, _, _ in advances:
        per_row.setdefault(row, set()).add((core, tag, n))
    # the target advanced by the control's record k and by its own lane's record k: the tags keep the counters apart
    assert sum(1 for v in per_row.values() for c, tag, n in v if tag == dref.TARGET_CTR and (c, dref.OWN_CTR, n) in v) > 5
    assert kept_t_max(summary, ev, tm.CAP_FUZZ) == T_MAX
    assert (res[:, :, 3] >> 31).any() and (res[:, :, 2] > 0).any() and states.any()
    assert len(pops) * FUZZ_SHOTS == 260


@pytest.mark.parametrize('lane_order', ORDERS, ids=ORDER_IDS)
def test_fuzz_with_readouts(emu, lane_order):
    check_fuzz_reach(lane_order)
    cfg, gs, summary, ev, want, _ = fuzz_case(lane_order)
    assert_same(run_decay(emu, cfg, gs, summary, ev, FUZZ_SHOTS, True, T_MAX), want)


# ---- 2. without readouts: 4 registers of 8 cores, 280 rows; times that wrap past 2^32 - 1; no counts ----

HAND_SHOTS = 70
HAND_TIMES = {c: (20 + 3 * c, 9 + 5 * c) for c in (0, 1, 2, 3, 5, 6)}       # the steps of 0..3 clocks matter
HAND_SLOW = {c: (20000 + 3000 * c, 9000 + 5000 * c) for c in (0, 1, 2, 3, 5, 6)}


@functools.lru_cache(maxsize=None)
def hand_case(lane_order):
    """core-major: the records start at t = 2^32 - 40 and wrap, so a lane's later records lie before its clock and
    advance nothing (the first advance, over 2^32 - 40 clocks, has G = E = 0), t_final 0; shot-major: times x 1,000 and a t_final past 2^31"""
    if lane_order == CM:
        summary, ev = tq.hand_records(HAND_SHOTS, lane_order, 2 ** 32 - 40, 31)
        gs, t_final = with_decay(tq.hand_gateset(), HAND_TIMES), 0
    else:
        summary, ev = tq.hand_records(HAND_SHOTS, lane_order, 5, 32)
        ev, gs, t_final = stretched(ev, 1000), with_decay(tq.hand_gateset(), HAND_SLOW), 2 ** 31 + 12345
    cfg = tq.hand_cfg(lane_order)
    advances = []
    want = dref.qsim_decay_gateset(cfg, gs, summary, ev, HAND_SHOTS, SHOT0, t_final=t_final, advances=advances)
    return cfg, gs, summary, ev, t_final, want, advances


def check_hand_reach(lane_order):
    cfg, gs, summary, ev, t_final, (pops, res, states, counts), advances = hand_case(lane_order)
    assert states is None and counts[:, :, 0].any() and counts[:, :, 1].any() and counts[[0, 2]][:, :, 2].any()
    if lane_order == CM:
        assert kept_t_max(summary, ev, tq.CAP_HAND) >= T_MAX - 3
        wrapped = 0                                      # lanes whose kept drive strobes go back in time
        for lane in range(summary.shape[0]):
            t = [r[0] for r in tq.qsim_ref.drive_strobes(summary, ev, lane, tq.CAP_HAND, 0)]
            wrapped += any(b < a for a, b in zip(t, t[1:]))
        assert wrapped > 5
    else:
        assert any(tag == dref.FINAL_CTR and dt > 2 ** 31 for _, _, tag, _, dt, _, _ in advances)


@pytest.mark.parametrize('lane_order', ORDERS, ids=ORDER_IDS)
def test_handbuilt_without_readouts(emu, lane_order):
    check_hand_reach(lane_order)
    cfg, gs, summary, ev, t_final, want, _ = hand_case(lane_order)
    assert_same(run_decay(emu, cfg, gs, summary, ev, HAND_SHOTS, False, t_final, want_counts=lane_order == CM), want)


# ---- 3. 64 cores, every core its own table ----

WIDE_TIMES = {c: (3000 + 500 * c, (3000 + 500 * c) * (0.3 + 1.5 * c / 63)) for c in range(64)}


@functools.lru_cache(maxsize=None)
def wide_case(which):
    """'1q': tests/test_gpu_qsim.py's 64 one-qubit registers x 5 shots (320 rows), no readouts; '2q':
    tests/test_gpu_qsim_meas.py's 32 two-qubit registers x 9 shots (288 rows), measuring"""
    if which == '1q':
        n, order, measure = 5, CM, False
        summary, ev = tq.wide_records(n, order, tq.wide_seed(which, n) + 50)
        cfg, gs = tq.hand_cfg(order, n_cores=tq.C_WIDE), tq.wide_gateset(which)
    else:
        n, order, measure = 9, SM, True
        summary, ev = tm.wide_meas_records(n, order, tq.wide_seed(which, n) + 50)
        cfg, gs = tm.fuzz_cfg(order, tq.C_WIDE, tm.CAP_WIDE), tm.wide_meas_gateset(which)
    ev, gs = stretched(ev, 500), with_decay(gs, WIDE_TIMES)
    want = dref.qsim_decay_gateset(cfg, gs, summary, ev, n, SHOT0, measure_readouts=measure, t_final=60000)
    return cfg, gs, summary, ev, n, measure, want


@pytest.mark.parametrize('which', ['1q', '2q'])
def test_64_cores_with_a_table_each(emu, which):
    cfg, gs, summary, ev, n, measure, want = wide_case(which)
    damp, deph = dref.decay_words(gs, 64)
    assert len({d.tobytes() for d in damp}) == 64 and len({d.tobytes() for d in deph}) == 64
    counts = want[3]
    assert (counts[:, :, 0] > 0).any(axis=1).sum() > len(counts) // 2                 # jumps in most registers
    assert (which == '1q') == (not counts[:, :, 2:].any())
    assert_same(run_decay(emu, cfg, gs, summary, ev, n, measure, 60000), want)


# ---- 4. the identity tables against the base calls, on the device ----

@pytest.mark.parametrize('measure', [False, True], ids=['qsim', 'qsim_meas'])
def test_identity_tables_equal_the_base_call(emu, measure):
    import torch
    cfg, _, summary, ev, _, _ = fuzz_case(CM)
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    base = emu.simulate_gates(cfg, tm.fuzz_gateset(), outs, FUZZ_SHOTS, shot_begin=SHOT0, measure=measure)
    assert emu.last_kernel() == ('qsim_kernel<meas>' if measure else 'qsim_kernel')
    gs = tm.fuzz_gateset()
    gs.decay[1] = tuple(np.full(32, ONE, np.uint32) for _ in range(2))
    counts = torch.full((2, FUZZ_SHOTS, 4), 7, dtype=torch.int32, device='cuda')
    got = emu.simulate_gates(cfg, gs, outs, FUZZ_SHOTS, shot_begin=SHOT0, measure=measure, decay_counts=counts)
    assert emu.last_kernel() == ('qsim_kernel<meas,decay>' if measure else 'qsim_kernel<decay>')
    assert len(got) == len(base) and all(torch.equal(g, b) for g, b in zip(got, base))
    assert not counts.any().item() and base[1][:, :, 1].any().item()


# ---- 5. the C ABI's refusals, no shots, timing ----

def test_refusals_no_shots_and_timing(emu):
    import torch
    cfg, gs, summary, ev, _, _ = fuzz_case(CM)
    n = FUZZ_SHOTS
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    p_buf = torch.full((2, n, 4), 7, dtype=torch.int64, device='cuda')
    bufs = [torch.full(s, 7, dtype=torch.int32, device='cuda') for s in ((2, n, 4), (n * 4,), (2, n, 4))]

    def call(dec_ptr='dec', states=bufs[1].data_ptr(), counts=bufs[2].data_ptr(), edit=None, **f):
        st, keep = gs.struct(cfg, n, SHOT0)
        for k, v in f.items():
            setattr(st, k, v)
        dec, keep_dec = gs.decay_struct(cfg, 1000)
        if edit:
            edit(dec, keep_dec)
        rc = emu._L.dpemu_qsim_decay(emu._h, C.addressof(cfg), C.addressof(st), C.addressof(dec) if dec_ptr else None,
                                     outs['summary'].data_ptr(), outs['events'].data_ptr(), p_buf.data_ptr(),
                                     bufs[0].data_ptr(), states, counts, None)
        return rc, emu._L.dpemu_last_error(emu._h)

    def above(dec, keep):
        keep[1][2, 31] = ONE + 1

    def null_damp(dec, keep):
        dec.damp = None

    def null_deph(dec, keep):
        dec.deph = None

    for kw, word in ((dict(dec_ptr=None), b'dec is NULL'), (dict(edit=null_damp), b'damp is NULL'),
                     (dict(edit=null_deph), b'deph is NULL'), (dict(edit=above), b'deph: entry 31 of core 2'),
                     (dict(n_regs=0), b'n_regs'), (dict(drv_elem=cfg.meas_elem), b'meas_elem'),
                     (dict(counts=bufs[2].data_ptr() + 4), b'counts')):
        rc, msg = call(**kw)
        assert rc == -22 and word in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all((b == 7).all().item() for b in [p_buf] + bufs)                         # nothing was launched
    rc, msg = call(states=None, drv_elem=cfg.meas_elem)      # without states cfg->meas_elem is not read, as in dpemu_qsim
    assert rc == 0, msg
    assert emu.last_kernel() == 'qsim_kernel<decay>'
    torch.cuda.synchronize()
    assert (bufs[1] == 7).all().item() and not (bufs[2] == 7).all().item()
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        p0, r0, s0 = emu.simulate_gates(cfg, gs, {}, 0, measure=True, t_final=5)
        assert tuple(p0.shape) == (2, 0, 4) and tuple(s0.shape) == (0,) and emu.kernel_times() == []
        emu.simulate_gates(cfg, gs, outs, n, shot_begin=SHOT0, measure=True)
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 1 and 0 < ms[0] < 100                                           # one pair: round the kernel
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, gs, outs, n, decay_counts=bufs[2][:1])
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, tm.fuzz_gateset(), outs, n, t_final=5)                # no decay in the gate set
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, tm.fuzz_gateset(), outs, n, decay_counts=bufs[2])


# ---- 6. the Ramsey workload behind dpemu_run ----

def test_ramsey_fringe_loses_contrast(emu):
    """workloads.config2_ramsey on 2 cores, delays of 16 and 2,016 clocks between the two X90, 4,096 shots (2,048 per
    delay): per core and delay the mean P(1) is (1 + e^(-tau / T2)) / 2 within 5 standard errors, a row's P(1)
    lying in [0, 1] (sigma <= 1/2): the bound of tests/test_qsim_decay.py's T2 experiment.  Core 0 has T2 = 2 T1,
    core 1 a shorter one"""
    import torch
    n, t1, t2 = 4096, 5000, {0: 10000, 1: 3000}
    ps = ProgramSet(workloads.config2_ramsey(n_cores=2, n_points=2, tau_step=2000))
    cfg = _abi.make_config(2, n_groups=2, shots_per_group=1, max_cycles=1 << 20, event_cap=8, meas_cap=2, seed=0x7A35E7)
    emu.load(ps)
    outs = alloc_device_outputs(cfg, n, want=('summary', 'events'))
    emu.run_device(cfg, n, 0, outs)
    torch.cuda.synchronize()
    ev = u32(outs['events']).reshape(cfg.event_cap, 2, n, 4)
    gs = qsim.GateSet(drv_elem=workloads.QDRV)
    for c in (0, 1):
        w = ev[:, c, 0]                                  # the first drive strobe of the core's first lane is its X90
        k = next(k for k in range(cfg.event_cap) if w[k, 1] >> 28 == 0 and (w[k, 1] >> 24) & 3 == workloads.QDRV)
        gs.add_rotation(c, int(w[k, 2] >> 17), int(w[k, 1] & 0xFFFFFF), int(w[k, 3] & 0xFFFF), np.pi / 2)
        gs.set_decay(c, t1, t2[c])
    gs.registers([0, 1])
    pops, result = emu.simulate_gates(cfg, gs, outs, n)
    assert emu.last_kernel() == 'qsim_kernel<decay>'
    torch.cuda.synchronize()
    res = u32(result)
    assert (res[:, :, 1] == 2).all() and not res[:, :, 2:].any()
    p = pops.cpu().numpy().view(np.uint64).astype(np.float64)
    p1 = p[:, :, 2] / p.sum(axis=2)
    for c in (0, 1):
        for point, tau in ((0, 16), (1, 2016)):
            want, mean = 0.5 * (1 + np.exp(-tau / t2[c])), p1[c, point::2].mean()
            print('core', c, 'tau', tau, 'mean', mean, 'want', want, 'in standard errors', (mean - want) / (0.5 / np.sqrt(n // 2)))
            assert abs(mean - want) <= 5 * 0.5 / np.sqrt(n // 2)
    # and the rows are the reference's, on the first 64 shots' worth of each core
    summary = u32(outs['summary']).reshape(2, n, 8)[:, :64].reshape(-1, 8)
    want = dref.qsim_decay_gateset(cfg, gs, summary, np.ascontiguousarray(ev[:, :, :64]).reshape(cfg.event_cap, -1, 4), 64)
    np.testing.assert_array_equal(pops.cpu().numpy().view(np.uint64)[:, :64], want[0])
    np.testing.assert_array_equal(res[:, :64], want[1])


# ---- 7. co-simulation with decaying qubits ----

def test_cosimulate_with_a_decay(emu):
    """workloads.cosim_active_reset on 8 cores x 37 shots (296 rows) with a T1 and a T2 per core: the loop converges
    within (distinct readout strobe times of a shot) + 1 = 3 passes from zeros, all-ones and random words, to one
    fixed point, whose outputs are the reference's on the final events"""
    import torch
    from tests.test_gpu_cosim import OUTS, fresh_outputs, kept_events, reset_cfg
    n, C_, shot0, t_final = 37, 8, 1000, 6000
    prog, gs = workloads.cosim_active_reset(C_, prep=1)
    with_decay(gs, {c: (1500 + 200 * c, 900 + 300 * c) for c in range(C_)})
    cfg = reset_cfg(C_, SM)
    emu.load(ProgramSet(prog))
    rng = np.random.default_rng(6)
    starts = {'zeros': None, 'ones': np.full(n * C_, -1, np.int32),
              'random': rng.integers(-2 ** 31, 2 ** 31, n * C_).astype(np.int32)}
    seen = {}
    for name, s0 in starts.items():
        dev = fresh_outputs(cfg, n, OUTS)
        st0 = None if s0 is None else torch.from_numpy(s0.copy()).cuda()
        pops, result, st, passes = emu.cosimulate(cfg, gs, dev, n, shot0, states=st0, t_final=t_final)
        assert emu.last_kernel() == 'qsim_kernel<meas,decay>' and passes <= 3, (name, passes)
        torch.cuda.synchronize()
        seen[name] = dict(pops=pops.cpu().numpy().view(np.uint64), result=u32(result), states=u32(st),
                          summary=u32(dev['summary']), events=u32(dev['events']), meas=u32(dev['meas']))
    zero = seen['zeros']
    for name in ('ones', 'random'):
        for k in ('pops', 'result', 'states', 'summary', 'meas'):
            np.testing.assert_array_equal(seen[name][k], zero[k], err_msg='{} from {}'.format(k, name))
        np.testing.assert_array_equal(kept_events(seen[name], cfg), kept_events(zero, cfg), err_msg='events from ' + name)
    want = dref.qsim_decay_gateset(cfg, gs, zero['summary'].reshape(-1, 8), zero['events'].reshape(cfg.event_cap, -1, 4), n,
                                   shot0, measure_readouts=True, t_final=t_final)
    for g, w, k in zip((zero['pops'], zero['result'], zero['states']), want, ('pops', 'result', 'states')):
        np.testing.assert_array_equal(g.reshape(-1), np.asarray(w).reshape(-1), err_msg=k)
    assert want[3][:, :, 0].any() and want[3][:, :, 1].any()                          # the decay acted
    assert (zero['summary'].reshape(-1, 8)[:, 6] == zero['states']).all()             # the interpreter's bits are the qubit's
    # without the decay every second readout finds |0>; a qubit that relaxes or is re-excited need not
    b = qsim.state_bits(zero['states'], cfg, n)
    assert set((b & 1).reshape(-1).tolist()) == {0, 1}
