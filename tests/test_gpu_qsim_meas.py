"""GPU tests of the measuring qubit-state stage and of the states it hands to
the readout stages (dpemu_qsim_meas and the *_st calls, include/dpemu.h):
qsim_kernel<true> against tests/qsim_meas_ref.py on every word of pops, result
and states over hand-built records; the *_st calls against their base calls
and against the injected numpy references; and the chain run -> dds ->
simulate_gates(measure=True) -> feedline ADC -> demodulator -> iq_stats, where
the discriminated bits are the qubit's."""

import ctypes as C
import functools
import math

import numpy as np
import pytest

from distributed_processor_amd import _abi, isa, qsim, workloads
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable, FeedlineTable, ResonatorTable
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from distributed_processor_amd.readout import ReadoutStats
from tests import qsim_meas_ref as mref, qsim_ref
from tests.handbuilt import random_words
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, freq_buffer
from tests.test_gpu_demod_iq import assembled
from tests.test_resonator import KAPPA

pytestmark = pytest.mark.gpu

ORDERS = [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR]
ORDER_IDS = ['core_major', 'shot_major']
ONE = 1 << 30
QDRV = workloads.QDRV


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def to_dev(a):
    import torch
    a = np.array(a, order='C')                          # a writable copy: cached arrays are read-only
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(pops, result, states):
    import torch
    torch.cuda.synchronize()
    return pops.cpu().numpy().view(np.uint64), result.cpu().numpy().view(np.uint32), states.cpu().numpy().view(np.uint32)


def assert_same(got, want):
    for g, w, name in zip(got, want, ('pops', 'result', 'states')):
        assert g.shape == w.shape and g.dtype == w.dtype, name
        np.testing.assert_array_equal(g, w, err_msg=name)


# ---- 1. bit-exact on hand-built records ----

C_FUZZ, CAP_FUZZ = 4, 56
REGS_FUZZ = [(0, 1), 2]                                 # core 3 is in no register
ENV = 0x040000
PHASES = (0, 1, 255, 256, 0x7FFF, 0x8000, 0x1FFFF)
TINY, GROW, ZERO = 5, 6, 7                              # freq indices of the non-unitary entries


def fuzz_gateset():
    """per core three rotations and a ZX on the control, error thresholds 0, 2^30, all, 2^28 by turns; on cores
    1 and 2 an entry scaled by 2^-6 (T ~ 2^48 after one: the shift is 5 or more; after five of them the state is
    all zero) and the zero matrix (a readout of the zero state: T = 0 reads 1 and shifts by 0), on core 0 one
    with rows of norm 2 (the clamp, wrapping sums)"""
    gs = qsim.GateSet(drv_elem=QDRV)
    rng = np.random.default_rng(78)
    thr = (0, 1 << 30, 0xFFFFFFFF, 1 << 28)
    for core in (0, 1, 2):
        for k in range(4):
            if k == 1 and core == 0:
                gs.add_zx(0, 1, k, ENV, 100, 1.3)
                gs.entries[-1]['err_thr'] = thr[1]
            else:
                gs.add_matrix(core, k, ENV, 100 + core, qsim.rotation(rng.uniform(0, 6.0), rng.uniform(0, 1.0)),
                              err_thr=thr[(k + core) % 4])
    for core in (1, 2):
        gs.add_matrix(core, TINY, ENV, 100 + core, qsim.rotation(np.pi / 2, 0.1 * core) / 64)
        gs.add_matrix(core, ZERO, ENV, 100 + core, np.zeros(8, np.int64))
    s = ONE
    gs.add_matrix(0, GROW, ENV, 100, np.array([s, -s, s, s, -s, s, s, -s]))
    gs.detune[0], gs.detune[1], gs.detune[2] = 0x00012345, 0xFFF00001, 0x80000001
    return gs.registers(REGS_FUZZ)


def fuzz_entries(core):
    """the rotations and the ZX of a core in fuzz_gateset"""
    return 4


@functools.lru_cache(maxsize=None)
def fuzz_records(n_shots, lane_order, seed, n_cores=C_FUZZ, cap=CAP_FUZZ, entries=fuzz_entries):
    """summary / events of n_shots x n_cores lanes, cap slots: per lane 0 .. cap + 5 records (empty lanes,
    lanes over event_cap) in nondecreasing time with steps of 0..3 clocks (ties between the lanes of a register
    are common).  A lane is readout-heavy with probability 0.2 (at cap 56 its first 40 of 45 or more records hold 40
    readout strobes), else a fifth of its records are readouts; the rest are drive strobes with a dictionary key
    (one of the core's first ``entries(core)``), an unmatched key or a non-unitary entry, strobes of element 1 or
    3, pulse_resets and records of kind >= 2; every slot past the count holds garbage"""
    rng = np.random.default_rng(seed)
    n_lanes = n_shots * n_cores
    summary = random_words(rng, (n_lanes, 8))
    ev = random_words(rng, (cap, n_lanes, 4))
    for sl in range(n_shots):
        for core in range(n_cores):
            lane = sl * n_cores + core if lane_order == _abi.LANES_SHOT_MAJOR else core * n_shots + sl
            heavy = rng.random() < 0.2
            n = int(rng.integers(cap - 11, cap + 6)) if heavy else int(
                rng.choice([0, cap + 5, rng.integers(1, cap + 1)], p=[0.1, 0.15, 0.75]))
            summary[lane, 2] = n
            t = 5
            for k in range(min(n, cap)):
                t += int(rng.integers(0, 4))
                what = rng.random()
                phase = int(PHASES[rng.integers(0, len(PHASES))] if rng.random() < 0.7 else rng.integers(0, 1 << 17))
                freq, elem, kind = int(rng.integers(0, entries(core))), QDRV, 0
                p_ro = 0.9 if heavy else 0.2
                if what < p_ro:
                    elem = RDLO
                elif what < p_ro + 0.03:
                    freq = 11                            # no such key
                elif what < p_ro + 0.07 and core in (1, 2):
                    freq = TINY
                elif what < p_ro + 0.09 and core in (1, 2):
                    freq = ZERO
                elif what < p_ro + 0.09 and core == 0:
                    freq = GROW
                elif what < p_ro + 0.14:
                    elem = int(rng.choice([1, 3]))
                elif what < p_ro + 0.18:
                    kind = int(rng.choice([1, 1, 2, 9, 15]))
                cfgw = (int(rng.integers(0, 4)) << 2) | elem
                ev[k, lane] = (t & 0xFFFFFFFF, ENV | (cfgw << 24) | (kind << 28), phase | (freq << 17),
                               (100 + core) | (int(rng.integers(0, 1 << 16)) << 16))
    summary.setflags(write=False)
    ev.setflags(write=False)
    return summary, ev


def fuzz_cfg(lane_order, n_cores=C_FUZZ, cap=CAP_FUZZ):
    return _abi.make_config(n_cores, event_cap=cap, lane_order=lane_order, seed=0x51C0FFEE12345678, meas_elem=RDLO)


@functools.lru_cache(maxsize=None)
def fuzz_reference(n_shots, lane_order, seed, shot0):
    summary, ev = fuzz_records(n_shots, lane_order, seed)
    shifts, amps = [], []
    out = mref.qsim_meas_gateset(fuzz_cfg(lane_order), fuzz_gateset(), summary, ev, n_shots, shot0, shifts=shifts,
                                 amps=amps)
    return out, shifts, amps


def check_fuzz_reach(n_shots, lane_order, seed, shot0):
    """what the records were built to reach, asserted on the reference"""
    summary, ev = fuzz_records(n_shots, lane_order, seed)
    (pops, res, states), shifts, amps = fuzz_reference(n_shots, lane_order, seed, shot0)
    cfg = fuzz_cfg(lane_order)
    assert (res[:, :, 3] >> 31).any() and not (res[:, :, 3] >> 31).all()              # a lane over event_cap
    assert (res[:, :, 2] > 0).any() and ((res[:, :, 3] & 0xFFFF) > 0).any()           # unmatched pulses; errors
    assert max(m for _, _, m, _, _ in shifts) >= 39                                   # 40 readouts in a lane ...
    assert (states == 0xFFFFFFFF).any() or np.unique(states).size > 100               # ... whose bits fill the word
    assert max(s for _, _, _, _, s in shifts) >= 5 and any(s == 0 for _, _, _, _, s in shifts)
    assert {b for _, _, _, b, _ in shifts} == {0, 1}
    lanes3 = [qsim_ref.lane_of(cfg, sl, 3, n_shots) for sl in range(n_shots)]
    assert not states[lanes3].any()                                                   # the core in no register
    assert any(any(mref.kept_strobes(summary, ev, L, CAP_FUZZ, QDRV, RDLO)) for L in lanes3)
    assert max(abs(v) for x in amps for c in x for v in c) == (1 << 31) - 1           # the clamp acted
    gone = [i for i, x in enumerate(amps) if all(c == (0, 0) for c in x)]             # the zero state, row i ...
    assert any(b == 1 and s == 0 and row in gone for row, _, m, b, s in shifts if m > 20)   # ... and read late
    ties = 0
    for sl in range(n_shots):
        a, b = ({(r[0], r[5]) for r in mref.kept_strobes(summary, ev, qsim_ref.lane_of(cfg, sl, c, n_shots), CAP_FUZZ,
                                                           QDRV, RDLO)} for c in (0, 1))
        ties += any((t, not ro_) in b for t, ro_ in a)                                # a readout at the other lane's drive t
    assert ties > 10


@pytest.mark.parametrize('n_shots', [70, 300])
@pytest.mark.parametrize('lane_order', ORDERS, ids=ORDER_IDS)
def test_fuzz_bit_exact(emu, lane_order, n_shots):
    """70 shots x 2 registers = 140 rows: a partly filled last wave, a workgroup whose rows span both registers;
    300 shots: three workgroups, the middle one spanning both; shots across 2^32"""
    seed, shot0 = 100 + n_shots, 2 ** 32 - 30
    check_fuzz_reach(n_shots, lane_order, seed, shot0)
    summary, ev = fuzz_records(n_shots, lane_order, seed)
    want = fuzz_reference(n_shots, lane_order, seed, shot0)[0]
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    got = host(*emu.simulate_gates(fuzz_cfg(lane_order), fuzz_gateset(), outs, n_shots, shot_begin=shot0, measure=True))
    assert emu.last_kernel() == 'qsim_kernel<meas>'
    assert_same(got, want)


# ---- 64 registers (tests/test_gpu_qsim.py's wide cases, measuring) ----

CAP_WIDE = 24


def wide_meas_records(n_shots, lane_order, seed):
    from tests.test_gpu_qsim import C_WIDE, wide_entries
    return fuzz_records(n_shots, lane_order, seed, C_WIDE, CAP_WIDE, wide_entries)


def wide_meas_gateset(which):
    from tests.test_gpu_qsim import wide_gateset
    return wide_gateset(which, drv_elem=QDRV)


@functools.lru_cache(maxsize=None)
def wide_meas_reference(which, n_shots, lane_order, seed, shot0=2 ** 32 - 30):
    from tests.test_gpu_qsim import C_WIDE
    summary, ev = wide_meas_records(n_shots, lane_order, seed)
    return mref.qsim_meas_gateset(fuzz_cfg(lane_order, C_WIDE, CAP_WIDE), wide_meas_gateset(which), summary, ev, n_shots,
                                  shot0)


@pytest.mark.parametrize('n_shots', [1, 5, 37])
@pytest.mark.parametrize('lane_order', ORDERS, ids=ORDER_IDS)
@pytest.mark.parametrize('which', ['1q', '2q'])
def test_64_registers_measuring(emu, which, lane_order, n_shots):
    """qsim_kernel<true> on 64 one-qubit and 32 two-qubit registers of 64 cores: up to 64 dictionary slots staged
    per workgroup (reach: tests/test_qsim_meas.py test_wide_cases_reach_every_slot_window)"""
    from tests.test_gpu_qsim import C_WIDE, wide_seed
    seed, shot0 = wide_seed(which, n_shots) + 1000, 2 ** 32 - 30
    summary, ev = wide_meas_records(n_shots, lane_order, seed)
    want = wide_meas_reference(which, n_shots, lane_order, seed)
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    got = host(*emu.simulate_gates(fuzz_cfg(lane_order, C_WIDE, CAP_WIDE), wide_meas_gateset(which), outs, n_shots,
                                   shot_begin=shot0, measure=True))
    assert emu.last_kernel() == 'qsim_kernel<meas>'
    assert_same(got, want)


def test_caller_buffers_and_refusals(emu):
    """caller-made outputs full of garbage are assigned (states too: the lanes of core 3 read 0); the three
    conditions dpemu_qsim_meas adds are refused with -22 before anything is launched, as dpemu_qsim's are"""
    import torch
    n_shots, order, seed, shot0 = 70, _abi.LANES_CORE_MAJOR, 170, 2 ** 32 - 30
    cfg, gs = fuzz_cfg(order), fuzz_gateset()
    summary, ev = fuzz_records(n_shots, order, seed)
    want = fuzz_reference(n_shots, order, seed, shot0)[0]
    outs = dict(summary=to_dev(summary), events=to_dev(ev))
    p_buf = torch.full((2, n_shots, 4), 0x5A5A5A5A5A5A, dtype=torch.int64, device='cuda')
    r_buf = torch.full((2, n_shots, 4), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    s_buf = torch.full((n_shots * C_FUZZ,), 0x5A5A5A5A, dtype=torch.int32, device='cuda')
    p2, r2, s2 = emu.simulate_gates(cfg, gs, outs, n_shots, shot_begin=shot0, pops=p_buf, result=r_buf, measure=True,
                                    states=s_buf)
    assert p2 is p_buf and r2 is r_buf and s2 is s_buf
    assert_same(host(p2, r2, s2), want)

    def call(cfg_=cfg, states=s_buf.data_ptr(), **f):
        st, keep = gs.struct(cfg, n_shots, shot0)
        for k, v in f.items():
            setattr(st, k, v)
        rc = emu._L.dpemu_qsim_meas(emu._h, C.addressof(cfg_), C.addressof(st), outs['summary'].data_ptr(),
                                    outs['events'].data_ptr(), p_buf.data_ptr(), r_buf.data_ptr(), states, None)
        return rc, emu._L.dpemu_last_error(emu._h)

    torch.cuda.synchronize()
    for b in (p_buf, r_buf, s_buf):
        b.fill_(7)
    bad4, same = fuzz_cfg(order), fuzz_cfg(order)
    bad4.meas_elem, same.meas_elem = 4, QDRV
    for kw, field in ((dict(states=None), b'states'), (dict(cfg_=bad4), b'meas_elem'), (dict(cfg_=same), b'meas_elem'),
                      (dict(drv_elem=4), b'drv_elem'), (dict(n_regs=0), b'n_regs'), (dict(n_lanes=5), b'n_lanes')):
        rc, msg = call(**kw)
        assert rc == -22 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert all((b == 7).all().item() for b in (p_buf, r_buf, s_buf))                  # nothing was launched
    # no shots: accepted, nothing launched, the tables still checked
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        p0, r0, s0 = emu.simulate_gates(cfg, gs, {}, 0, measure=True)
        assert tuple(p0.shape) == (2, 0, 4) and tuple(s0.shape) == (0,) and emu.kernel_times() == []
        emu.simulate_gates(cfg, gs, outs, n_shots, shot_begin=shot0, measure=True)
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 1 and 0 < ms[0] < 100                                           # one pair: round the kernel
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, gs, outs, n_shots, measure=True, states=s_buf[:5])
    with pytest.raises(DpemuError):
        emu.simulate_gates(cfg, gs, outs, n_shots, states=s_buf)                      # states without measure


# ---- 2. behind dpemu_run on config 4 ----

def rb_run(emu, n_seq, depth, spg, lane_order=_abi.LANES_CORE_MAJOR, shot0=0, n_shots=None, demod=None, seed=0xA5EED):
    groups = workloads.config4_rb2q(n_seq=n_seq, depth=depth)
    ps = ProgramSet(groups, cores_per_shot=2)
    cfg = _abi.make_config(2, n_groups=n_seq, shots_per_group=spg, max_cycles=1 << 22, event_cap=8 * depth + 16,
                           meas_cap=2, lane_order=lane_order, seed=seed, meas_elem=RDLO, demod=demod)
    n = n_seq * spg if n_shots is None else n_shots
    emu.load(ps)
    outs = alloc_device_outputs(cfg, n, want=('summary', 'events'))
    emu.run_device(cfg, n, shot0, outs)
    return ps, cfg, outs, n


def test_unused_meas_elem_equals_qsim(emu):
    """workloads.config4_rb2q(n_seq=8, depth=10): with meas_elem an element no strobe uses, pops and result are
    dpemu_qsim's bit for bit and states is zero; with the rdlo element every lane has its one readout"""
    import torch
    ps, cfg, outs, n = rb_run(emu, 8, 10, 2)
    gs = workloads.rb2q_gateset(2, over_rotation=0.03, err_1q=2.0 ** -5, err_2q=2.0 ** -4)
    base = emu.simulate_gates(cfg, gs, outs, n)
    assert emu.last_kernel() == 'qsim_kernel'
    cfg3 = _abi.make_config(2, n_groups=8, shots_per_group=2, max_cycles=1 << 22, event_cap=cfg.event_cap, meas_cap=2,
                            seed=0xA5EED, meas_elem=3)
    ev = outs['events'].cpu().numpy().view(np.uint32)
    written = np.arange(ev.shape[0])[:, None] < outs['summary'].cpu().numpy().view(np.uint32)[:, 2][None, :]
    assert not (written & (ev[:, :, 1] >> 28 == 0) & ((ev[:, :, 1] >> 24) & 3 == 3)).any()
    p, r, s = emu.simulate_gates(cfg3, gs, outs, n, measure=True)
    assert emu.last_kernel() == 'qsim_kernel<meas>'
    assert torch.equal(p, base[0]) and torch.equal(r, base[1]) and not s.any().item()
    assert (base[1][:, :, 1] > 20).all().item() and (base[1][:, :, 3] != 0).any().item()
    got = host(*emu.simulate_gates(cfg, gs, outs, n, measure=True))
    want = mref.qsim_meas_gateset(cfg, gs, outs['summary'].cpu().numpy(), outs['events'].cpu().numpy(), n)
    assert_same(got, want)
    assert (got[2] <= 1).all() and set(got[2].tolist()) == {0, 1}
    assert torch.equal(r[:, :, 1:], torch.from_numpy(got[1].view(np.int32)).cuda()[:, :, 1:])    # the counts do not change


@pytest.mark.parametrize('lane_order', ORDERS, ids=ORDER_IDS)
def test_two_half_batches(emu, lane_order):
    """counter-based draws: shots [5, 13) and [13, 21) in two runs equal [5, 21) in one, on all three outputs"""
    gs = workloads.rb2q_gateset(2, over_rotation=0.2, err_1q=2.0 ** -5, err_2q=2.0 ** -4)
    ps, cfg, outs, n = rb_run(emu, 8, 10, 2, lane_order, shot0=5)
    whole = host(*emu.simulate_gates(cfg, gs, outs, n, shot_begin=5, measure=True))
    assert set(whole[2].tolist()) == {0, 1}
    bits = qsim.state_bits(whole[2], cfg, n)
    for b in (0, 8):
        _, _, o2, _ = rb_run(emu, 8, 10, 2, lane_order, shot0=5 + b, n_shots=8)
        p, r, s = host(*emu.simulate_gates(cfg, gs, o2, 8, shot_begin=5 + b, measure=True))
        np.testing.assert_array_equal(p, whole[0][:, b:b + 8])
        np.testing.assert_array_equal(r, whole[1][:, b:b + 8])
        np.testing.assert_array_equal(qsim.state_bits(s, cfg, 8), bits[:, b:b + 8])


# ---- 3. states into the readout stages ----

ST_SHOTS, ST_CLKS, ST_CAP = 16, 2048, 2
ST_F = [0x0C000000 + k * (2 ** 32 // 32) for k in (0, 3, 7, 12)]
ST_KEY = lambda c: (0, ENV, 7000 + 100 * c)                                           # noqa: E731


def st_programs(x90s, reads_at=(80, 900), window=40):
    """one group of 4 cores: core c plays x90s[c] X90 drive pulses, then two readouts (rdrv, rdlo 20 clocks later)"""
    env = np.full(4 * (window + 10), SQUARE, np.uint32)
    prog = {}
    for c in range(4):
        reads = [dict(A=15000 + 1000 * c, ph_d=1000 * c, ph_lo=77 * c, L_d=window + 5, L_lo=window, lo_at=20,
                      gap=reads_at[1] - reads_at[0]) for _ in range(2)]
        words = ro_program(reads, t0=reads_at[0])
        pulses = [isa.pulse_cmd(freq_word=0, phase_word=0, amp_word=ST_KEY(c)[2], env_word=ENV, cfg_word=QDRV,
                                cmd_time=10 + 16 * k) for k in range(x90s[c])]
        words[1:1] = pulses
        prog[c] = assembled(words, env, env, freq_buffer(ST_F[c], 1), freq_buffer(ST_F[c], 1))
    return ProgramSet([prog], cores_per_shot=4)


def st_gateset():
    gs = qsim.GateSet(drv_elem=QDRV)
    for c in range(4):
        gs.add_rotation(c, *ST_KEY(c), np.pi / 2)
    return gs.registers([(0, 1), 2, 3])


def st_cfg(lane_order, p1=0.5, sigma=20.0, seed=0xFEED5EED):
    return _abi.make_config(4, max_cycles=1 << 20, event_cap=16, meas_cap=ST_CAP, meas_latency=32, seed=seed, p1=p1,
                            lane_order=lane_order, meas_elem=RDLO,
                            demod=dict(drv_elem=RDRV, cpw=4, delay=20, theta=(0.3, 2.2), gain=(0.9, 0.6), sigma=sigma,
                                       axis=[0.1, 0.9, 1.7, 2.5], thr=-50))


def st_pipeline(emu, cfg, ps, n_shots, shot0, who):
    import torch
    emu.load(ps)
    out = alloc_device_outputs(cfg, n_shots, want=('summary', 'events'))
    emu.run_device(cfg, n_shots, shot0, out)
    params = {RDRV: (1, 1), RDLO: (1, 1)}
    drv = ChannelPlan(ps, cfg, shot0, n_shots, [(s_, c, RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, shot0, n_shots, [(s_, c, RDLO) for s_, c in who], params)
    iq_d, iq_l = emu.synthesize(drv, out, ST_CLKS), emu.synthesize(lo, out, ST_CLKS)
    pt = DemodPairTable(cfg, drv, lo)
    states = emu.simulate_gates(cfg, st_gateset(), out, n_shots, shot_begin=shot0, measure=True)[2]
    torch.cuda.synchronize()
    h = dict(summary=out['summary'].cpu().numpy(), events=out['events'].cpu().numpy(), iq_d=iq_d.cpu().numpy(),
             iq_l=iq_l.cpu().numpy(), states=states.cpu().numpy().view(np.uint32))
    return out, iq_d, iq_l, pt, states, h


def packed_draws(cfg, n_shots, shot0):
    """the per-lane words of the base calls' own draws"""
    lanes = np.arange(n_shots * 4)
    if cfg.lane_order == _abi.LANES_SHOT_MAJOR:
        core, sl = lanes % 4, lanes // 4
    else:
        core, sl = lanes // n_shots, lanes % n_shots
    return mref.draw_words(cfg, sl + shot0, core, n_bits=ST_CAP)


@pytest.mark.parametrize('lane_order', ORDERS, ids=ORDER_IDS)
def test_states_into_the_readout_stages(emu, lane_order):
    """2 lines x 3 members out of 16 shots x 4 cores, 2,048 LO samples, meas_cap 2, two readouts per lane, one
    X90 per core (the measured states are random; the second readout repeats the first).  Per *_st call:
    states = NULL and states = the packed draws are the base call bit for bit; the states of dpemu_qsim_meas give
    the injected numpy reference bit for bit"""
    import torch
    shot0 = 2 ** 32 - 9
    cfg, ps = st_cfg(lane_order), st_programs([1, 1, 1, 1])
    who = [(shot0 + s_, c) for s_ in (3, 12) for c in (2, 0, 1)]
    lines = [[0, 1, 2], [3, 4, 5]]
    out, iq_d, iq_l, pt, states, h = st_pipeline(emu, cfg, ps, ST_SHOTS, shot0, who)
    ft = FeedlineTable(pt, lines)
    bits = qsim.state_bits(h['states'], cfg, ST_SHOTS)
    assert set(bits.reshape(-1).tolist()) == {0, 3}                                   # two readouts, the second repeats
    draws = packed_draws(cfg, ST_SHOTS, shot0)
    lane = pt.cols['lane'].astype(np.int64)
    assert not np.array_equal(draws[lane], h['states'][lane]) and len(set(draws[lane].tolist())) > 1
    d_draws = to_dev(draws)
    null = C.c_void_p(None)
    pst, lst = pt.struct(ST_CAP, ST_CLKS, ST_CLKS), ft.struct()
    o = (out['summary'].data_ptr(), out['events'].data_ptr())

    def u32(t):
        torch.cuda.synchronize()
        return t.cpu().numpy().view(np.uint32)

    def raw(name, *args):
        rc = getattr(emu._L, name)(emu._h, C.addressof(cfg), C.addressof(pst), C.addressof(lst), *args, None)
        assert rc == 0, (name, emu._L.dpemu_last_error(emu._h))

    # the plain ADC stage
    base = emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS)
    buf = torch.zeros_like(base)
    raw('dpemu_feedline_adc_st', *o, iq_d.data_ptr(), buf.data_ptr(), null)
    assert torch.equal(buf, base) and emu.last_kernel() == 'feedline_adc_kernel'
    assert torch.equal(emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, states=d_draws), base)
    adc = emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, states=states)
    want = mref.feedline_adc_st(h['states'], cfg, pt.cols, lines, h['summary'], h['events'], h['iq_d'], ST_CLKS, ST_CAP)
    np.testing.assert_array_equal(u32(adc), want)
    assert not torch.equal(adc, base)
    # the resonator stage
    rng = np.random.default_rng(5)
    ang = rng.uniform(0, 2 * np.pi, (pt.n_pairs, 2, 2))
    coef = np.rint(np.stack([0.9 * np.cos(ang[..., 0]), 0.9 * np.sin(ang[..., 0]), 0.1 * np.cos(ang[..., 1]),
                             0.1 * np.sin(ang[..., 1])], axis=-1) * ONE).astype(np.int64)
    tab = ResonatorTable.from_coefficients(pt, coef, 300)
    base_r = emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, resonators=tab)
    rs = tab.struct()
    buf = torch.zeros_like(base_r)
    raw('dpemu_feedline_adc_res_st', C.addressof(rs), *o, iq_d.data_ptr(), buf.data_ptr(), null)
    assert torch.equal(buf, base_r) and emu.last_kernel() == 'feedline_res_kernel'
    assert torch.equal(emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, resonators=tab, states=d_draws), base_r)
    adc_r = emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, resonators=tab, states=states)
    want = mref.feedline_adc_res_st(h['states'], cfg, pt.cols, lines, tab.coef, tab.adc_sigma, h['summary'], h['events'],
                                    h['iq_d'], ST_CLKS, ST_CAP)
    np.testing.assert_array_equal(u32(adc_r), want)
    assert not torch.equal(adc_r, base_r)
    # demodulate_feedline passes states on to the ADC stage it makes
    acc, res = emu.demodulate_feedline(cfg, ft, iq_l, out, iq_drv=iq_d, states=states)
    acc2, res2 = emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc)
    assert torch.equal(acc, acc2) and torch.equal(res, res2)
    with pytest.raises(DpemuError):
        emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc, states=states)
    # the traces
    base_t = emu.feedline_traces(cfg, ft, iq_l, out, adc, 16, 4, by_slot=True)
    tb = _abi.TraceBins(16, 4, 1)
    buf = torch.full_like(base_t, 5)
    raw('dpemu_feedline_traces_st', C.addressof(tb), *o, adc.data_ptr(), iq_l.data_ptr(), buf.data_ptr(), null)
    assert torch.equal(buf, base_t) and emu.last_kernel() == 'feedline_trace_kernel'
    assert torch.equal(emu.feedline_traces(cfg, ft, iq_l, out, adc, 16, 4, by_slot=True, states=d_draws), base_t)
    tr = emu.feedline_traces(cfg, ft, iq_l, out, adc, 16, 4, by_slot=True, states=states)
    want = mref.feedline_traces_st(h['states'], cfg, pt.cols, lines, h['summary'], h['events'], u32(adc), h['iq_l'], ST_CAP,
                                   16, 4, True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(tr.cpu().numpy(), want)
    assert not torch.equal(tr, base_t)
    # iq_stats with pairs=: the run layout's words are gathered to the pairs' lanes
    h_acc, h_res = acc.cpu().numpy(), u32(res)
    base_s, base_b = emu.iq_stats(cfg, acc, res, pairs=pt, by_slot=True, bits=True)
    ist = _abi.IQColumns(pt.n_pairs, ST_CAP, 1, 2)
    core_a, shot_a = np.ascontiguousarray(pt.cols['core'], np.uint32), np.ascontiguousarray(pt.cols['shot'], np.uint64)
    ist.core, ist.shot = core_a.ctypes.data, shot_a.ctypes.data
    buf, bbuf = torch.full_like(base_s, 5), torch.zeros_like(base_b)
    rc = emu._L.dpemu_iq_stats_st(emu._h, C.addressof(cfg), C.addressof(ist), acc.data_ptr(), res.data_ptr(),
                                  buf.data_ptr(), bbuf.data_ptr(), null, None)
    assert rc == 0 and torch.equal(buf, base_s) and torch.equal(bbuf, base_b) and emu.last_kernel() == 'iq_stats_kernel'
    s2, b2 = emu.iq_stats(cfg, acc, res, pairs=pt, by_slot=True, bits=True, states=d_draws)
    assert torch.equal(s2, base_s) and torch.equal(b2, base_b)
    s3, b3 = emu.iq_stats(cfg, acc, res, pairs=pt, by_slot=True, bits=True, states=states)
    want_s, want_b = mref.iq_stats_st(h['states'][lane], cfg, h_acc, h_res[:, 0], core=pt.cols['core'],
                                      shot=pt.cols['shot'], by_slot=True)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s3.cpu().numpy(), want_s)
    np.testing.assert_array_equal(u32(b3), want_b)
    assert not torch.equal(s3, base_s) and want_s[..., 0].sum() == 2 * pt.n_pairs
    # iq_stats in the run layout: a column is a lane, dpemu_qsim_meas's buffer as it is (any acc serves)
    n_lanes = ST_SHOTS * 4
    acc_l = to_dev(rng.integers(-2 ** 31, 2 ** 31, (ST_CAP, n_lanes, 2)).astype(np.int32))
    h_cnt = h['summary'].view(np.uint32).reshape(-1, 8)[:, 5]
    assert (h_cnt == 2).all()
    base_s, base_b = emu.iq_stats(cfg, acc_l, out['summary'], shot_begin=shot0, bits=True)
    s2, b2 = emu.iq_stats(cfg, acc_l, out['summary'], shot_begin=shot0, bits=True, states=d_draws)
    assert torch.equal(s2, base_s) and torch.equal(b2, base_b)
    ist = _abi.IQColumns(n_lanes, ST_CAP, 0, 8)
    ist.shot_begin = shot0
    buf = torch.full_like(base_s, 5)
    rc = emu._L.dpemu_iq_stats_st(emu._h, C.addressof(cfg), C.addressof(ist), acc_l.data_ptr(),
                                  out['summary'].data_ptr() + 20, buf.data_ptr(), None, null, None)
    assert rc == 0 and torch.equal(buf, base_s)
    s3, b3 = emu.iq_stats(cfg, acc_l, out['summary'], shot_begin=shot0, bits=True, states=states)
    want_s, want_b = mref.iq_stats_st(h['states'], cfg, acc_l.cpu().numpy(), h_cnt, shot_begin=shot0)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(s3.cpu().numpy(), want_s)
    np.testing.assert_array_equal(u32(b3), want_b)
    assert not torch.equal(s3, base_s)
    for bad in (states[:5], states.to(torch.int64), states.cpu()):
        with pytest.raises(DpemuError):
            emu.iq_stats(cfg, acc_l, out['summary'], shot_begin=shot0, states=bad)
        with pytest.raises(DpemuError):
            emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, states=bad)


# ---- 4. the whole chain ----

def calibrated_axes(emu, cfg, ft, iq_d, iq_l, out, n_lanes, tab=None):
    """a prepare-0 / prepare-1 calibration through the injection: per core the axis word along the mean of
    acc(all ones) - acc(all zeros) at readout 0 and the threshold at the midpoint's projection"""
    import torch
    pt = ft.pairs
    acc = []
    for word in (0, -1):
        st = torch.full((n_lanes,), word, dtype=torch.int32, device='cuda')
        acc.append(emu.demodulate_feedline(cfg, ft, iq_l, out, iq_drv=iq_d, resonators=tab, states=st)[0][0]
                   .cpu().numpy().astype(np.float64))
    core = pt.cols['core'].astype(np.int64)
    axis, thr = [], []
    for c in range(cfg.cores_per_shot):
        a0, a1 = acc[0][core == c].mean(axis=0), acc[1][core == c].mean(axis=0)
        ang = math.atan2(a1[1] - a0[1], a1[0] - a0[0])
        w = _abi.axis_word(ang)
        ai, aq = ((w & 0xFFFF) ^ 0x8000) - 0x8000, ((w >> 16) ^ 0x8000) - 0x8000
        mid = (a0 + a1) / 2
        axis.append(w)
        thr.append(int((mid[0] * ai + mid[1] * aq) / 32768))
        sep = ((a1 - a0)[0] * ai + (a1 - a0)[1] * aq) / 32768
        assert sep > 2000, (c, sep)                                                   # the classes are far apart
    return axis, thr


def test_chain_reads_what_the_gates_prepared(emu):
    """4 cores x 64 shots, an X180 on the odd cores only, one line of four orthogonal tones per shot through the
    dispersive resonators, no noise: the discriminated bits are 1 on the odd cores and 0 on the even ones in
    every shot and the fidelity against the simulated states is 1.0; the same chain through the base calls with
    p1 = 0.5 classes the readouts by draws that no gate prepared, and its bits differ"""
    import torch
    n, shot0 = 64, 500
    cfg = st_cfg(_abi.LANES_SHOT_MAJOR, sigma=0.0)
    cfg.ro_theta[0], cfg.ro_theta[1] = 0, 1 << 31
    ps = st_programs([0, 2, 0, 2], reads_at=(80, 1100), window=160)                   # 640-clock windows: whole turns
    who = [(shot0 + s_, c) for s_ in range(n) for c in range(4)]
    out, iq_d, iq_l, pt, states, h = st_pipeline(emu, cfg, ps, n, shot0, who)
    assert emu.last_kernel() == 'qsim_kernel<meas>'
    bits_q = qsim.state_bits(h['states'], cfg, n)
    assert (bits_q[1::2] == 3).all() and not bits_q[0::2].any()
    ft = FeedlineTable(pt, [[4 * s_ + c for c in range(4)] for s_ in range(n)])
    chi = KAPPA // 2
    tab = ResonatorTable(pt, [[(ST_F[c] - chi) & 0xFFFFFFFF, (ST_F[c] + chi) & 0xFFFFFFFF] for c in pt.cols['core']], KAPPA)
    axis, thr = calibrated_axes(emu, cfg, ft, iq_d, iq_l, out, n * 4, tab)
    adc = emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, resonators=tab, states=states)
    acc, res = emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc)
    stats, bits = emu.iq_stats(cfg, acc, res, pairs=pt, axis=axis, thr=thr, bits=True, states=states)
    torch.cuda.synchronize()
    got = bits.cpu().numpy().view(np.uint32).reshape(n, 4).T                          # pairs are (shot, core) in order
    assert (got[1::2] == 3).all() and not got[0::2].any()
    rs = ReadoutStats(stats.cpu().numpy(), cfg, axis=axis, thr=thr)
    assert rs.fidelity() == 1.0 and rs.n.sum() == 2 * 4 * n
    assert not rs.n[0, 0::2, 1].any() and not rs.n[0, 1::2, 0].any()                  # the classes are the true states
    assert qsim.readout_survival(got, st_gateset().reg_core, n).tolist() == [0.0]
    # through the base calls: the draws, not the gates
    adc_b = emu.feedline_adc(cfg, ft, iq_d, out, ST_CLKS, resonators=tab)
    acc_b, res_b = emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc_b)
    stats_b, bits_b = emu.iq_stats(cfg, acc_b, res_b, pairs=pt, axis=axis, thr=thr, bits=True)
    torch.cuda.synchronize()
    assert not torch.equal(bits_b, bits)
    base = bits_b.cpu().numpy().view(np.uint32).reshape(n, 4).T
    assert 0 < ((base[1::2] & 1) == 0).sum() and 0 < ((base[0::2] & 1) == 1).sum()


def test_rb_survival_through_the_readout(emu):
    """workloads.config4_rb2q(n_seq=16, depth=20), 10 shots each; both cores of a shot on one feedline (their
    tones are whole turns apart over the rdlo window), theta = (0, pi), no noise, the axes calibrated through the
    injection.  Ideal gates: every state bit is 0 and readout_survival is 1.0; with over_rotation = 0.02 the
    survival read from the discriminated bits equals the one computed from the states, exactly"""
    import torch
    n_seq, depth, spg = 16, 20, 10
    demod = dict(drv_elem=RDRV, cpw=4, delay=workloads.RDLO_DELAY, theta=(0.0, math.pi), gain=(1.0, 1.0), sigma=0.0,
                 axis=0.0, thr=0)
    ps, cfg, out, n = rb_run(emu, n_seq, depth, spg, demod=demod)
    t_end = int(out['summary'][:, 0].max().item())
    n_clks = (t_end + 63) // 64 * 64
    who = [(s_, c) for s_ in range(n) for c in range(2)]
    params = {e: (workloads.ELEMS[e]['samples_per_clk'], workloads.ELEMS[e]['interp_ratio']) for e in (RDRV, RDLO)}
    drv = ChannelPlan(ps, cfg, 0, n, [(s_, c, RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, 0, n, [(s_, c, RDLO) for s_, c in who], params)
    iq_d = emu.synthesize(drv, out, n_clks * params[RDRV][0])
    iq_l = emu.synthesize(lo, out, n_clks * params[RDLO][0])
    pt = DemodPairTable(cfg, drv, lo)
    ft = FeedlineTable(pt, [[2 * s_, 2 * s_ + 1] for s_ in range(n)])
    axis, thr = calibrated_axes(emu, cfg, ft, iq_d, iq_l, out, 2 * n)
    reg = workloads.rb2q_gateset(2).reg_core
    seen = {}
    for name, gs in (('ideal', workloads.rb2q_gateset(2)), ('over', workloads.rb2q_gateset(2, over_rotation=0.02))):
        pops, result, states = emu.simulate_gates(cfg, gs, out, n, measure=True)
        acc, res = emu.demodulate_feedline(cfg, ft, iq_l, out, iq_drv=iq_d, states=states)
        stats, bits = emu.iq_stats(cfg, acc, res, pairs=pt, axis=axis, thr=thr, bits=True, states=states)
        torch.cuda.synchronize()
        st = qsim.state_bits(states, cfg, n)
        got = bits.cpu().numpy().view(np.uint32).reshape(n, 2).T                      # pairs are (shot, core) in order
        assert (res.cpu().numpy()[:, 0] == 1).all() and (result.cpu().numpy()[:, :, 2] == 0).all()
        np.testing.assert_array_equal(got, st)
        surv = qsim.readout_survival(got, reg, spg)
        # after its one readout a register is in a basis state: the final sample is the measured pair of bits
        np.testing.assert_array_equal(surv, qsim.survival(result, spg)[0])
        np.testing.assert_array_equal(surv, qsim.readout_survival(st, reg, spg))
        assert ReadoutStats(stats.cpu().numpy(), cfg, axis=axis, thr=thr).fidelity() == 1.0
        seen[name] = (st, surv)
    assert not seen['ideal'][0].any() and (seen['ideal'][1] == 1.0).all()
    assert seen['over'][0].any() and seen['over'][1].min() < 1.0 and seen['over'][1].mean() > 0.5
