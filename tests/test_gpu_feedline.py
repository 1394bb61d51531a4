"""dpemu_feedline_adc / dpemu_demod_feedline (csrc/feedline.hip) on the GPU:
run_device -> synthesize (the GPU DDS) -> feedline_adc -> demodulate_feedline,
bit for bit against the numpy restatement (tests/feedline_ref.py) on the same
GPU event and iq arrays; the degenerate equivalence with dpemu_demod_iq;
readout crosstalk through the statistics stage; and the argument checks of the
C ABI."""

import ctypes as C
import math
import random

import numpy as np
import pytest

from distributed_processor_amd import _abi, isa
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable, FeedlineTable
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from distributed_processor_amd.readout import ReadoutStats
from tests import feedline_ref, iq_stats_ref
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, freq_buffer
from tests.test_gpu_demod_iq import assembled

pytestmark = pytest.mark.gpu

N_CLKS = 1200
MEAS_CAP = 4


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def pipeline(emu, ps, cfg, n_shots, shot0, who, params, n_clks, lines=None):
    """run, synthesise the drive and LO channels of the (shot, core) list `who`,
    then both feedline stages over `lines` (default: FeedlineTable's).  Returns
    the device tensors and tables, and host copies of everything compared."""
    import torch
    emu.load(ps)
    out = alloc_device_outputs(cfg, n_shots, want=('summary', 'events'))
    emu.run_device(cfg, n_shots, shot0, out)
    drv = ChannelPlan(ps, cfg, shot0, n_shots, [(s_, c, RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, shot0, n_shots, [(s_, c, RDLO) for s_, c in who], params)
    iq_d = emu.synthesize(drv, out, n_clks * params[RDRV][0])
    iq_l = emu.synthesize(lo, out, n_clks * params[RDLO][0])
    pt = DemodPairTable(cfg, drv, lo)
    ft = FeedlineTable(pt, lines)
    adc = emu.feedline_adc(cfg, ft, iq_d, out, iq_l.shape[1])
    assert emu.last_kernel() == 'feedline_adc_kernel'
    acc, res = emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc)
    assert emu.last_kernel() == 'feedline_demod_kernel'
    torch.cuda.synchronize()
    dev = dict(out=out, drv=drv, lo=lo, iq_d=iq_d, iq_l=iq_l, adc=adc, acc=acc, res=res, pt=pt, ft=ft)
    host = dict(summary=out['summary'].cpu().numpy(), events=out['events'].cpu().numpy(), iq_d=iq_d.cpu().numpy(),
                iq_l=iq_l.cpu().numpy(), adc=adc.cpu().numpy().view(np.uint32), acc=acc.cpu().numpy(),
                res=res.cpu().numpy().view(np.uint32))
    return dev, host


def exact_case(spc, lane_order, seed, gain=None):
    """4 cores in 3 groups (shot s runs group s % 3), about 1,200 clocks, windows
    of 1, 7 and 200 words; every core's strobes at its own times (staggered);
    group 1's core 1 has no drive pulse; group 2's core 0 has 5 reads (meas_cap
    4); group 0's core 2 starts its 200-word window at ~700, so n_samples clips
    it; three detunings; random 17-bit phases, thetas, gains, axes; noise on."""
    rng = random.Random(seed)
    env = [np.array([((rng.randint(-30000, 30000) & 0xFFFF) << 16) | (rng.randint(-30000, 30000) & 0xFFFF)
                     for _ in range(1000)], np.uint32) for _ in range(2)]
    groups = []
    for g in range(3):
        prog = {}
        for c in range(4):
            f_d = rng.getrandbits(32)
            dets = (0, rng.randint(-40, 40), rng.randint(-2 ** 26, 2 ** 26))
            fb_lo = np.concatenate([freq_buffer((f_d - d) & 0xFFFFFFFF, spc[1]) for d in dets])

            def read(L, k, gap):
                return dict(A=rng.randint(30000, 65535), ph_d=rng.getrandbits(17), ph_lo=rng.getrandbits(17),
                            L_d=L, L_lo=L, fi_lo=k % 3, lo_at=20 + 3 * c, gap=gap)
            if g == 2 and c == 0:
                reads = [read(1, 0, 60), read(7, 1, 80), read(200, 2, 880), read(1, 0, 60), read(7, 1, 60)]
            elif g == 0 and c == 2:
                reads = [read(1, 0, 60), read(7, 1, 620), read(200, 2, 100)]
            else:
                reads = [read(1, 0, 60 + 7 * c), read(7, 1, 80 + 11 * c), read(200, 2, 100)]
            words = ro_program(reads)
            if g == 1 and c == 1:                     # the LO pulses alone
                words = [w for i, w in enumerate(words) if i == 0 or i % 2 == 0 or i == len(words) - 1]
            prog[c] = assembled(words, env[0], env[1], freq_buffer(f_d, spc[0]), fb_lo)
        groups.append(prog)
    ps = ProgramSet(groups, cores_per_shot=4)
    cfg = _abi.make_config(4, n_groups=3, max_cycles=1 << 20, event_cap=16, meas_cap=MEAS_CAP, meas_latency=32,
                           seed=seed, p1=[0.3, 0.6, 0.5, 0.7], lane_order=lane_order,
                           demod=dict(drv_elem=RDRV, cpw=4, delay=20, theta=(rng.uniform(-4, 4), rng.uniform(-4, 4)),
                                      gain=gain or (0.5 + 0.5 * rng.random(), 0.5 + 0.5 * rng.random()),
                                      axis=[rng.uniform(-4, 4) for _ in range(4)],
                                      sigma=rng.uniform(5, 250), thr=rng.randint(-10 ** 6, 10 ** 6)))
    return ps, cfg


def readouts_of(cfg, host, pt, i):
    return feedline_ref.kept_readouts(cfg, host['summary'].view(np.uint32), host['events'].view(np.uint32),
                                      int(pt.cols['lane'][i]), MEAS_CAP, cfg.event_cap)


def check_against_reference(cfg, host, pt, lines):
    want_adc, want_acc, want_res = feedline_ref.feedline(cfg, pt.cols, lines, host['summary'], host['events'],
                                                         host['iq_d'], host['iq_l'], MEAS_CAP)
    np.testing.assert_array_equal(host['adc'], want_adc)
    np.testing.assert_array_equal(host['res'], want_res)
    np.testing.assert_array_equal(host['acc'], want_acc)
    return want_adc, want_acc, want_res


def check_exact_case(cfg, host, pt, who, spc, adc, acc, res):
    """exact_case holds what it claims (asserted on the arrays the comparison ran on)"""
    reads = {w: readouts_of(cfg, host, pt, i) for i, w in enumerate(who)}
    n_lo = N_CLKS * spc[1]
    summ, ev = host['summary'].view(np.uint32), host['events'].view(np.uint32)
    strobes = {w: sum(1 for e in ev[:min(int(summ[lane, 2]), cfg.event_cap), lane]
                      if e[1] >> 28 == 0 and (e[1] >> 24) & 3 == RDLO)
               for w, lane in zip(who, pt.cols['lane'].tolist())}
    assert strobes[(1001, 0)] == 5 and len(reads[(1001, 0)]) == MEAS_CAP              # more readouts than meas_cap
    assert all(len(r) == 3 for w, r in reads.items() if w != (1001, 0))
    assert not host['iq_d'][who.index((1000, 1))].any() and host['iq_l'][who.index((1000, 1))].any()    # no drive
    t, pe = reads[(1002, 2)][2]                                                       # clipped at n_samples
    assert t * spc[1] < n_lo < (t + ((pe >> 12) & 0xFFF) * 4) * spc[1]
    t, pe = reads[(1000, 0)][2]
    assert (t + ((pe >> 12) & 0xFFF) * 4) * spc[1] <= n_lo
    for s_ in range(3):                                                               # staggered members
        seen = [np.array([sum(t <= n for t, _ in reads[(1000 + s_, c)]) for n in range(N_CLKS)]) for c in range(3)]
        assert (seen[0] != seen[1]).any() and (seen[1] != seen[2]).any()
    half = np.concatenate([feedline_ref.s16(adc[0::2]).ravel(), feedline_ref.s16(adc[0::2] >> 16).ravel()])
    assert 0 < (np.abs(half) == 32767).sum() < half.size // 4 and half.min() == -32767        # the converter clips
    assert np.abs(acc[2].astype(np.int64)).max() > 10 ** 6 and not np.delete(acc[3], 4, axis=0).any()
    assert [int(w) for w in res[:, 0]] == [3] * 4 + [4] + [3] * 7


@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR], ids=['core_major', 'shot_major'])
@pytest.mark.parametrize('spc', [(16, 4), (1, 1)], ids=['16_4', '1_1'])
def test_bit_exact_against_reference(emu, spc, lane_order):
    ps, cfg = exact_case(spc, lane_order, 5200 + 16 * spc[0] + spc[1])
    who = [(1000 + s_, c) for s_ in range(3) for c in range(4)]
    params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}          # interp = spc: 4 clocks per env word
    lines = [ln for s_ in range(3) for ln in ([4 * s_ + 2, 4 * s_, 4 * s_ + 1], [4 * s_ + 3])]
    dev, host = pipeline(emu, ps, cfg, 3, 1000, who, params, N_CLKS, lines)
    pt = dev['pt']
    adc, acc, res = check_against_reference(cfg, host, pt, lines)
    check_exact_case(cfg, host, pt, who, spc, adc, acc, res)
    # demodulate_feedline makes the same ADC trace itself when none is passed
    import torch
    acc2, res2 = emu.demodulate_feedline(cfg, dev['ft'], dev['iq_l'], dev['out'], iq_drv=dev['iq_d'])
    assert torch.equal(acc2, dev['acc']) and torch.equal(res2, dev['res'])


def test_sixteen_members_on_one_line(emu):
    """4 shots x 4 cores, all 16 pairs on a single line (DPEMU_FEEDLINE_MAX)"""
    ps, cfg = exact_case((16, 4), _abi.LANES_SHOT_MAJOR, 5300)
    who = [(1000 + s_, c) for s_ in range(4) for c in range(4)]
    order = list(range(16))
    random.Random(1).shuffle(order)
    dev, host = pipeline(emu, ps, cfg, 4, 1000, who, {RDRV: (16, 16), RDLO: (4, 4)}, N_CLKS, [order])
    adc, acc, res = check_against_reference(cfg, host, dev['pt'], [order])
    assert adc.shape == (1, 4 * N_CLKS) and dev['ft'].member.tolist() == order
    assert (feedline_ref.s16(adc) == 32767).any() and (feedline_ref.s16(adc >> 16) == -32767).any()


def test_degenerate_equivalence(emu):
    """one member per line with unit gains (and no window that reaches the
    lane's next readout strobe): Emulator.demodulate's acc and result, bit for bit"""
    import torch
    for spc in ((16, 4), (1, 1)):
        ps, cfg = exact_case(spc, _abi.LANES_CORE_MAJOR, 5400 + spc[0], gain=(1.0, 1.0))
        assert cfg.ro_gain[0] == cfg.ro_gain[1] == 65536
        who = [(1000 + s_, c) for s_ in range(3) for c in range(4)]
        params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}
        dev, host = pipeline(emu, ps, cfg, 3, 1000, who, params, N_CLKS, [[i] for i in range(12)])
        for i in range(12):                                  # the precondition
            r = readouts_of(cfg, host, dev['pt'], i)
            assert all(t + ((pe >> 12) & 0xFFF) * 4 <= r[k + 1][0] for k, (t, pe) in enumerate(r[:-1]))
        acc, res = emu.demodulate(cfg, dev['drv'], dev['iq_d'], dev['lo'], dev['iq_l'], dev['out'], pairs=dev['pt'])
        assert torch.equal(res, dev['res']) and torch.equal(acc, dev['acc'])
        assert np.abs(host['acc'][2].astype(np.int64)).max() > 10 ** 6


def crosstalk_case(dets, seed=0xC0FFEE):
    """3 reading cores (a fourth idles) with the same program: a square 64-word
    drive and LO pulse, amplitude word 20000 (3 x 10000 < 32767), thetas (0,
    pi), p1 = 0.5, core c's tone at f0 + dets[c] with its LO on it"""
    read = [dict(A=20000, ph_d=0, ph_lo=0, L_d=66, L_lo=64, lo_at=24)]
    f0 = 0x0C000000
    env = np.full(300, SQUARE, np.uint32)
    prog = {c: assembled(ro_program(read), env, env, freq_buffer((f0 + dets[c]) & 0xFFFFFFFF, 4),
                         freq_buffer((f0 + dets[c]) & 0xFFFFFFFF, 4)) for c in range(3)}
    prog[3] = assembled([isa.done_cmd()], env, env, freq_buffer(f0, 4), freq_buffer(f0, 4))
    ps = ProgramSet([prog], cores_per_shot=4)
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=16, meas_cap=MEAS_CAP, meas_latency=32, seed=seed, p1=0.5,
                           lane_order=_abi.LANES_SHOT_MAJOR,
                           demod=dict(drv_elem=RDRV, cpw=4, delay=20, theta=(0.0, math.pi), sigma=1.0, axis=0.3))
    return ps, cfg


def fitted_confusion_gpu(emu, cfg, acc, res, pt):
    """fit the discriminator on the statistics of (acc, res), measure with it: (confusion [C, 2, 2], fidelity)"""
    import torch
    stats, _ = emu.iq_stats(cfg, acc, res, pairs=pt)
    torch.cuda.synchronize()
    d = ReadoutStats(stats.cpu().numpy(), cfg).fit()
    assert d.fitted[:3].all()
    stats, _ = emu.iq_stats(cfg, acc, res, pairs=pt, axis=d.axis_words, thr=d.thr)
    torch.cuda.synchronize()
    rs = ReadoutStats(stats.cpu().numpy(), cfg, axis=d.axis_words, thr=d.thr)
    return rs.confusion[0], rs.fidelity()


def fitted_confusion_ref(cfg, acc, res, pt):
    core, shot = pt.cols['core'], pt.cols['shot']
    t, _ = iq_stats_ref.iq_stats(cfg, acc, res[:, 0], core=core, shot=shot)
    d = ReadoutStats(t, cfg).fit()
    t, _ = iq_stats_ref.iq_stats(cfg, acc, res[:, 0], core=core, shot=shot, axis=d.axis_words, thr=d.thr)
    rs = ReadoutStats(t, cfg, axis=d.axis_words, thr=d.thr)
    return rs.confusion[0], rs.fidelity()


def test_crosstalk_through_the_statistics(emu):
    """3 cores x 64 shots on one feedline per shot.  Tones a whole number of
    turns per window apart: the fitted discriminator's fidelity is that of the
    un-multiplexed dpemu_demod_iq run.  Identical tones: every accumulator
    follows the majority of the three prepared states, the confusion counts are
    the reference's and those of the draws themselves, and the fidelity -- 0.75
    in expectation -- is below 0.9 (this seed: 141 / 192 = 0.734 from the draws alone, a
    CPU computation that needs no waveform)."""
    n, shot0, N = 64, 500, 256
    who = [(shot0 + s_, c) for s_ in range(n) for c in range(3)]
    params = {RDRV: (4, 4), RDLO: (4, 4)}
    step = 2 ** 32 // N                                       # one turn per 256-clock window
    for dets, same_tone in (((0, 3 * step, 7 * step), False), ((0, 0, 0), True)):
        ps, cfg = crosstalk_case(dets)
        dev, host = pipeline(emu, ps, cfg, n, shot0, who, params, 320)
        pt, ft = dev['pt'], dev['ft']
        assert ft.n_lines == n and all(len(ln) == 3 for ln in ft.lines)
        assert max(np.abs(feedline_ref.s16(host['adc'])).max(), np.abs(feedline_ref.s16(host['adc'] >> 16)).max()) < 32767
        conf, fid = fitted_confusion_gpu(emu, cfg, dev['acc'], dev['res'], pt)
        st = iq_stats_ref.states(cfg, pt.cols['shot'], pt.cols['core'], 0).reshape(n, 3)
        if not same_tone:
            acc1, res1 = emu.demodulate(cfg, dev['drv'], dev['iq_d'], dev['lo'], dev['iq_l'], dev['out'], pairs=pt)
            conf1, fid1 = fitted_confusion_gpu(emu, cfg, acc1, res1, pt)
            print('orthogonal tones: fidelity', fid, 'un-multiplexed', fid1)
            assert fid == fid1 == 1.0
            np.testing.assert_array_equal(conf, conf1)
            continue
        _, want_acc, want_res = check_against_reference(cfg, host, pt, ft.lines)
        conf_ref, fid_ref = fitted_confusion_ref(cfg, want_acc, want_res, pt)
        major = (st.sum(axis=1, keepdims=True) >= 2).astype(np.int64) + 0 * st
        conf_draws = np.zeros((4, 2, 2), np.int64)
        for c in range(3):
            for s_, o in zip(st[:, c], major[:, c]):
                conf_draws[c, s_, o] += 1
        print('identical tones: fidelity', fid, 'reference', fid_ref, 'confusion', conf[:3].tolist())
        np.testing.assert_array_equal(conf, conf_ref)
        np.testing.assert_array_equal(conf, conf_draws)
        assert fid == fid_ref < 0.9 and fid > 0.6


def test_timing_records_the_main_kernels(emu):
    ps, cfg = crosstalk_case((0, 0, 0))
    who = [(s_, c) for s_ in range(2) for c in range(3)]
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        pipeline(emu, ps, cfg, 2, 0, who, {RDRV: (4, 4), RDLO: (4, 4)}, 320)
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 5 and all(0 < v < 100 for v in ms)    # the run, two syntheses, the two feedline kernels


def test_refusals_at_the_c_abi(emu):
    """every DPEMU_E_INVALID condition, before any launch: -22 and a message
    that names the field; dpemu_last_kernel after each accepted stage"""
    import torch
    cfg = _abi.make_config(2, event_cap=16, meas_cap=4, demod=dict(drv_elem=RDRV))
    dev = torch.device('cuda', 0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev)
    summ, ev, iq_d, iq_l = z(4, 8), z(16, 4, 4), z(3, 64), z(3, 16)
    adc, acc, res = z(2, 16), z(4, 3, 2), z(3, 2)
    ptr = {k: v.data_ptr() for k, v in dict(summary=summ, events=ev, iq_drv=iq_d, iq_lo=iq_l, adc=adc, acc=acc,
                                            result=res).items()}

    def call(stage, lines=((0, 1), (2,)), n_lines=None, first=None, meas_cap=4, event_cap=16, n_lo=16, cfg_=cfg,
             no_pairs=False, no_lines=False, **kw):
        a = dict(lane=[0, 3, 1], core=[0, 1, 1], drv_row=[0, 1, 2], lo_row=[0, 1, 2], spc_drv=[16, 16, 16],
                 spc_lo=[4, 4, 4])
        a.update({k: v for k, v in kw.items() if k in a})
        p = dict(ptr)
        p.update({k: v for k, v in kw.items() if k in p})
        arr = {k: np.array(v, np.uint32) for k, v in a.items()}
        arr['shot'] = np.array([5, 6, 6], np.uint64)
        st = _abi.DemodPairs(3, 4, event_cap, meas_cap, 64, n_lo)
        for k, v in arr.items():
            setattr(st, k, v.ctypes.data)
        lf = np.array(first if first is not None else np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]),
                      np.uint32)
        mem = np.array([m for ln in lines for m in ln] or [0], np.uint32)
        ls = _abi.Feedlines(len(lines) if n_lines is None else n_lines, lf.ctypes.data, mem.ctypes.data)
        head = (emu._h, C.addressof(cfg_) if cfg_ is not None else None, None if no_pairs else C.addressof(st),
                None if no_lines else C.addressof(ls), p['summary'], p['events'])
        if stage == 'adc':
            rc = emu._L.dpemu_feedline_adc(*head, p['iq_drv'], p['adc'], None)
        else:
            rc = emu._L.dpemu_demod_feedline(*head, p['adc'], p['iq_lo'], p['acc'], p['result'], None)
        return rc, emu._L.dpemu_last_error(emu._h)

    assert call('adc')[0] == 0 and emu.last_kernel() == 'feedline_adc_kernel'
    assert call('demod')[0] == 0 and emu.last_kernel() == 'feedline_demod_kernel'
    assert call('adc', lines=((2, 0),))[0] == 0               # the ADC stage takes a table with unlisted pairs
    torch.cuda.synchronize()
    for t in (adc, acc, res):
        t.zero_()
    gain = _abi.make_config(2, event_cap=16, meas_cap=4, demod=dict(drv_elem=RDRV))
    gain.ro_gain[1] = 65537
    common = ((dict(cfg_=None), b'cfg'), (dict(no_pairs=True), b'pairs'), (dict(no_lines=True), b'lines'),
              (dict(summary=None), b'summary'), (dict(events=None), b'events'), (dict(adc=None), b'adc'),
              (dict(n_lines=0), b'n_lines'), (dict(lines=((0, 1), ()), first=[0, 2, 2]), b'empty'),
              (dict(lines=(tuple([0] * 17),)), b'17 members'), (dict(lines=((0, 3),)), b'member 3'),
              (dict(lines=((0, 1), (1, 2))), b'two lines'), (dict(lines=((0, 0, 1), (2,))), b'two lines'),
              (dict(spc_drv=[16, 8, 16]), b'spc_drv'), (dict(spc_drv=[4, 2, 4], spc_lo=[4, 2, 4]), b'spc_'),
              (dict(n_lo=0), b'n_samples_lo'), (dict(n_lo=18), b'n_samples_lo'),
              (dict(adc=ptr['adc'] + 4), b'adc must be 16-byte aligned'), (dict(event_cap=1025), b'event_cap'),
              (dict(meas_cap=0), b'meas_cap'), (dict(meas_cap=33), b'meas_cap'), (dict(lane=[0, 4, 1]), b'lane'),
              (dict(core=[0, 2, 1]), b'core'), (dict(first=[1, 2, 3]), b'line_first'))
    only = {'adc': ((dict(iq_drv=None), b'iq_drv'), (dict(cfg_=gain), b'ro_gain')),
            'demod': ((dict(iq_lo=None), b'iq_lo'), (dict(acc=None), b'acc'), (dict(result=None), b'result'),
                      (dict(iq_lo=ptr['iq_lo'] + 8), b'iq_lo must be 16-byte aligned'),
                      (dict(lines=((0, 1),)), b'pair 2 is in no line'))}
    for stage in ('adc', 'demod'):
        for kw, field in common + only[stage]:
            rc, msg = call(stage, **kw)
            assert rc == -22 and field in msg, (stage, kw, rc, msg)
    torch.cuda.synchronize()
    assert not adc.any().item() and not acc.any().item() and not res.any().item()     # nothing was launched
