"""dpemu_feedline_adc_res (csrc/resonator.hip) on the GPU: run_device ->
synthesize (the GPU DDS) -> feedline_adc(resonators=...) ->
demodulate_feedline, adc, acc and result bit for bit against the numpy
restatement (tests/resonator_ref.py, tests/feedline_ref.py) on the same GPU
event and iq arrays; the degenerate equivalence with feedline_adc_kernel; a
dispersive readout through the statistics stage; and the argument checks of
the C ABI."""

import ctypes as C
import math
import random

import numpy as np
import pytest

from distributed_processor_amd import _abi
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable, FeedlineTable, ResonatorTable
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from tests import feedline_ref, resonator_ref
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, freq_buffer
from tests.test_gpu_demod_iq import assembled
from tests.test_gpu_feedline import MEAS_CAP, exact_case, pipeline
from tests.test_resonator import (KAPPA, WINDOWS, check_dispersive, dispersive_case, dispersive_f_res, dispersive_lines,
                                  predicted_acc)

pytestmark = pytest.mark.gpu

N_CLKS = 1204                        # LO samples: 1,204 at 1:1, 4,816 at 16:4 -- multiples of 4, not of the 64-sample tile
POLE_MAX = ResonatorTable.POLE_MAX


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def random_table(pt, seed, adc_sigma=700):
    """per pair and state: a pole anywhere inside the bound (a third of them on it), a coupling of about 1 - |a|
    (a quarter of them: of about 1, so that single returns and line sums clip) at a random angle"""
    rng = random.Random(seed)
    coef = np.zeros((pt.n_pairs, 2, 4), np.int64)
    for p in range(pt.n_pairs):
        for s_ in (0, 1):
            mag = POLE_MAX if rng.random() < 0.33 else rng.uniform(0, POLE_MAX)
            th = rng.uniform(0, 2 * math.pi)
            coef[p, s_, 0], coef[p, s_, 1] = int(mag * math.cos(th)), int(mag * math.sin(th))      # (towards zero)
            k = rng.uniform(0.3, 1.5) * max(2 ** 30 - mag, 2 ** 19)
            if rng.random() < 0.25:
                k = rng.uniform(0.5, 1.0) * 2 ** 30
            th = rng.uniform(0, 2 * math.pi)
            k = min(k, 2 ** 30)
            coef[p, s_, 2], coef[p, s_, 3] = int(k * math.cos(th)), int(k * math.sin(th))
    return ResonatorTable.from_coefficients(pt, coef, adc_sigma)


def run_stage(emu, cfg, dev, tab):
    """the new stage and the demodulator on the pipeline's tensors: host (adc, acc, res)"""
    import torch
    adc = emu.feedline_adc(cfg, dev['ft'], dev['iq_d'], dev['out'], dev['iq_l'].shape[1], resonators=tab)
    assert emu.last_kernel() == 'feedline_res_kernel'
    acc, res = emu.demodulate_feedline(cfg, dev['ft'], dev['iq_l'], dev['out'], adc=adc)
    torch.cuda.synchronize()
    return adc, acc, res


def check_against_reference(cfg, host, pt, lines, tab, got, y_peak=None):
    adc, acc, res = got
    want_adc = resonator_ref.feedline_adc_res(cfg, pt.cols, lines, tab.coef, tab.adc_sigma, host['summary'],
                                              host['events'], host['iq_d'], host['iq_l'].shape[1], MEAS_CAP,
                                              y_peak=y_peak)
    np.testing.assert_array_equal(adc.cpu().numpy().view(np.uint32), want_adc)
    want_acc, want_res = feedline_ref.demod_feedline(cfg, pt.cols, lines, host['summary'], host['events'], want_adc,
                                                     host['iq_l'], MEAS_CAP)
    np.testing.assert_array_equal(res.cpu().numpy().view(np.uint32), want_res)
    np.testing.assert_array_equal(acc.cpu().numpy(), want_acc)
    return want_adc, want_acc, want_res


@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR], ids=['core_major', 'shot_major'])
@pytest.mark.parametrize('spc', [(16, 4), (1, 1)], ids=['16_4', '1_1'])
def test_bit_exact_against_reference(emu, spc, lane_order):
    """test_gpu_feedline's exact_case (4 cores in 3 groups, staggered strobes, a member without a drive, five
    readouts against meas_cap 4, a window clipped by n_samples), lines of 3 + 1 members, random coefficients,
    converter noise on"""
    import torch
    ps, cfg = exact_case(spc, lane_order, 6200 + 16 * spc[0] + spc[1])
    who = [(1000 + s_, c) for s_ in range(3) for c in range(4)]
    params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}
    lines = [ln for s_ in range(3) for ln in ([4 * s_ + 2, 4 * s_, 4 * s_ + 1], [4 * s_ + 3])]
    dev, host = pipeline(emu, ps, cfg, 3, 1000, who, params, N_CLKS, lines)
    pt = dev['pt']
    tab = random_table(pt, 77 + spc[0])
    got = run_stage(emu, cfg, dev, tab)
    adc, acc, res = check_against_reference(cfg, host, pt, lines, tab, got)
    assert host['iq_l'].shape[1] % 64 and (adc != host['adc']).mean() > 0.5         # ragged tiles; not the old trace
    half = np.concatenate([feedline_ref.s16(adc).ravel(), feedline_ref.s16(adc >> 16).ravel()])
    assert (half == 32767).any() and half.min() == -32767 and (np.abs(half) < 32767).mean() > 0.5    # the converter clips
    assert [int(w) for w in res[:, 0]] == [3] * 4 + [4] + [3] * 7 and np.abs(acc[2].astype(np.int64)).max() > 10 ** 4
    assert not host['iq_d'][who.index((1000, 1))].any()                            # the member without a drive
    # demodulate_feedline makes the same trace itself when given the table
    acc2, res2 = emu.demodulate_feedline(cfg, dev['ft'], dev['iq_l'], dev['out'], iq_drv=dev['iq_d'], resonators=tab)
    assert torch.equal(acc2, got[1]) and torch.equal(res2, got[2])
    # without noise the trace differs; the noise of a line follows its first member
    quiet = ResonatorTable.from_coefficients(pt, tab.coef, 0)
    adc0 = emu.feedline_adc(cfg, dev['ft'], dev['iq_d'], dev['out'], host['iq_l'].shape[1], resonators=quiet)
    want0 = resonator_ref.feedline_adc_res(cfg, pt.cols, lines, tab.coef, 0, host['summary'], host['events'],
                                           host['iq_d'], host['iq_l'].shape[1], MEAS_CAP)
    np.testing.assert_array_equal(adc0.cpu().numpy().view(np.uint32), want0)
    assert (want0 != adc).any()


def test_sixteen_members_on_one_line(emu):
    """4 shots x 4 cores, all 16 pairs on a single line (DPEMU_FEEDLINE_MAX), in a shuffled order"""
    ps, cfg = exact_case((16, 4), _abi.LANES_SHOT_MAJOR, 6300)
    who = [(1000 + s_, c) for s_ in range(4) for c in range(4)]
    order = list(range(16))
    random.Random(2).shuffle(order)
    dev, host = pipeline(emu, ps, cfg, 4, 1000, who, {RDRV: (16, 16), RDLO: (4, 4)}, N_CLKS, [order])
    tab = random_table(dev['pt'], 78)
    adc, _, _ = check_against_reference(cfg, host, dev['pt'], [order], tab, run_stage(emu, cfg, dev, tab))
    assert adc.shape == (1, 4 * N_CLKS) and (feedline_ref.s16(adc) == 32767).any()


def test_more_members_than_a_workgroup(emu):
    """70 shots x 4 cores at 1:1: 70 lines of 3, then 14 lines of 5 -- 280 members.  A workgroup takes whole
    lines up to 16 members: five lines of 3 or three of 5, and the next line would straddle the boundary if
    lines were not kept whole"""
    ps, cfg = exact_case((1, 1), _abi.LANES_SHOT_MAJOR, 6400)
    n = 70
    who = [(1000 + s_, c) for s_ in range(n) for c in range(4)]
    lines = [[4 * s_ + 1, 4 * s_ + 2, 4 * s_] for s_ in range(n)] + \
            [[4 * s_ + 3 for s_ in range(5 * g, 5 * g + 5)] for g in range(n // 5)]
    filled, cur = [], 0
    for ln in lines:                                         # the host's greedy packing
        if cur + len(ln) > 16:
            filled.append(cur)
            cur = 0
        cur += len(ln)
    assert sum(filled) + cur == 280 and len(filled) == 18 and set(filled) == {15}
    dev, host = pipeline(emu, ps, cfg, n, 1000, who, {RDRV: (1, 1), RDLO: (1, 1)}, N_CLKS, lines)
    tab = random_table(dev['pt'], 79)
    check_against_reference(cfg, host, dev['pt'], lines, tab, run_stage(emu, cfg, dev, tab))


def test_pole_at_the_bound_on_resonance(emu):
    """2 shots x 2 cores at 1:1, a full-scale square pulse of 8,000 samples on a resonator at |a| = 1 - 2^-12
    whose angle is the drive's phase step: |y| passes 10^8, the 64-bit products carry it"""
    f_d = [0x0A000000, 0x35000000]
    env = np.full(4 * 2000, SQUARE, np.uint32)
    read = [dict(A=65535, ph_d=0, ph_lo=0, L_d=2000, L_lo=2000, lo_at=10)]
    prog = {c: assembled(ro_program(read), env, env, freq_buffer(f_d[c], 1), freq_buffer(f_d[c], 1)) for c in range(2)}
    ps = ProgramSet([prog], cores_per_shot=2)
    cfg = _abi.make_config(2, max_cycles=1 << 20, event_cap=16, meas_cap=MEAS_CAP, meas_latency=32, seed=41, p1=0.5,
                           demod=dict(drv_elem=RDRV, cpw=4, delay=10, sigma=3.0, axis=0.2))
    who = [(7 + s_, c) for s_ in range(2) for c in range(2)]
    lines = [[0, 1], [3, 2]]
    dev, host = pipeline(emu, ps, cfg, 2, 7, who, {RDRV: (1, 1), RDLO: (1, 1)}, 8204, lines)
    pt = dev['pt']
    coef = np.zeros((4, 2, 4), np.int64)
    for p in range(4):
        th = 2 * math.pi * f_d[int(pt.cols['core'][p])] / 2.0 ** 32
        for s_ in (0, 1):
            coef[p, s_] = (int(POLE_MAX * math.cos(th)), int(POLE_MAX * math.sin(th)), (1 + s_) << 15, -(1 << 15))
    tab = ResonatorTable.from_coefficients(pt, coef, 50)
    peak = []
    adc, _, _ = check_against_reference(cfg, host, pt, lines, tab, run_stage(emu, cfg, dev, tab), y_peak=peak)
    print('peak |y| component', peak[0])
    assert 10 ** 8 < peak[0] < 2 ** 28
    assert 2000 < np.abs(feedline_ref.s16(adc)).max() < 32767            # the return of |y| ~ 10^8 does not clip


def test_degenerate_equivalence(emu):
    """pole 0, the coupling of ro_theta, no noise: feedline_adc_kernel's trace at unit gains, bit for bit"""
    for spc in ((16, 4), (1, 1)):
        ps, cfg = exact_case(spc, _abi.LANES_CORE_MAJOR, 6500 + spc[0], gain=(1.0, 1.0))
        assert cfg.ro_gain[0] == cfg.ro_gain[1] == 65536
        who = [(1000 + s_, c) for s_ in range(3) for c in range(4)]
        params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}
        lines = [ln for s_ in range(3) for ln in ([4 * s_ + 2, 4 * s_, 4 * s_ + 1], [4 * s_ + 3])]
        dev, host = pipeline(emu, ps, cfg, 3, 1000, who, params, N_CLKS, lines)
        tab = ResonatorTable.from_coefficients(dev['pt'], resonator_ref.degenerate_coef(cfg, 12))
        adc, acc, res = run_stage(emu, cfg, dev, tab)
        np.testing.assert_array_equal(adc.cpu().numpy().view(np.uint32), host['adc'])
        np.testing.assert_array_equal(acc.cpu().numpy(), host['acc'])
        assert host['adc'].any()


def test_dispersive_readout_through_the_statistics(emu):
    """tests/test_resonator.py's dispersive case on the GPU's outputs: 3 cores x 64 shots, fidelity 1.0, the
    centroids and the short window's separation where the transient formula puts them"""
    runs = {}
    n, shot0 = 64, 500
    for w in WINDOWS:
        cfg, progs, f, env, n_clks = dispersive_case(w)
        prog = {c: assembled(progs[c], env, env, freq_buffer(f[c], 4), freq_buffer(f[c], 4)) for c in range(4)}
        ps = ProgramSet([prog], cores_per_shot=4)
        who = [(shot0 + s_, c) for s_ in range(n) for c in range(4)]
        emu.load(ps)
        out = alloc_device_outputs(cfg, n, want=('summary', 'events'))
        emu.run_device(cfg, n, shot0, out)
        drv = ChannelPlan(ps, cfg, shot0, n, [(s_, c, RDRV) for s_, c in who], {RDRV: (4, 4), RDLO: (4, 4)})
        lo = ChannelPlan(ps, cfg, shot0, n, [(s_, c, RDLO) for s_, c in who], {RDRV: (4, 4), RDLO: (4, 4)})
        iq_d, iq_l = emu.synthesize(drv, out, 4 * n_clks), emu.synthesize(lo, out, 4 * n_clks)
        pt = DemodPairTable(cfg, drv, lo)
        lines = dispersive_lines(pt.cols)
        ft = FeedlineTable(pt, lines)
        tab = ResonatorTable(pt, dispersive_f_res(pt.cols['core']), KAPPA)
        acc, res = emu.demodulate_feedline(cfg, ft, iq_l, out, iq_drv=iq_d, resonators=tab)
        assert emu.last_kernel() == 'feedline_demod_kernel'
        host = [t.cpu().numpy() for t in (out['summary'], out['events'], iq_d, iq_l)]
        runs[w] = (acc.cpu().numpy(), res.cpu().numpy().view(np.uint32), predicted_acc(cfg, pt.cols, lines, tab, *host))
    check_dispersive(cfg, pt.cols, tab, runs)


def test_timing_records_the_kernel(emu):
    ps, cfg = exact_case((1, 1), _abi.LANES_CORE_MAJOR, 6600)
    who = [(1000, c) for c in range(4)]
    dev, _ = pipeline(emu, ps, cfg, 1, 1000, who, {RDRV: (1, 1), RDLO: (1, 1)}, 400, [[0, 1, 2, 3]])
    tab = random_table(dev['pt'], 80)
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        emu.feedline_adc(cfg, dev['ft'], dev['iq_d'], dev['out'], 400, resonators=tab)
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 1 and 0 < ms[0] < 100 and emu.last_kernel() == 'feedline_res_kernel'


def test_refusals_at_the_c_abi(emu):
    """every DPEMU_E_INVALID condition, before any launch: -22 and a message that names the field"""
    import torch
    cfg = _abi.make_config(2, event_cap=16, meas_cap=4, demod=dict(drv_elem=RDRV))
    dev = torch.device('cuda', 0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=dev)
    summ, ev, iq_d, adc = z(4, 8), z(16, 4, 4), z(3, 64), z(2, 16)
    ptr = {k: v.data_ptr() for k, v in dict(summary=summ, events=ev, iq_drv=iq_d, adc=adc).items()}
    lim = POLE_MAX

    def call(lines=((0, 1), (2,)), n_lines=None, first=None, meas_cap=4, event_cap=16, n_lo=16, cfg_=cfg,
             no_pairs=False, no_lines=False, no_res=False, no_coef=False, coef=None, sigma=5, **kw):
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
        k = np.zeros((3, 2, 4), np.int32)
        k[..., 0], k[..., 2] = lim, 1 << 30
        for at, v in (coef or {}).items():
            k[at] = v
        rs = _abi.Resonators(None if no_coef else k.ctypes.data, sigma)
        rc = emu._L.dpemu_feedline_adc_res(emu._h, C.addressof(cfg_) if cfg_ is not None else None,
                                           None if no_pairs else C.addressof(st), None if no_lines else C.addressof(ls),
                                           None if no_res else C.addressof(rs), p['summary'], p['events'], p['iq_drv'],
                                           p['adc'], None)
        return rc, emu._L.dpemu_last_error(emu._h)

    gain = _abi.make_config(2, event_cap=16, meas_cap=4, demod=dict(drv_elem=RDRV))
    gain.ro_gain[1] = 65537                                  # dpemu_feedline_adc's bound: not read here
    for kw in (dict(), dict(lines=((2, 0),)), dict(cfg_=gain), dict(sigma=0),
               dict(coef={(0, 0, 0): 0, (0, 0, 1): -lim, (1, 1, 2): -(1 << 30), (1, 1, 3): 1 << 30})):
        rc, msg = call(**kw)
        assert rc == 0 and emu.last_kernel() == 'feedline_res_kernel', (kw, rc, msg)
    torch.cuda.synchronize()
    adc.zero_()
    refused = ((dict(cfg_=None), b'cfg'), (dict(no_pairs=True), b'pairs'), (dict(no_lines=True), b'lines'),
               (dict(no_res=True), b'res is NULL'), (dict(no_coef=True), b'coef is NULL'),
               (dict(summary=None), b'summary'), (dict(events=None), b'events'), (dict(adc=None), b'adc'),
               (dict(iq_drv=None), b'iq_drv'),
               (dict(n_lines=0), b'n_lines'), (dict(lines=((0, 1), ()), first=[0, 2, 2]), b'empty'),
               (dict(lines=(tuple([0] * 17),)), b'17 members'), (dict(lines=((0, 3),)), b'member 3'),
               (dict(lines=((0, 1), (1, 2))), b'two lines'), (dict(lines=((0, 0, 1), (2,))), b'two lines'),
               (dict(spc_drv=[16, 8, 16]), b'spc_drv'), (dict(spc_drv=[4, 2, 4], spc_lo=[4, 2, 4]), b'spc_'),
               (dict(n_lo=0), b'n_samples_lo'), (dict(n_lo=18), b'n_samples_lo'),
               (dict(adc=ptr['adc'] + 4), b'adc must be 16-byte aligned'), (dict(event_cap=1025), b'event_cap'),
               (dict(meas_cap=0), b'meas_cap'), (dict(meas_cap=33), b'meas_cap'), (dict(lane=[0, 4, 1]), b'lane'),
               (dict(core=[0, 2, 1]), b'core'), (dict(first=[1, 2, 3]), b'line_first'),
               (dict(coef={(2, 1, 0): lim + 1}), b'pair 2 state 1: pole'), (dict(coef={(0, 0, 1): 1 << 18}), b'pole'),
               (dict(coef={(1, 0, 0): -(2 ** 31)}), b'pole'),
               (dict(coef={(1, 0, 2): (1 << 30) + 1}), b'pair 1 state 0: coupling'),
               (dict(coef={(0, 1, 3): -(1 << 30) - 1}), b'coupling'))
    for kw, field in refused:
        rc, msg = call(**kw)
        assert rc == -22 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert not adc.any().item()                              # nothing was launched
