"""dpemu_feedline_traces (csrc/traces.hip) on the GPU: run_device -> synthesize
(the GPU DDS) -> feedline_adc -> feedline_traces, the table bit for bit against
the numpy restatement (tests/traces_ref.py) on the same GPU event and iq
arrays; hand-built full-range inputs; more pairs than a workgroup's chunk and
than one of its staging runs; the
sum identity with feedline_demod_kernel; the matched-filter loop end to end;
timing; and the argument checks of the C ABI.  What the inputs reach is
asserted on the CPU, from the references alone, in tests/test_traces.py."""

import ctypes as C
import random

import numpy as np
import pytest

from distributed_processor_amd import _abi
from distributed_processor_amd.dds import ResonatorTable
from distributed_processor_amd.emulator import Emulator, ProgramSet
from distributed_processor_amd.readout import ReadoutTraces
from tests import feedline_ref, handbuilt as hb, iq_stats_ref, resonator_ref, traces_ref
from tests import test_traces as T
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, freq_buffer
from tests.test_gpu_demod_iq import assembled
from tests.test_gpu_feedline import MEAS_CAP, exact_case, pipeline
from tests.test_gpu_resonator import random_table
from tests.test_resonator import KAPPA, dispersive_f_res, dispersive_lines

pytestmark = pytest.mark.gpu

N_CLKS = T.EXACT_CLKS                # LO samples: 1,204 at 1:1, 4,816 at 16:4 -- multiples of 4, not of 64
GARBAGE = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C').view(np.int32)).cuda()


def gpu_traces(emu, cfg, ft, iq_l, out, adc, n_bins, bin_clocks, by_slot, traces=None):
    import torch
    got = emu.feedline_traces(cfg, ft, iq_l, out, adc, n_bins, bin_clocks=bin_clocks, by_slot=by_slot, traces=traces)
    assert emu.last_kernel() == 'feedline_trace_kernel'
    torch.cuda.synchronize()
    assert traces is None or got is traces
    S = cfg.meas_cap if by_slot else 1
    assert got.dtype == torch.int64 and tuple(got.shape) == (S, cfg.cores_per_shot, 2, n_bins, _abi.TRACE_WORDS)
    return got.cpu().numpy()


def ref_traces(cfg, pt, lines, host, adc, n_bins, bin_clocks, by_slot):
    return traces_ref.feedline_traces(cfg, pt.cols, lines, host['summary'], host['events'], adc, host['iq_l'],
                                      cfg.meas_cap, n_bins, bin_clocks, by_slot=by_slot)


@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR], ids=['core_major', 'shot_major'])
@pytest.mark.parametrize('spc', [(16, 4), (1, 1)], ids=['16_4', '1_1'])
def test_bit_exact_against_reference(emu, spc, lane_order):
    """test_gpu_feedline's exact_case (4 cores in 3 groups, staggered strobes, five readouts against meas_cap 4, a
    window clipped by n_samples, at 1:1 window starts that are no multiple of 4), lines of 3 + 1 members, the
    resonator stage's noisy trace; bin_clocks 1 and 3, both class layouts, 250 bins: the 800-clock windows drop
    samples, the 4- and 28-clock windows end before the last bin.  Once into a caller's tensor full of garbage"""
    import torch
    ps, cfg = exact_case(spc, lane_order, 7200 + 16 * spc[0] + spc[1])
    who = [(1000 + s_, c) for s_ in range(3) for c in range(4)]
    params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}
    lines = T.exact_lines(3)
    d, host = pipeline(emu, ps, cfg, 3, 1000, who, params, N_CLKS, lines)
    pt, ft = d['pt'], d['ft']
    tab = random_table(pt, 87 + spc[0])
    adc = emu.feedline_adc(cfg, ft, d['iq_d'], d['out'], d['iq_l'].shape[1], resonators=tab)
    torch.cuda.synchronize()
    adc_h = adc.cpu().numpy().view(np.uint32)
    for bin_clocks in (1, 3):
        for by_slot in (False, True):
            mine = None
            if bin_clocks == 3 and by_slot:
                mine = torch.full((MEAS_CAP, 4, 2, T.EXACT_BINS, 4), GARBAGE, dtype=torch.int64, device=adc.device)
            got = gpu_traces(emu, cfg, ft, d['iq_l'], d['out'], adc, T.EXACT_BINS, bin_clocks, by_slot, traces=mine)
            want = ref_traces(cfg, pt, lines, host, adc_h, T.EXACT_BINS, bin_clocks, by_slot)
            np.testing.assert_array_equal(got, want, err_msg='bin_clocks {} by_slot {}'.format(bin_clocks, by_slot))
            if not by_slot:                                  # the inputs reach what tests/test_traces.py says
                reached = T.coverage(cfg, pt.cols, host['summary'], host['events'], host['iq_l'].shape[1], T.EXACT_BINS,
                                     bin_clocks, want)
                assert {'samples dropped', 'window ends before the last bin', 'clipped by n_samples_lo',
                        'more readouts than meas_cap', 'both states in every reading core'} <= reached
                assert spc[1] != 1 or 'unaligned window start' in reached
            else:
                assert want[3].any() and not (want == GARBAGE).any()


@pytest.mark.parametrize('name', T.HB_TRACE_CASES)
def test_bit_exact_on_handbuilt_inputs(emu, name):
    """tests/handbuilt.py's inputs: the readout scan's 32 slots and a pair without readouts, full-range words (the
    product P_I = 2^31 on a caller's trace), the 32,768-sample window in bins of 8 clocks, rows of four samples"""
    c, adc, n_bins, bin_clocks = T.hb_trace_inputs(name)
    out = {'summary': dev(c.summary), 'events': dev(c.events)}
    iq_l, adc_d = dev(c.iq_lo), dev(adc)
    for by_slot in (False, True):
        got = gpu_traces(emu, c.cfg, c.ft, iq_l, out, adc_d, n_bins, bin_clocks, by_slot)
        np.testing.assert_array_equal(got, T.hb_trace_reference(name, by_slot), err_msg='by_slot {}'.format(by_slot))


@pytest.mark.parametrize('name', list(hb.MANY))
def test_many_pairs_restage_the_window_table(emu, name):
    """tests/handbuilt.py's many_pairs cases at meas_cap 32 and 17: a chunk of 64 pairs of the 72-pair core is staged
    in runs of 32 (60) pairs, so the loop over the runs goes round twice and the second run's windows are summed from
    a rewritten table (asserted on the CPU: test_handbuilt_inputs.test_many_pairs_case_crosses_a_staging_run).  Both
    layouts (by slot: 32 or 17 grid layers over 142 pairs), bins of 1 clock and bins of 5 clocks that several threads
    add to and that end before the windows do; once into a caller's tensor full of garbage"""
    import torch
    c, adc, n_bins, bin_clocks = T.hb_trace_inputs(name)
    assert (n_bins, bin_clocks) == (300, 1)
    out = {'summary': dev(c.summary), 'events': dev(c.events)}
    iq_l, adc_d = dev(c.iq_lo), dev(adc)
    for by_slot in (False, True):
        got = gpu_traces(emu, c.cfg, c.ft, iq_l, out, adc_d, n_bins, bin_clocks, by_slot)
        np.testing.assert_array_equal(got, T.hb_trace_reference(name, by_slot), err_msg='by_slot {}'.format(by_slot))
        mine = None
        if by_slot:
            mine = torch.full((c.cfg.meas_cap, 4, 2, 2, 4), GARBAGE, dtype=torch.int64, device=adc_d.device)
        got = gpu_traces(emu, c.cfg, c.ft, iq_l, out, adc_d, 2, 5, by_slot, traces=mine)
        want = traces_ref.feedline_traces(c.cfg, c.pt.cols, c.lines, c.summary, c.events, adc, c.iq_lo, c.cfg.meas_cap, 2, 5,
                                          by_slot=by_slot)
        np.testing.assert_array_equal(got, want, err_msg='bin_clocks 5 by_slot {}'.format(by_slot))
        assert want[-1, 2, :, 1, 1].all() and not (want == GARBAGE).any()


def test_more_pairs_than_a_chunk(emu):
    """70 shots x 4 cores at 1:1, the pair order shuffled so that cores interleave: every core has 70 pairs, more
    than the 64 of one workgroup's chunk, and the sorted table's chunk boundaries fall between cores"""
    ps, cfg = exact_case((1, 1), _abi.LANES_SHOT_MAJOR, 7400)
    n = 70
    who = [(1000 + s_, c) for s_ in range(n) for c in range(4)]
    random.Random(3).shuffle(who)
    at = {w: i for i, w in enumerate(who)}
    lines = [ln for s_ in range(n) for ln in ([at[(1000 + s_, 2)], at[(1000 + s_, 0)], at[(1000 + s_, 1)]],
                                               [at[(1000 + s_, 3)]])]
    d, host = pipeline(emu, ps, cfg, n, 1000, who, {RDRV: (1, 1), RDLO: (1, 1)}, N_CLKS, lines)
    pt = d['pt']
    cores = pt.cols['core'].tolist()
    assert all(cores.count(c) == 70 for c in range(4)) and cores[:8] != sorted(cores[:8])
    for bin_clocks, by_slot in ((1, False), (3, True)):
        got = gpu_traces(emu, cfg, d['ft'], d['iq_l'], d['out'], d['adc'], 200, bin_clocks, by_slot)
        np.testing.assert_array_equal(got, ref_traces(cfg, pt, lines, host, host['adc'], 200, bin_clocks, by_slot))
    assert got[..., 0].max() > 30                            # tens of readouts in one class and bin


@pytest.mark.parametrize('spc', [(16, 4), (1, 1)], ids=['16_4', '1_1'])
def test_sum_identity_with_the_demodulator(emu, spc):
    """one pair alone on a line, ro_sigma 0, the bins covering the window: the sum of (w2, w3) over the bins is the S
    of feedline_demod_kernel, whose acc is sat((S + 2^(h-1)) >> h) bit for bit"""
    env = np.full(4 * 70, SQUARE, np.uint32)
    reads = [[dict(A=30000 + 9000 * c + 1000 * k, ph_d=9000 * k + c, ph_lo=555 * c, L_d=L, L_lo=L, lo_at=21 + c,
                   gap=400) for k, L in enumerate((1, 7, 60))] for c in range(2)]
    f_d, f_lo = [0x1234567, 0x7654321], [0x1234560, 0x7654300]
    prog = {c: assembled(ro_program(reads[c]), env, env, freq_buffer(f_d[c], spc[0]), freq_buffer(f_lo[c], spc[1]))
            for c in range(2)}
    cfg = _abi.make_config(2, max_cycles=1 << 22, event_cap=16, meas_cap=MEAS_CAP, meas_latency=32, p1=0.5,
                           demod=dict(drv_elem=RDRV, cpw=4, delay=20, theta=(0.3, 2.0), gain=(0.9, 0.7), sigma=0.0))
    who = [(5, 0), (5, 1)]
    params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}
    d, host = pipeline(emu, ProgramSet([prog], cores_per_shot=2), cfg, 1, 5, who, params, 1100, [[0], [1]])
    assert (host['res'][:, 0] == 3).all() and np.abs(host['acc'][2].astype(np.int64)).max() > 10 ** 5
    for bin_clocks, n_bins in ((1, 240), (7, 35)):
        got = gpu_traces(emu, cfg, d['ft'], d['iq_l'], d['out'], d['adc'], n_bins, bin_clocks, True)
        assert T.check_sum_identity(cfg, d['pt'].cols, got, host['acc'], host['res'], bin_clocks) == 6


def test_matched_filter_loop(emu):
    """tests/test_traces.py's loop end to end on the GPU at its shot count: traces with a square LO ->
    matched_filter per core -> the programs reassembled with those rdlo envelopes -> run, DDS ->
    demodulate_feedline on the same ADC traces -> iq_stats -> fit.  Traces, both accumulator buffers and every
    statistics table equal the references bit for bit; the physical assertions are check_loop's, with its
    tolerances"""
    import torch
    seed, n, shot0 = T.MF_SEEDS[1], T.MF_SHOTS, 500
    cfg, progs, f, env, n_clks = T.mf_case(seed)
    who = [(shot0 + s_, c) for s_ in range(n) for c in range(4)]
    params = {RDRV: (4, 4), RDLO: (4, 4)}

    def program_set(envs):
        return ProgramSet([{c: assembled(progs[c], env, envs[c], freq_buffer(f[c], 4), freq_buffer(f[c], 4))
                            for c in range(4)}], cores_per_shot=4)
    d, host = pipeline(emu, program_set([env] * 4), cfg, n, shot0, who, params, n_clks)
    pt = d['pt']
    lines = dispersive_lines(pt.cols)
    from distributed_processor_amd.dds import FeedlineTable
    ft = FeedlineTable(pt, lines)
    tab = ResonatorTable(pt, dispersive_f_res(pt.cols['core']), KAPPA, adc_sigma=T.MF_ADC_SIGMA / 65536.0)
    adc = emu.feedline_adc(cfg, ft, d['iq_d'], d['out'], d['iq_l'].shape[1], resonators=tab)
    n_bins = 4 * T.MF_LO_WORDS
    tr = gpu_traces(emu, cfg, ft, d['iq_l'], d['out'], adc, n_bins, 1, False)
    adc_h = adc.cpu().numpy().view(np.uint32)
    np.testing.assert_array_equal(adc_h, resonator_ref.feedline_adc_res(
        cfg, pt.cols, lines, tab.coef, tab.adc_sigma, host['summary'], host['events'], host['iq_d'],
        host['iq_l'].shape[1], cfg.meas_cap))
    np.testing.assert_array_equal(tr, ref_traces(cfg, pt, lines, host, adc_h, n_bins, 1, False))
    rt = ReadoutTraces(tr, cfg)

    def measured(iq_l, iq_l_host):
        acc, res = emu.demodulate_feedline(cfg, ft, iq_l, d['out'], adc=adc)
        torch.cuda.synchronize()
        acc_h, res_h = acc.cpu().numpy(), res.cpu().numpy().view(np.uint32)
        want = feedline_ref.demod_feedline(cfg, pt.cols, lines, host['summary'], host['events'], adc_h, iq_l_host,
                                           cfg.meas_cap)
        np.testing.assert_array_equal(acc_h, want[0])
        np.testing.assert_array_equal(res_h, want[1])

        def iq_stats(axis, thr):
            stats, _ = emu.iq_stats(cfg, acc, res, pairs=pt, axis=axis, thr=thr)
            torch.cuda.synchronize()
            t = stats.cpu().numpy()
            np.testing.assert_array_equal(t, iq_stats_ref.iq_stats(cfg, acc_h, res_h[:, 0], core=pt.cols['core'],
                                                                   shot=pt.cols['shot'], axis=axis, thr=thr)[0])
            return t
        return T.fitted_stats(cfg, pt.cols, acc_h, res_h, iq_stats=iq_stats)
    before = measured(d['iq_l'], host['iq_l'])
    envs = [T.mf_envelope(rt.matched_filter(c)) for c in range(3)] + [env]
    d2, host2 = pipeline(emu, program_set(envs), cfg, n, shot0, who, params, n_clks)
    np.testing.assert_array_equal(host2['summary'], host['summary'])       # the envelope changes no event
    counted = np.arange(cfg.event_cap)[:, None] < host['summary'].view(np.uint32)[None, :, 2]
    np.testing.assert_array_equal(host2['events'][counted], host['events'][counted])
    assert (host2['iq_l'] != host['iq_l']).any() and np.array_equal(host2['iq_d'], host['iq_d'])
    after = measured(d2['iq_l'], host2['iq_l'])
    gains = [rt.predicted_gain(c) for c in range(3)]
    worst_axis, worst_ratio = T.check_loop(before, after, gains)
    print('snr {} -> {}, predicted gains {}, fidelity {:.4f} -> {:.4f}, axis {:.2e} rad, ratio dev {:.3e}'.format(
        np.round(before[0][:3], 3), np.round(after[0][:3], 3), np.round(gains, 3), before[2], after[2], worst_axis,
        worst_ratio))
    assert worst_axis <= T.AXIS_TOL and worst_ratio <= T.GAIN_TOL


def test_timing_records_the_main_kernel(emu):
    c, adc, n_bins, bin_clocks = T.hb_trace_inputs('edge_four_samples')
    out = {'summary': dev(c.summary), 'events': dev(c.events)}
    iq_l, adc_d = dev(c.iq_lo), dev(adc)
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        gpu_traces(emu, c.cfg, c.ft, iq_l, out, adc_d, n_bins, bin_clocks, False)
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 1 and 0 < ms[0] < 100 and emu.last_kernel() == 'feedline_trace_kernel'


def test_refusals_at_the_c_abi(emu):
    """every DPEMU_E_INVALID condition, before any launch: -22 and a message that names the field; traces stays
    as preset"""
    import torch
    cfg = _abi.make_config(2, event_cap=16, meas_cap=4, demod=dict(drv_elem=RDRV))
    device = torch.device('cuda', 0)

    def z(*shape):
        return torch.zeros(shape, dtype=torch.int32, device=device)
    summ, ev, iq_l, adc = z(4, 8), z(16, 4, 4), z(3, 16), z(2, 16)
    traces = torch.full((4, 2, 2, 8, 4), 7, dtype=torch.int64, device=device)
    ptr = {k: v.data_ptr() for k, v in dict(summary=summ, events=ev, iq_lo=iq_l, adc=adc, traces=traces).items()}

    def call(lines=((0, 1), (2,)), n_lines=None, first=None, meas_cap=4, event_cap=16, n_lo=16, cfg_=cfg, n_pairs=3,
             no_pairs=False, no_lines=False, no_bins=False, n_bins=8, bin_clocks=1, by_slot=1, **kw):
        a = dict(lane=[0, 3, 1], core=[0, 1, 1], drv_row=[0, 1, 2], lo_row=[0, 1, 2], spc_drv=[16, 16, 16],
                 spc_lo=[4, 4, 4])
        a.update({k: v for k, v in kw.items() if k in a})
        p = dict(ptr)
        p.update({k: v for k, v in kw.items() if k in p})
        arr = {k: np.array(v, np.uint32) for k, v in a.items()}
        arr['shot'] = np.array([5, 6, 6], np.uint64)
        st = _abi.DemodPairs(n_pairs, 4, event_cap, meas_cap, 64, n_lo)
        for k, v in arr.items():
            setattr(st, k, v.ctypes.data)
        lf = np.array(first if first is not None else np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]),
                      np.uint32)
        mem = np.array([m for ln in lines for m in ln] or [0], np.uint32)
        ls = _abi.Feedlines(len(lines) if n_lines is None else n_lines, lf.ctypes.data, mem.ctypes.data)
        tb = _abi.TraceBins(n_bins, bin_clocks, by_slot)
        rc = emu._L.dpemu_feedline_traces(emu._h, C.addressof(cfg_) if cfg_ is not None else None,
                                          None if no_pairs else C.addressof(st), None if no_lines else C.addressof(ls),
                                          None if no_bins else C.addressof(tb), p['summary'], p['events'], p['adc'],
                                          p['iq_lo'], p['traces'], None)
        return rc, emu._L.dpemu_last_error(emu._h)

    assert call()[0] == 0 and emu.last_kernel() == 'feedline_trace_kernel'
    torch.cuda.synchronize()
    assert not traces.any().item()                            # assigned: the events hold no readout
    traces.fill_(7)
    cases = ((dict(cfg_=None), b'cfg'), (dict(no_pairs=True), b'pairs'), (dict(no_lines=True), b'lines'),
             (dict(no_bins=True), b'bins'), (dict(summary=None), b'summary'), (dict(events=None), b'events'),
             (dict(adc=None), b'adc'), (dict(iq_lo=None), b'iq_lo'), (dict(traces=None), b'traces'),
             # everything dpemu_demod_feedline refuses
             (dict(n_lines=0), b'n_lines'), (dict(lines=((0, 1), ()), first=[0, 2, 2]), b'empty'),
             (dict(lines=(tuple([0] * 17),)), b'17 members'), (dict(lines=((0, 3), (1, 2))), b'member 3'),
             (dict(lines=((0, 1), (1, 2))), b'two lines'), (dict(spc_drv=[16, 8, 16]), b'spc_drv'),
             (dict(spc_drv=[4, 2, 4], spc_lo=[4, 2, 4]), b'spc_'), (dict(n_lo=0), b'n_samples_lo'),
             (dict(n_lo=18), b'n_samples_lo'), (dict(adc=ptr['adc'] + 4), b'adc must be 16-byte aligned'),
             (dict(iq_lo=ptr['iq_lo'] + 8), b'iq_lo must be 16-byte aligned'), (dict(event_cap=1025), b'event_cap'),
             (dict(meas_cap=0), b'meas_cap'), (dict(meas_cap=33), b'meas_cap'), (dict(lane=[0, 4, 1]), b'lane'),
             (dict(core=[0, 2, 1]), b'core'), (dict(first=[1, 2, 3]), b'line_first'),
             (dict(lines=((0, 1),)), b'pair 2 is in no line'),
             # the stage's own
             (dict(n_bins=0), b'n_bins'), (dict(n_bins=4097), b'n_bins'), (dict(bin_clocks=0), b'bin_clocks'),
             (dict(by_slot=2), b'by_slot'), (dict(traces=ptr['traces'] + 4), b'traces must be 8-byte aligned'),
             (dict(bin_clocks=2 ** 31 // (3 * 4 * 16) + 1), b'bin_clocks'),
             (dict(bin_clocks=0xFFFFFFFF, n_pairs=65535, meas_cap=32), b'bin_clocks'))
    for kw, field in cases:
        rc, msg = call(**kw)
        assert rc == -22 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert (traces == 7).all().item()                         # nothing was launched
    assert call(bin_clocks=2 ** 31 // (3 * 4 * 16), by_slot=0)[0] == 0               # the bound itself is accepted
    torch.cuda.synchronize()
    assert (traces[1:] == 7).all().item() and not traces[0].any().item()             # by_slot 0 assigns layer 0 alone
