"""The five readout kernels (demod_iq_kernel, feedline_index_kernel,
feedline_adc_kernel, feedline_res_kernel, feedline_demod_kernel) on hand-built
events, pair tables and iq rows (tests/handbuilt.py), bit for bit against
tests/demod_iq_ref.py, tests/feedline_ref.py and tests/resonator_ref.py.

The pipeline tests (test_gpu_demod_iq, test_gpu_feedline, test_gpu_resonator)
feed these kernels what dpemu_run and dpemu_dds produce: 16 event records, at
most 5 readouts, waveforms that never saturate.  The inputs here reach the
readout scan past its first chunk and its 32 slots, full-range int16 words
(-32768 in a caller's ADC trace and LO row included), the int32 clamp of the
scaled sum and the wrap of the accumulator, and the ends of every buffer.
The many_pairs cases bring 142 pairs at 32 (and 17) slots to all of them, and
every case carries per-lane state words for the *_st entry points.  That each
input set reaches what it is for is asserted on the CPU, from the references
alone, in tests/test_handbuilt_inputs.py.

lane_order: the pair columns are given by hand and a pair names its lane, so
neither the tables nor the kernels depend on cfg.lane_order; one value is run."""

import numpy as np
import pytest

from tests import handbuilt as hb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def emu():
    from distributed_processor_amd.emulator import Emulator
    e = Emulator(0)
    yield e
    e.close()


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order='C').view(np.int32)).cuda()      # (a copy: the references are read-only)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def check_demod(got, want, what):
    acc, res = got
    np.testing.assert_array_equal(u32(res), want[1], err_msg=what + ': result')
    np.testing.assert_array_equal(acc.cpu().numpy(), want[0], err_msg=what + ': acc')


@pytest.mark.parametrize('name', list(hb.CASES))
def test_bit_exact_on_handbuilt_inputs(emu, name):
    """all four entry points on one input set: demodulate(pairs=), feedline_adc, feedline_adc(resonators=) and
    demodulate_feedline(adc=) on the plain trace, the resonator trace and -- where the case has one -- the
    caller-made trace"""
    import torch
    c, ref = hb.case(name), hb.reference(name)
    cfg = c.cfg
    out = {'summary': dev(c.summary), 'events': dev(c.events)}
    iq_d, iq_l = dev(c.iq_drv), dev(c.iq_lo)

    got = emu.demodulate(cfg, None, iq_d, None, iq_l, out, pairs=c.pt)
    assert emu.last_kernel() == 'demod_iq_kernel'
    check_demod(got, (ref['acc_iq'], ref['res_iq']), 'demodulate')

    adc = emu.feedline_adc(cfg, c.ft, iq_d, out, c.n_lo)
    assert emu.last_kernel() == 'feedline_adc_kernel'
    np.testing.assert_array_equal(u32(adc), ref['adc'], err_msg='feedline_adc')

    adc_res = emu.feedline_adc(cfg, c.ft, iq_d, out, c.n_lo, resonators=c.resonators())
    assert emu.last_kernel() == 'feedline_res_kernel'
    np.testing.assert_array_equal(u32(adc_res), ref['adc_res'], err_msg='feedline_adc(resonators=)')

    # the demodulator on the references' traces (its input does not depend on the two kernels above)
    for key, trace in (('fl', ref['adc']), ('fl_res', ref['adc_res']), ('fl_in', c.adc_in)):
        if trace is None:
            continue
        got = emu.demodulate_feedline(cfg, c.ft, iq_l, out, adc=dev(trace))
        assert emu.last_kernel() == 'feedline_demod_kernel'
        check_demod(got, ref[key], 'demodulate_feedline(adc=' + key + ')')
    torch.cuda.synchronize()


@pytest.mark.parametrize('name', list(hb.CASES))
def test_supplied_states_on_handbuilt_inputs(emu, name):
    """the *_st entry points on hb.states(name): full-range words, bits at and above a lane's readout count set (the
    references read none of them: tests/test_handbuilt_inputs.py), against tests/qsim_meas_ref.py's injected
    references -- feedline_adc, feedline_adc(resonators=), feedline_traces in both layouts on the trace
    test_gpu_traces uses, and iq_stats by slot on the demodulator's reference accumulators"""
    import torch
    from tests import test_traces as T
    c, ref, want = hb.case(name), hb.reference(name), hb.reference_st(name)
    cfg = c.cfg
    out = {'summary': dev(c.summary), 'events': dev(c.events)}
    iq_d, iq_l, states = dev(c.iq_drv), dev(c.iq_lo), dev(hb.states(name))

    adc = emu.feedline_adc(cfg, c.ft, iq_d, out, c.n_lo, states=states)
    assert emu.last_kernel() == 'feedline_adc_kernel'
    np.testing.assert_array_equal(u32(adc), want['adc'], err_msg='feedline_adc(states=)')

    adc_res = emu.feedline_adc(cfg, c.ft, iq_d, out, c.n_lo, resonators=c.resonators(), states=states)
    assert emu.last_kernel() == 'feedline_res_kernel'
    np.testing.assert_array_equal(u32(adc_res), want['adc_res'], err_msg='feedline_adc(resonators=, states=)')

    _, trace, n_bins, bin_clocks = T.hb_trace_inputs(name)
    trace_d = dev(trace)
    for by_slot in (False, True):
        got = emu.feedline_traces(cfg, c.ft, iq_l, out, trace_d, n_bins, bin_clocks=bin_clocks, by_slot=by_slot,
                                  states=states)
        assert emu.last_kernel() == 'feedline_trace_kernel'
        np.testing.assert_array_equal(got.cpu().numpy(), want['traces', by_slot],
                                      err_msg='feedline_traces(states=, by_slot={})'.format(by_slot))

    acc, res = ref['fl']
    stats, bits = emu.iq_stats(cfg, torch.from_numpy(np.array(acc)).cuda(), dev(res), pairs=c.pt, states=states,
                               by_slot=True, bits=True)
    assert emu.last_kernel() == 'iq_stats_kernel'
    np.testing.assert_array_equal(u32(bits), want['bits'], err_msg='iq_stats(states=): bits')
    np.testing.assert_array_equal(stats.cpu().numpy(), want['stats'], err_msg='iq_stats(states=): stats')
    torch.cuda.synchronize()
