"""The cached device tables of the readout entry points (csrc/capi.cpp
DevTable: pair, line and resonator tables are uploaded only when their bytes
change) through the real calls on one Emulator: a table of the same size with
other content, a smaller table, then the first again.  4 pairs x 2 readouts x
256 LO samples; every result bit for bit against the numpy restatements."""

import copy
import random

import numpy as np
import pytest

from distributed_processor_amd import _abi
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable, FeedlineTable
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from tests import demod_iq_ref, feedline_ref, resonator_ref
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import freq_buffer
from tests.test_gpu_demod_iq import assembled
from tests.test_gpu_resonator import random_table

pytestmark = pytest.mark.gpu

N_LO = 256
MEAS_CAP = 4
ORDER = ('A', 'B', 'A', 'S', 'A')       # same size with other content, back, shrink, grow


@pytest.fixture(scope='module')
def case():
    """2 shots x 2 cores at 1:1, two readouts each (windows of 1 and 7 words), run and
    synthesised once; the pair tables A (rows i with i), B (A with the rows of pairs 1 and 2
    swapped: the same size, other content) and S (pairs 2 and 3 alone)"""
    import torch
    rng = random.Random(99)
    env = [np.array([((rng.randint(-30000, 30000) & 0xFFFF) << 16) | (rng.randint(-30000, 30000) & 0xFFFF)
                     for _ in range(64)], np.uint32) for _ in range(2)]
    prog = {}
    for c in range(2):
        f_d = rng.getrandbits(32)
        reads = [dict(A=rng.randint(30000, 65535), ph_d=rng.getrandbits(17), ph_lo=rng.getrandbits(17), L_d=L, L_lo=L,
                      lo_at=20 + 3 * c, gap=60) for L in (1, 7)]
        prog[c] = assembled(ro_program(reads), env[0], env[1], freq_buffer(f_d, 1),
                            freq_buffer((f_d - 17 * c) & 0xFFFFFFFF, 1))
    ps = ProgramSet([prog], cores_per_shot=2)
    cfg = _abi.make_config(2, max_cycles=1 << 20, event_cap=16, meas_cap=MEAS_CAP, meas_latency=32, seed=99,
                           p1=[0.3, 0.6], demod=dict(drv_elem=RDRV, cpw=4, delay=20, theta=(0.7, -2.1), gain=(0.9, 0.6),
                                                     axis=[0.3, -1.2], sigma=40.0, thr=-20000))
    who = [(1000 + s_, c) for s_ in range(2) for c in range(2)]
    emu = Emulator(0)
    emu.load(ps)
    out = alloc_device_outputs(cfg, 2, want=('summary', 'events'))
    emu.run_device(cfg, 2, 1000, out)
    drv = ChannelPlan(ps, cfg, 1000, 2, [(s_, c, RDRV) for s_, c in who], {RDRV: (1, 1), RDLO: (1, 1)})
    lo = ChannelPlan(ps, cfg, 1000, 2, [(s_, c, RDLO) for s_, c in who], {RDRV: (1, 1), RDLO: (1, 1)})
    iq_d, iq_l = emu.synthesize(drv, out, N_LO), emu.synthesize(lo, out, N_LO)
    torch.cuda.synchronize()
    a = DemodPairTable(cfg, drv, lo)
    b = copy.copy(a)
    b.cols = {k: v.copy() for k, v in a.cols.items()}
    for col in ('drv_row', 'lo_row'):   # (the ADC stages read the drive rows, the demodulator the LO rows)
        b.cols[col][[1, 2]] = a.cols[col][[2, 1]]
    tables = {'A': a, 'B': b, 'S': DemodPairTable(cfg, drv, lo, drv_rows=[2, 3], lo_rows=[2, 3])}
    host = dict(summary=out['summary'].cpu().numpy(), events=out['events'].cpu().numpy(), iq_d=iq_d.cpu().numpy(),
                iq_l=iq_l.cpu().numpy())
    assert host['iq_d'].any() and host['iq_l'].any()
    yield emu, cfg, out, iq_d, iq_l, tables, host
    emu.close()


def test_pair_table_alternation(case):
    import torch
    emu, cfg, out, iq_d, iq_l, tables, host = case
    want = {k: demod_iq_ref.demod_iq(cfg, pt.cols, host['summary'], host['events'], host['iq_d'], host['iq_l'], MEAS_CAP)
            for k, pt in tables.items()}
    assert want['A'][1][:, 0].tolist() == [2, 2, 2, 2]                                  # two readouts per pair
    assert not np.array_equal(want['A'][0], want['B'][0])                              # B is another table
    for step, k in enumerate(ORDER):
        acc, res = emu.demodulate(cfg, None, iq_d, None, iq_l, out, pairs=tables[k])
        torch.cuda.synchronize()
        np.testing.assert_array_equal(acc.cpu().numpy(), want[k][0], err_msg='step {} table {}'.format(step, k))
        np.testing.assert_array_equal(res.cpu().numpy().view(np.uint32), want[k][1],
                                      err_msg='step {} table {}'.format(step, k))


def test_line_and_resonator_table_alternation(case):
    """feedline_adc, then feedline_adc_res on the same lines (one line table for both stages), per pair table"""
    import torch
    emu, cfg, out, iq_d, iq_l, tables, host = case
    lines = {'A': [[0, 1], [2, 3]], 'B': [[0, 1], [2, 3]], 'S': [[1, 0]]}
    ft = {k: FeedlineTable(tables[k], lines[k]) for k in tables}
    rt = {k: random_table(tables[k], 300 + i) for i, k in enumerate(sorted(tables))}
    args = (host['summary'], host['events'], host['iq_d'], N_LO, MEAS_CAP)
    want = {k: (feedline_ref.feedline_adc(cfg, tables[k].cols, lines[k], *args),
                resonator_ref.feedline_adc_res(cfg, tables[k].cols, lines[k], rt[k].coef, rt[k].adc_sigma, *args))
            for k in tables}
    assert not np.array_equal(want['A'][0], want['B'][0]) and not np.array_equal(want['A'][1], want['B'][1])
    for step, k in enumerate(ORDER):
        adc = emu.feedline_adc(cfg, ft[k], iq_d, out, N_LO)
        assert emu.last_kernel() == 'feedline_adc_kernel'
        adc_res = emu.feedline_adc(cfg, ft[k], iq_d, out, N_LO, resonators=rt[k])
        assert emu.last_kernel() == 'feedline_res_kernel'
        torch.cuda.synchronize()
        np.testing.assert_array_equal(adc.cpu().numpy().view(np.uint32), want[k][0],
                                      err_msg='step {} table {}: feedline_adc'.format(step, k))
        np.testing.assert_array_equal(adc_res.cpu().numpy().view(np.uint32), want[k][1],
                                      err_msg='step {} table {}: feedline_adc_res'.format(step, k))
