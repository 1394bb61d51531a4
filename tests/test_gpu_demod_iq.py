"""dpemu_demod_iq (csrc/demod_iq.hip) on the GPU: run_device -> synthesize (the
GPU DDS) -> demodulate, bit for bit against the numpy restatement
(tests/demod_iq_ref.py) on the same GPU event and iq arrays; the outcome bits
against the interpreter's DEMOD model on config 3; the flat-top agreement and
the envelope weighting of tests/test_demod_iq.py on the GPU's own outputs; and
the argument checks of the C ABI."""

import ctypes as C
import math
import random

import numpy as np
import pytest

from distributed_processor_amd import _abi, isa, workloads
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from distributed_processor_amd.hwconfig import DDSElementConfig
from tests import demod_iq_ref
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, flat_tolerance, freq_buffer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def assembled(words, env_d, env_lo, fb_d, fb_lo):
    """one core's program with its rdrv / rdlo buffers, as the assembler hands them over"""
    z = np.zeros(0, np.uint32)
    return {'cmd_buf': isa.words_to_bytes(words),
            'env_buffers': [z.tobytes(), np.asarray(env_d, np.uint32).tobytes(), np.asarray(env_lo, np.uint32).tobytes()],
            'freq_buffers': [z.tobytes(), np.asarray(fb_d, np.uint32).tobytes(), np.asarray(fb_lo, np.uint32).tobytes()]}


def pipeline(emu, ps, cfg, n_shots, shot0, who, params, n_clks, want=('summary', 'events')):
    """run, synthesise the drive and LO channels of the (shot, core) list `who`
    (two dpemu_dds calls: the rates differ, so do the row lengths), demodulate.
    Returns host copies: outputs, pair table, iq_drv, iq_lo, acc, result."""
    import torch
    emu.load(ps)
    out = alloc_device_outputs(cfg, n_shots, want=want)
    emu.run_device(cfg, n_shots, shot0, out)
    drv = ChannelPlan(ps, cfg, shot0, n_shots, [(s_, c, RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, shot0, n_shots, [(s_, c, RDLO) for s_, c in who], params)
    iq_d = emu.synthesize(drv, out, n_clks * params[RDRV][0])
    iq_l = emu.synthesize(lo, out, n_clks * params[RDLO][0])
    acc, res = emu.demodulate(cfg, drv, iq_d, lo, iq_l, out)
    assert emu.last_kernel() == 'demod_iq_kernel'
    torch.cuda.synchronize()
    host = {k: v.cpu().numpy() for k, v in out.items()}
    return (host, DemodPairTable(cfg, drv, lo), iq_d.cpu().numpy(), iq_l.cpu().numpy(), acc.cpu().numpy(),
            res.cpu().numpy().view(np.uint32))


N_CLKS = 4800


def exact_case(spc, lane_order, seed):
    """2 cores x 3 shots in 3 groups: windows of 1, 7 and 1000 words (16, 112
    and 16,000 LO samples at 4 per clock); group 1's core 1 has no drive pulse;
    group 2's core 0 has 5 reads (meas_cap 4), its third window clipped by
    n_samples and its fourth clipped to nothing; three detunings (the LO's
    freq entries); random 17-bit phases, thetas, gains, axes; noise on."""
    rng = random.Random(seed)
    env = [np.array([((rng.randint(-30000, 30000) & 0xFFFF) << 16) | (rng.randint(-30000, 30000) & 0xFFFF)
                     for _ in range(4000)], np.uint32) for _ in range(2)]
    groups = []
    for g in range(3):
        prog = {}
        for c in range(2):
            f_d = rng.getrandbits(32)
            dets = (0, rng.randint(-40, 40), rng.randint(-2 ** 26, 2 ** 26))
            fb_lo = np.concatenate([freq_buffer((f_d - d) & 0xFFFFFFFF, spc[1]) for d in dets])

            def read(L, k, lo_at, gap):
                return dict(A=rng.randint(1000, 65535), ph_d=rng.getrandbits(17), ph_lo=rng.getrandbits(17),
                            L_d=L, L_lo=L, fi_lo=k % 3, lo_at=lo_at, gap=gap)
            if g == 2 and c == 0:
                reads = [read(1, 0, 140, 300), read(7, 1, 150, 300), read(1000, 2, 300, 4400), read(1, 0, 140, 300),
                         read(7, 1, 140, 300)]
            else:
                reads = [read(1, 0, 140, 300), read(7, 1, 133, 300), read(1000, 2, 150, 300)]
            words = ro_program(reads)
            if g == 1 and c == 1:                     # the LO pulses alone
                words = [w for i, w in enumerate(words) if i == 0 or i % 2 == 0 or i == len(words) - 1]
            prog[c] = assembled(words, env[0], env[1], freq_buffer(f_d, spc[0]), fb_lo)
        groups.append(prog)
    ps = ProgramSet(groups, cores_per_shot=2)
    cfg = _abi.make_config(2, n_groups=3, max_cycles=1 << 20, event_cap=16, meas_cap=4, meas_latency=32, seed=seed,
                           p1=[0.3, 0.6], lane_order=lane_order,
                           demod=dict(drv_elem=RDRV, cpw=4, delay=140, theta=(rng.uniform(-4, 4), rng.uniform(-4, 4)),
                                      gain=(rng.random(), rng.random()), axis=[rng.uniform(-4, 4) for _ in range(2)],
                                      sigma=rng.uniform(5, 300), thr=rng.randint(-10 ** 6, 10 ** 6)))
    return ps, cfg


@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR], ids=['core_major', 'shot_major'])
@pytest.mark.parametrize('spc', [(16, 4), (4, 4), (2, 1), (1, 1)], ids=['16_4', '4_4', '2_1', '1_1'])
def test_bit_exact_against_reference(emu, spc, lane_order):
    ps, cfg = exact_case(spc, lane_order, 4200 + 16 * spc[0] + spc[1])
    who = [(1000 + s_, c) for s_ in range(3) for c in range(2)]
    params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}          # interp = spc: 4 clocks per env word
    out, pt, iq_d, iq_l, acc, res = pipeline(emu, ps, cfg, 3, 1000, who, params, N_CLKS)
    want_acc, want_res = demod_iq_ref.demod_iq(cfg, pt.cols, out['summary'], out['events'], iq_d, iq_l, 4)
    # the case holds what it claims: 3 reads everywhere, 4 of 5 kept on (shot 1001, core 0)
    counts = {w: int(want_res[i, 0]) for i, w in enumerate(who)}
    assert counts[(1001, 0)] == 4 and all(v == 3 for w, v in counts.items() if w != (1001, 0))
    assert not iq_d[who.index((1000, 1))].any() and iq_d[who.index((1000, 0))].any() and iq_l.any()
    np.testing.assert_array_equal(res, want_res)
    np.testing.assert_array_equal(acc, want_acc)
    assert np.abs(want_acc[2].astype(np.int64)).max() > 10 ** 6 and not np.delete(want_acc[3], 2, axis=0).any()


def test_one_plan_one_buffer(emu):
    """both channels of every pair in one plan and one iq buffer (demodulate_plan):
    the same bits as the reference on that buffer"""
    import torch
    ps, cfg = exact_case((4, 4), _abi.LANES_SHOT_MAJOR, 4300)
    emu.load(ps)
    out = alloc_device_outputs(cfg, 3, want=('summary', 'events'))
    emu.run_device(cfg, 3, 1000, out)
    chans = [(1000 + s_, c, e) for s_ in range(3) for c in range(2) for e in (RDLO, RDRV)]
    plan = ChannelPlan(ps, cfg, 1000, 3, chans, {RDRV: (4, 4), RDLO: (4, 4)})
    iq = emu.synthesize(plan, out, 4 * N_CLKS)
    acc, res = emu.demodulate_plan(cfg, plan, iq, out)
    torch.cuda.synchronize()
    pt = DemodPairTable.one_plan(cfg, plan)
    assert pt.n_pairs == 6 and pt.cols['lo_row'].tolist() == [0, 2, 4, 6, 8, 10]
    host_iq = iq.cpu().numpy()
    want_acc, want_res = demod_iq_ref.demod_iq(cfg, pt.cols, out['summary'].cpu().numpy(), out['events'].cpu().numpy(),
                                               host_iq, host_iq, 4)
    np.testing.assert_array_equal(res.cpu().numpy().view(np.uint32), want_res)
    np.testing.assert_array_equal(acc.cpu().numpy(), want_acc)
    assert want_res[:, 0].tolist() == [3, 3, 4, 3, 3, 3]


def test_outcomes_equal_the_interpreters(emu):
    """config 3 under the DEMOD model with square envelopes and no noise: the
    outcome bits of the demodulated waveforms equal the run's meas_bits for
    every readout of the sampled lanes (the Philox counter (global shot, core,
    m), the state's theta and gain, and the discriminator, against lane.h)"""
    ps = ProgramSet(workloads.config3_active_reset(8))
    for c in range(8):
        env = ps.buffers[(0, c)][0]
        env[RDRV] = np.full(len(env[RDRV]), SQUARE, np.uint32)
    cfg = _abi.make_config(8, n_groups=ps.n_groups, max_cycles=50000, event_cap=16, trace_cap=0, meas_cap=4,
                           meas_latency=workloads.CONFIG3_DEMOD_LATENCY, seed=0x5EED, p1=0.5,
                           demod=workloads.config3_demod(ps, sigma=0.0))
    shot0, n = 7000, 64
    who = [(shot0 + s_, c) for s_ in range(0, n, 9) for c in range(8)]
    params = {e: (d['samples_per_clk'], d['interp_ratio']) for e, d in enumerate(workloads.ELEMS)}
    out, pt, iq_d, iq_l, acc, res = pipeline(emu, ps, cfg, n, shot0, who, params, 3200,
                                             want=('summary', 'events', 'meas'))
    s = _abi.unpack_summary(out['summary'].view(np.uint32))
    assert int(s['t_end'].max()) < 3200 and (s['n_meas'] == 2).all()
    lanes = pt.cols['lane']
    np.testing.assert_array_equal(res[:, 0], s['n_meas'][lanes])
    np.testing.assert_array_equal(res[:, 1], s['meas_bits'][lanes] & 3)
    assert 0 < (res[:, 1] & 1).mean() < 1                         # both states occur
    assert np.abs(acc[:2].astype(np.int64)).max(axis=2).min() > 10 ** 7


def _shape_case(emu, env_d, state):
    """config 3's readout shape (16:4, 1000 clocks, delay 300) on the GPU:
    (closed-form acc of the DEMOD run, waveform acc)"""
    f = 0x1999999A
    reads = [dict(A=39321, ph_d=0, ph_lo=14597, L_d=250, L_lo=250, lo_at=300)]
    prog = assembled(ro_program(reads), env_d, np.full(1000, SQUARE, np.uint32), freq_buffer(f, 16),
                     freq_buffer(f, 4))
    ps = ProgramSet([{0: prog}], cores_per_shot=1)
    cfg = _abi.make_config(1, max_cycles=1 << 20, event_cap=16, meas_cap=4, meas_latency=32, p1=float(state),
                           demod=dict(drv_elem=RDRV, cpw=4, delay=300, theta=(math.pi, 0.0), sigma=0.0))
    out, pt, iq_d, iq_l, acc, res = pipeline(emu, ps, cfg, 1, 0, [(0, 0)], {RDRV: (16, 16), RDLO: (4, 4)}, 1400,
                                             want=('summary', 'events', 'acc'))
    assert int(res[0, 0]) == 1
    return out['acc'][0, 0].astype(np.int64), acc[0, 0].astype(np.int64)


def test_flat_top_and_envelope_weighting_on_gpu_outputs(emu):
    """tests/test_demod_iq.py's flat-top agreement and envelope weighting, one
    case each, on the GPU's DEMOD run, DDS and demodulation (same tolerance)"""
    cf, wave = _shape_case(emu, np.full(1000, SQUARE, np.uint32), 1)
    assert np.hypot(*cf.astype(float)) > 1.9e7
    assert np.abs(wave - cf).max() <= flat_tolerance(cf), (cf, wave)
    env = DDSElementConfig(**workloads.ELEMS[RDRV]).get_env_buffer(workloads.RDRV_ENV)
    mean = float(demod_iq_ref.s16(env >> 16).mean()) / 32767
    cf, wave = _shape_case(emu, env, 0)
    tol = flat_tolerance(cf)
    assert np.abs(wave - cf * mean).max() <= tol, (cf, wave, mean)
    assert np.abs(wave - cf).max() > 10 * tol


def test_refusals_at_the_c_abi(emu):
    """argument checks made before any launch: -22 and the field's name"""
    import torch
    cfg = _abi.make_config(2, event_cap=16, meas_cap=4, demod=dict(drv_elem=RDRV))
    dev = torch.device('cuda', 0)
    summ, ev = torch.zeros((4, 8), dtype=torch.int32, device=dev), torch.zeros((16, 4, 4), dtype=torch.int32, device=dev)
    iq_d, iq_l = torch.zeros((2, 64), dtype=torch.int32, device=dev), torch.zeros((2, 16), dtype=torch.int32, device=dev)
    acc, res = torch.zeros((4, 2, 2), dtype=torch.int32, device=dev), torch.zeros((2, 2), dtype=torch.int32, device=dev)

    def call(iq_lo=iq_l.data_ptr(), meas_cap=4, **cols):
        a = dict(lane=[0, 3], core=[0, 1], drv_row=[0, 1], lo_row=[0, 1], spc_drv=[16, 16], spc_lo=[4, 4])
        a.update(cols)
        arr = {k: np.array(v, np.uint32) for k, v in a.items()}
        arr['shot'] = np.array([5, 6], np.uint64)
        st = _abi.DemodPairs(2, 4, 16, meas_cap, 64, 16)
        for k, v in arr.items():
            setattr(st, k, v.ctypes.data)
        rc = emu._L.dpemu_demod_iq(emu._h, C.addressof(cfg), C.addressof(st), summ.data_ptr(), ev.data_ptr(),
                                   iq_d.data_ptr(), iq_lo, acc.data_ptr(), res.data_ptr(), None)
        return rc, emu._L.dpemu_last_error(emu._h)

    assert call()[0] == 0                                         # the baseline call is accepted
    for kw, field in ((dict(spc_drv=[16, 6]), b'spc_drv'), (dict(spc_drv=[3, 3], spc_lo=[3, 3]), b'spc_lo'),
                      (dict(lane=[0, 4]), b'lane'), (dict(iq_lo=None), b'iq_lo'), (dict(meas_cap=0), b'meas_cap'),
                      (dict(core=[0, 2]), b'core')):
        rc, msg = call(**kw)
        assert rc == -22 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert not acc.any().item() and res.cpu().numpy().tolist() == [[0, 0], [0, 0]]
