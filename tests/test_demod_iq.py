"""The waveform demodulation stage (dpemu_demod_iq, include/dpemu.h; DESIGN.md
§2 "Waveform demodulation") on the CPU: its numpy restatement
(tests/demod_iq_ref.py) applied to oracle_dds waveforms, against the DEMOD
model's flat-top closed form (oracle.fast_run, ro_sigma = 0) -- the first test
that ties the closed form to the DDS it claims to demodulate -- and the
Python-side pair table.  The GPU kernel is held to the same restatement bit
for bit in tests/test_gpu_demod_iq.py.

Tolerance of "waveform == closed form" (flat_tolerance): |dI|, |dQ| <= REL_TOL
|acc| + ABS_TOL.  ABS_TOL = 64 covers the integer roundings, which do not
scale with the sum: the >> 15 of the DDS drive sample, of the return and of
the LO sample (weight ~0.6) each leave +-0.5 uniform per sample, variance
(1 + 1 + 0.36) / 12, sigma 0.44; a 1000-clock window at one sample per clock
adds 1000 of them, sigma 14 (at 4 samples per clock 4000 of them divided by
4: sigma 7), and the bound is four sigma, rounded up.  The relative part is
the 12-bit carrier phase of the two DDS channels and of theta (2 pi / 4096 =
1.5e-3 each way) and the three 32767 / 32768 factors.  Measured over
test_flat_top_matches_closed_form's cases on the CPU: worst (max(|dI|, |dQ|)
- ABS_TOL) / |acc| = 1.099e-3; the bound is twice that, REL_TOL = 2.2e-3
(< 1e-2, above which a difference is a
convention error, not rounding)."""

import math
import random

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, isa, workloads
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.hwconfig import DDSElementConfig
from tests import demod_iq_ref
from tests.progfuzz import pack_programs
from tests.test_demod import RDLO, RDRV, ro_program

ABS_TOL = 64
REL_TOL = 2.2e-3
F_CLK = 500e6
SQUARE = 0x7FFF0000            # env word: I = 32767 (high half), Q = 0


def flat_tolerance(acc):
    """the bound on |dI| and |dQ| between a waveform acc and the closed form `acc`"""
    return REL_TOL * float(np.hypot(*np.asarray(acc, np.float64))) + ABS_TOL


def freq_buffer(word, spc):
    """one entry of an element's freq buffer (asmparse.py:64-86 format: the
    32-bit word, then the 15 sub-sample rotations) for frequency word `word`"""
    buf = DDSElementConfig(samples_per_clk=spc).get_freq_buffer([word * F_CLK / 2 ** 32])
    assert int(buf[0]) == word
    return buf


def synth(words, cfg, f_d, f_lo, spc, interp, env_d, env_lo, n_clks, n_shots=1, shot0=0, clip=(None, None)):
    """one core running `words`: oracle.fast_run (events, closed-form acc), then
    oracle.dds of the drive and LO channels of every shot.  Returns (fast
    outputs, pair table, iq_drv, iq_lo)."""
    pw, offs, ni = pack_programs([words])
    ro = (np.array([f_d, f_lo], np.uint32), np.array([0], np.uint32), np.array([1], np.uint32),
          np.array([1], np.uint32), np.array([1], np.uint32))
    out = oracle.fast_run(cfg, pw, offs, ni, np.zeros(1, np.uint32), shot0, n_shots, ro=ro)
    iq = []
    for elem, f, env, s_, ip, n_clip in ((RDRV, f_d, env_d, spc[0], interp[0], clip[0]),
                                         (RDLO, f_lo, env_lo, spc[1], interp[1], clip[1])):
        fb = freq_buffer(f, s_)
        desc = [(lane, elem, s_, ip, 0, len(env), 0, len(fb)) for lane in range(n_shots)]
        n = n_clks * s_ if n_clip is None else n_clip
        iq.append(oracle.dds(desc, out['summary'], out['events'], env, fb, n, cfg.event_cap))
    pairs = dict(lane=np.arange(n_shots), core=np.zeros(n_shots, int), shot=shot0 + np.arange(n_shots),
                 drv_row=np.arange(n_shots), lo_row=np.arange(n_shots), spc_drv=[spc[0]] * n_shots,
                 spc_lo=[spc[1]] * n_shots)
    return out, pairs, iq[0], iq[1]


def demod_cfg(delay, theta, gain, p1, sigma=0.0, meas_cap=4, axis=0.0, seed=0x5EED):
    return _abi.make_config(1, max_cycles=1 << 22, event_cap=16, meas_cap=meas_cap, meas_latency=32, p1=p1,
                            seed=seed, demod=dict(drv_elem=RDRV, cpw=4, delay=delay, theta=theta, gain=gain,
                                                  sigma=sigma, axis=axis))


# (ro_delay, lo_at, extra drive words): full overlap at delay 0 (the drive one
# word longer than the window that starts 3 clocks into it) and at delay 300;
# the window starting after / before the return, and ending after it
OVERLAPS = ((0, 3, 1), (300, 300, 0), (300, 310, 0), (300, 290, 0), (0, 3, 0))
# detunings F_d - F_lo: zero, Hz-scale words (one word = 0.116 Hz), and 2^20
# words = 122 kHz, a quarter turn over a 1000-clock window.  The waveform sum
# has spc_lo sub-sample terms per clock where the closed form has one, so it
# carries the factor mean_k e^{i beta k / spc_lo}: at 2^20 words
# that is 5.8e-4 from 1; test_subsample_factor_at_large_detuning takes a
# detuning at which the factor itself is the test
DETUNINGS = (0, 1, -3, 7, 1 << 20)
RATES = (((16, 4), (16, 4)), ((4, 4), (4, 4)), ((1, 1), (1, 1)))      # (spc drv, lo), (interp drv, lo)
LENGTHS = (1, 7, 250)


def flat_case(rates, det, state, overlap, seed, lengths=LENGTHS):
    """one program of len(lengths) reads with square envelopes; returns the
    closed-form acc and the waveform acc of every read"""
    rng = random.Random(seed)
    (spc, interp), (delay, lo_at, extra) = rates, overlap
    f_d = rng.getrandbits(32)
    f_lo = (f_d - det) & 0xFFFFFFFF
    reads = [dict(A=rng.randint(20000, 65535), ph_d=rng.getrandbits(17), ph_lo=rng.getrandbits(17), L_d=L + extra,
                  L_lo=L, lo_at=lo_at, gap=1500) for L in lengths]
    cfg = demod_cfg(delay, (rng.uniform(-4, 4), rng.uniform(-4, 4)), (0.3 + 0.7 * rng.random(), 1.0), float(state))
    env = np.full(4 * (max(lengths) + 1), SQUARE, np.uint32)
    out, pairs, iq_d, iq_l = synth(ro_program(reads), cfg, f_d, f_lo, spc, interp, env, env,
                                   10 + 1500 * len(lengths))
    acc, res = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, cfg.meas_cap)
    assert int(res[0, 0]) == len(lengths) == int(out['summary'][0, 5])
    return out['acc'][:len(lengths), 0].astype(np.int64), acc[:len(lengths), 0].astype(np.int64)


def flat_cases():
    k = 0
    for rates in RATES:
        for det in DETUNINGS:
            for state in (0, 1):
                for ov in OVERLAPS:
                    k += 1
                    yield rates, det, state, ov, 9000 + k


def test_flat_top_matches_closed_form():
    """square envelopes at 32767, full-scale LO: the demodulated waveforms give
    the DEMOD model's closed-form acc (sample rates 16:4, 4:4, 1:1; detunings
    0, Hz-scale and 2^20 words; both states; delays 0 and 300; full and partial
    overlaps; windows of 1, 7 and 250 words) within flat_tolerance.  Measured
    worst relative deviation 1.099e-3, bound REL_TOL = 2.2e-3 (module docstring)."""
    worst, big = 0.0, 0
    for rates, det, state, ov, seed in flat_cases():
        cf, wave = flat_case(rates, det, state, ov, seed)
        for a, b in zip(cf, wave):
            err, mag = int(np.abs(a - b).max()), float(np.hypot(*a.astype(np.float64)))
            if mag > 0:
                worst = max(worst, max(0, err - ABS_TOL) / mag)
            big += mag > 1e6
            assert err <= flat_tolerance(a), (rates, det, state, ov, a, b)
    print('worst relative deviation {:.3e} (REL_TOL {:.1e})'.format(worst, REL_TOL))
    assert big > 100                     # the long windows carry real signal
    assert REL_TOL < 1e-2


def test_subsample_factor_at_large_detuning():
    """a detuning of 0.01 turns per clock (5 MHz): the waveform sum has spc_lo
    terms per clock, the closed form one, so acc_wave = closed form *
    mean_k e^{2 pi i det k / (2^32 spc_lo)} (2.4 % from 1 at 4 samples per
    clock, exactly 1 at 1), within the flat-top tolerance"""
    det = int(0.01 * 2 ** 32)
    for rates in RATES:
        spc_lo = rates[0][1]
        g = np.mean(np.exp(2j * np.pi * det * np.arange(spc_lo) / (2 ** 32 * spc_lo)))
        for state in (0, 1):
            cf, wave = flat_case(rates, det, state, OVERLAPS[1], 7000 + state, lengths=(7, 250))
            for a, b in zip(cf, wave):
                want = complex(*a) * g
                tol = flat_tolerance(a)
                assert abs(b[0] - want.real) <= tol and abs(b[1] - want.imag) <= tol, (rates, state, a, b, want)
                if spc_lo > 1 and abs(complex(*a)) > 1e4:
                    assert abs(complex(*b) - complex(*a)) > 3 * tol      # the factor is visible


def envelope_case(env_d, state=1):
    """config 3's readout shape (1000 clocks, delay = lo_at = 300, 16:4) with
    drive envelope table env_d at zero detuning; (closed form, waveform, mean
    envelope / 32767)"""
    f = 0x1999999A
    cfg = demod_cfg(300, (math.pi, 0.0), (1.0, 1.0), float(state))
    reads = [dict(A=39321, ph_d=0, ph_lo=14597, L_d=250, L_lo=250, lo_at=300)]
    out, pairs, iq_d, iq_l = synth(ro_program(reads), cfg, f, f, (16, 4), (16, 4), env_d,
                                   np.full(1000, SQUARE, np.uint32), 1400)
    acc, _ = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, cfg.meas_cap)
    mean = float(demod_iq_ref.s16(env_d >> 16)[:1000].mean()) / 32767
    return out['acc'][0, 0].astype(np.int64), acc[0, 0].astype(np.int64), mean


def test_envelope_weights_the_accumulator():
    """the gap the flat-top model leaves: with workloads.RDRV_ENV (cos_edge_square,
    ramp fraction 0.25) the waveform acc is the closed form times mean(env) /
    32767 = 0.75, within the flat-top tolerance -- and more than ten times
    that tolerance away from the unscaled closed form"""
    env = DDSElementConfig(**workloads.ELEMS[RDRV]).get_env_buffer(workloads.RDRV_ENV)
    assert len(env) == 1000 and not (env & 0xFFFF).any()
    for state in (0, 1):
        cf, wave, mean = envelope_case(env, state)
        assert 0.74 < mean < 0.76
        tol = flat_tolerance(cf)
        assert np.abs(wave - cf * mean).max() <= tol, (cf, wave, mean)
        assert np.abs(wave - cf).max() > 10 * tol
        assert np.hypot(*cf.astype(float)) > 1.9e7


def lo_only_program(t=10, L=250):
    return [isa.pulse_reset(), isa.pulse_cmd(freq_word=0, phase_word=0, amp_word=0xFFFF, env_word=L << 12,
                                             cfg_word=RDLO, cmd_time=t), isa.done_cmd()]


def test_no_drive_or_empty_window_reads_noise_only():
    """without a drive pulse, or with the window clipped to nothing by the LO
    buffer, acc is the DEMOD model's noise of the same (shot, core, m)"""
    cfg = demod_cfg(300, (0.3, 2.0), (1.0, 1.0), 0.5, sigma=1.5)
    env = np.full(1000, SQUARE, np.uint32)
    n, shot0 = 16, 123456789012
    out, pairs, iq_d, iq_l = synth(lo_only_program(), cfg, 5, 5, (16, 4), (16, 4), env, env, 1100, n, shot0)
    assert not iq_d.any() and iq_l.any()
    acc, res = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, cfg.meas_cap)
    assert (res[:, 0] == 1).all()
    np.testing.assert_array_equal(acc, out['acc'])               # fast_run: no drive -> noise only
    assert np.abs(acc[0]).max() > 10000 and not acc[1:].any()
    # a drive is there, but the LO buffer ends before the window starts
    reads = [dict(L_d=250, L_lo=250, lo_at=300)]
    out2, pairs, iq_d, iq_l = synth(ro_program(reads), cfg, 5, 5, (16, 4), (16, 4), env, env, 1400, n, shot0,
                                    clip=(None, 4 * 310))
    acc2, res2 = demod_iq_ref.demod_iq(cfg, pairs, out2['summary'], out2['events'], iq_d, iq_l, cfg.meas_cap)
    assert (res2[:, 0] == 1).all() and iq_d.any()
    np.testing.assert_array_equal(acc2, out['acc'])
    for i in range(n):                                           # the noise formula itself
        _, zi, zq = demod_iq_ref.noise(cfg.seed, shot0 + i, 0, 0, cfg.ro_sigma)
        assert (zi, zq) == tuple(int(v) for v in acc[0, i])


def test_buffer_clipping_and_meas_cap():
    """clipping the window by n_samples_lo or n_samples_drv equals
    zero-extending the buffers; reads beyond meas_cap are dropped, count
    saturates and unused slots are zero"""
    cfg = demod_cfg(300, (0.3, 2.0), (0.8, 1.0), 0.5, sigma=0.5, axis=1.0)
    env = np.full(1000, SQUARE, np.uint32)
    reads = [dict(L_d=250, L_lo=250, lo_at=300, gap=1500, ph_d=1000 * k) for k in range(3)]
    out, pairs, iq_d, iq_l = synth(ro_program(reads), cfg, 77, 70, (16, 4), (16, 4), env, env, 4700, 2, 40)
    full, res = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, 4)
    assert (res[:, 0] == 3).all() and full[:3].all() and not full[3].any()
    for n_d, n_l in ((16 * 2400, 4 * 4700), (16 * 4700, 4 * 3900), (16 * 1701, 4 * 3333)):
        zd, zl = iq_d.copy(), iq_l.copy()
        zd[:, n_d:] = 0
        zl[:, n_l:] = 0
        a0, r0 = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], zd, zl, 4)
        a1, r1 = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d[:, :n_d], iq_l[:, :n_l], 4)
        np.testing.assert_array_equal(a0, a1)
        np.testing.assert_array_equal(r0, r1)
        assert not np.array_equal(a0, full)
    a2, r2 = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, 2)
    assert a2.shape == (2, 2, 2) and (r2[:, 0] == 2).all()
    np.testing.assert_array_equal(a2, full[:2])
    np.testing.assert_array_equal(r2[:, 1], res[:, 1] & 3)
    # event_cap hides later events, as for the DDS: 1 reset + 2 reads + the third drive
    a3, r3 = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, 4, event_cap=6)
    assert (r3[:, 0] == 2).all() and not a3[2:].any()


def test_pair_table_and_argument_checks():
    """the Python side without a device: ChannelPlan keeps its triples, the pair
    table pairs row i with row i and refuses mismatched plans and wrong
    elements, and demodulate's tensor checks refuse what they can see"""
    import torch
    from distributed_processor_amd.dds import ChannelPlan, DemodPairTable
    from distributed_processor_amd.emulator import ProgramSet
    from distributed_processor_amd.stage_tensors import check_demod_tensors
    ps = ProgramSet(workloads.config3_active_reset(2))
    cfg = _abi.make_config(2, n_groups=ps.n_groups, max_cycles=50000, event_cap=16, meas_cap=4,
                           lane_order=_abi.LANES_SHOT_MAJOR, demod=workloads.config3_demod(ps))
    params = {RDRV: (16, 16), RDLO: (4, 4)}
    who = [(100 + s_, c) for s_ in range(3) for c in range(2)]
    drv = ChannelPlan(ps, cfg, 100, 3, [(s_, c, RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, 100, 3, [(s_, c, RDLO) for s_, c in who], params)
    assert drv.channels == [(s_, c, RDRV) for s_, c in who]
    pt = DemodPairTable(cfg, drv, lo)
    assert pt.n_pairs == 6 and pt.n_lanes == 6 and pt.n_rows == (6, 6)
    np.testing.assert_array_equal(pt.cols['lane'], [(s_ - 100) * 2 + c for s_, c in who])
    np.testing.assert_array_equal(pt.cols['core'], [c for _, c in who])
    np.testing.assert_array_equal(pt.cols['shot'], [s_ for s_, _ in who])
    np.testing.assert_array_equal(pt.cols['drv_row'], np.arange(6))
    np.testing.assert_array_equal(pt.cols['spc_drv'], [16] * 6)
    np.testing.assert_array_equal(pt.cols['spc_lo'], [4] * 6)
    st = pt.struct(4, 1600, 400)
    assert (st.n_pairs, st.n_lanes, st.event_cap, st.meas_cap, st.n_samples_drv, st.n_samples_lo) == \
        (6, 6, 16, 4, 1600, 400) and pt.cols['shot'].dtype == np.uint64
    # both channels in one plan
    both = ChannelPlan(ps, cfg, 100, 3, [(s_, c, e) for s_, c in who for e in (RDRV, RDLO)], params)
    one = DemodPairTable.one_plan(cfg, both)
    np.testing.assert_array_equal(one.cols['drv_row'], np.arange(0, 12, 2))
    np.testing.assert_array_equal(one.cols['lo_row'], np.arange(1, 12, 2))
    # refusals
    lo_rev = ChannelPlan(ps, cfg, 100, 3, [(s_, c, RDLO) for s_, c in reversed(who)], params)
    for bad in ((drv, lo_rev), (lo, drv), (drv, drv),
                (drv, ChannelPlan(ps, cfg, 100, 3, [(s_, c, RDLO) for s_, c in who[:5]], params)),
                (drv, ChannelPlan(ps, cfg, 100, 3, [(s_, c, RDLO) for s_, c in who], {RDLO: (3, 1)}))):
        with pytest.raises(DpemuError):
            DemodPairTable(cfg, *bad)
    summ, ev = torch.zeros((6, 8), dtype=torch.int32), torch.zeros((16, 6, 4), dtype=torch.int32)
    iq_d, iq_l = torch.zeros((6, 1600), dtype=torch.int32), torch.zeros((6, 400), dtype=torch.int32)
    with pytest.raises(DpemuError, match='events'):
        check_demod_tensors(pt, cfg, iq_d, iq_l, dict(summary=summ), None, None, 0)
    with pytest.raises(DpemuError, match='iq_drv'):
        check_demod_tensors(pt, cfg, iq_d[:5], iq_l, dict(summary=summ, events=ev), None, None, 0)
    with pytest.raises(DpemuError, match='cpu'):                 # host tensors are not device tensors
        check_demod_tensors(pt, cfg, iq_d, iq_l, dict(summary=summ, events=ev), None, None, 0)
    cfg.meas_cap = 0
    with pytest.raises(DpemuError, match='meas_cap'):
        check_demod_tensors(pt, cfg, iq_d, iq_l, dict(summary=summ, events=ev), None, None, 0)
