"""The resonator stage (dpemu_feedline_adc_res, include/dpemu.h; DESIGN.md §2
"Resonator response") on the CPU: its numpy restatement
(tests/resonator_ref.py) applied to oracle_dds waveforms -- the degenerate
equivalence with dpemu_feedline_adc, the Lorentzian line shape, ring-up and
ring-down, a dispersive readout through the statistics stage, the converter
noise -- and the Python-side resonator table.  The GPU kernel is held to the
same restatement bit for bit in tests/test_gpu_resonator.py.

Tolerance of the line-shape tests (LINE_TOL): |adc / d - H| / |H| past ten
time constants, d the delayed drive sample and H = c / (1 - a e^{-i phi_d}).
The recurrence itself contributes roundings of a few 1e-5 of full scale; the
deviation is the drive's own: its carrier phase is quantised to 12 bits (2 pi /
4096 = 1.5e-3 rad each way) sample by sample, which the resonator averages
over ~1 / (1 - |a|) samples while the ratio divides by the one quantised
sample, and its 32767 / 32768 factors.  Measured over test_line_shape's cases
on the CPU: worst 8.643e-4 at 1:1, 9.432e-4 at 16:4; the bound is twice the
worst, LINE_TOL = 1.9e-3.  Ring-down: RING_ABS = 2.2 LSB, three roundings of at
most 0.5 per component (0.71 in magnitude) -- the accumulated rounding of y
times the coupling (<= 0.71 gain, gain = 1), and the return's own at the
reference sample and at the sample compared."""

import cmath
import math

import numpy as np
import pytest

from distributed_processor_amd import ResonatorTable, _abi, isa
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.readout import ReadoutStats
from tests import feedline_ref, iq_stats_ref, resonator_ref
from tests.test_demod import ro_program
from tests.test_demod_iq import SQUARE
from tests.test_feedline import fl_cfg, iq16, switching_case, synth_cores

LINE_TOL = 1.9e-3
RING_ABS = 2.2


class PT:
    """the columns ResonatorTable reads of a DemodPairTable"""

    def __init__(self, pairs):
        self.n_pairs = len(pairs['lane'])
        self.cols = {k: np.asarray(v) for k, v in pairs.items()}


def cplx(words):
    i, q = iq16(words)
    return i.astype(np.float64) + 1j * q.astype(np.float64)


def run_res(cfg, pairs, lines, table, out, iq_d, n_lo, y_peak=None):
    return resonator_ref.feedline_adc_res(cfg, pairs, lines, table.coef, table.adc_sigma, out['summary'],
                                          out['events'], iq_d, n_lo, cfg.meas_cap, y_peak=y_peak)


def test_degenerate_equivalence():
    """pole 0 and the coupling of ro_theta: feedline_ref.feedline_adc's trace at unit gains, bit for bit (16:4
    and 1:1; lines of 4 staggered members -- one without a drive, one without a strobe -- with state switches
    inside the trace); a nonzero pole changes it"""
    env = np.full(500, SQUARE, np.uint32)
    f_d, f_lo = [0x03000000, 0x05100000, 0x07200000, 0x09300000], [0x03000100, 0x05100100, 0x07200100, 0x09300100]
    for spc in ((16, 4), (1, 1)):
        for variant in (False, True):
            cfg = fl_cfg(4, delay=5, theta=(0.4, 2.9), gain=(1.0, 1.0), p1=0.5, meas_cap=3, seed=0xFEED)
            out, pairs, iq_d, iq_l = synth_cores(switching_case(variant), cfg, f_d, f_lo, spc, spc, env, 1500,
                                                 n_shots=2, shot0=31)
            lines = [[0, 1, 2, 3], [6, 4, 7, 5]]
            n_lo = iq_l.shape[1]
            want = feedline_ref.feedline_adc(cfg, pairs, lines, out['summary'], out['events'], iq_d, n_lo, 3)
            coef = resonator_ref.degenerate_coef(cfg, 8)
            got = run_res(cfg, pairs, lines, ResonatorTable.from_coefficients(PT(pairs), coef), out, iq_d, n_lo)
            np.testing.assert_array_equal(got, want)
            assert want.any()
            states = {feedline_ref.state(cfg, 31 + s_, c, m) for s_ in range(2) for c in range(4) for m in range(3)}
            assert states == {0, 1}
            coef[:, :, 0] = 1 << 28
            other = run_res(cfg, pairs, lines, ResonatorTable.from_coefficients(PT(pairs), coef), out, iq_d, n_lo)
            assert (other != want).any()


# ---- one member, a square pulse of many ring-up times ------------------------------------------------------
KAPPA = int(0.005 * 2 ** 32)         # full linewidth, per clock: amplitude time constant 1 / (pi 0.005) = 64 clocks
PULSE_WORDS, DELAY, N_CLKS = 250, 7, 1300
DETUNINGS = (0, KAPPA // 2, -(KAPPA // 2), 2 * KAPPA)           # of the drive from f_res


def line_case(spc, det, f_res, state=0, gain=1.0, phase=0.0):
    """one core, one 1000-clock full-scale square drive pulse at f_res + det.  Returns (adc of the new stage, adc
    of the existing stage, the delayed drive, a, c, phi_d) as complex arrays / numbers per LO sample"""
    f_d = (f_res + det) & 0xFFFFFFFF
    read = [dict(A=65535, ph_d=12345, ph_lo=0, L_d=PULSE_WORDS, L_lo=20, lo_at=30)]
    cfg = fl_cfg(1, delay=DELAY, theta=(0.0, 0.0), p1=float(state), meas_cap=2)
    out, pairs, iq_d, iq_l = synth_cores([ro_program(read)], cfg, [f_d], [f_d], spc, spc,
                                         np.full(4 * PULSE_WORDS, SQUARE, np.uint32), N_CLKS)
    n_lo = iq_l.shape[1]
    tab = ResonatorTable(PT(pairs), [[f_res, (f_res + 999) & 0xFFFFFFFF][::1 if state == 0 else -1]], KAPPA, gain, phase)
    peak = []
    adc = run_res(cfg, pairs, [[0]], tab, out, iq_d, n_lo, y_peak=peak)
    old = feedline_ref.feedline_adc(cfg, pairs, [[0]], out['summary'], out['events'], iq_d, n_lo, cfg.meas_cap)
    d_i, d_q, st = resonator_ref.member_inputs(cfg, pairs, 0, out['summary'].view(np.uint32),
                                               out['events'].view(np.uint32), iq_d.view(np.uint32), n_lo, 2, 16)
    assert (st == state).all()
    a = complex(*tab.coef[0, state, :2]) / 2 ** 30
    c = complex(*tab.coef[0, state, 2:]) / 2 ** 30
    return cplx(adc[0]), cplx(old[0]), d_i + 1j * d_q, a, c, 2 * math.pi * f_d / (2.0 ** 32 * spc[1]), peak[0]


LINE_CASES = [(spc, det, f_res) for spc in ((1, 1), (16, 4)) for det in DETUNINGS
              for f_res in (0x0C345678, 0xC1234567)]            # the second is above 2^31: the unsigned convention


@pytest.fixture(scope='module')
def line_runs():
    return {k: line_case(*k) for k in LINE_CASES}


def pulse_span(d):
    nz = np.nonzero(d)[0]
    assert len(nz) == nz[-1] - nz[0] + 1                         # one contiguous pulse
    return int(nz[0]), int(nz[-1])


def test_line_shape(line_runs):
    """past ten time constants adc / d = H = c / (1 - a e^{-i phi_d}) within LINE_TOL |H|; on resonance H = gain
    e^{i phase}; |H| at 0, +-kappa / 2, 2 kappa is 1, 1 / sqrt 2, 1 / sqrt 17"""
    worst = {}
    for (spc, det, f_res), (adc, _, d, a, c, phi, peak) in line_runs.items():
        j0, j1 = pulse_span(d)
        tau = 1.0 / (1.0 - abs(a))                               # samples
        lo = j0 + int(10 * tau) + 1
        assert j1 - lo > 200 and abs(d[lo]) > 32000
        H = c / (1 - a * cmath.exp(-1j * phi))
        dev = float(np.abs(adc[lo:j1 + 1] / d[lo:j1 + 1] - H).max() / abs(H))
        worst[spc] = max(worst.get(spc, 0.0), dev)
        want = {0: 1.0, KAPPA // 2: 2 ** -0.5, -(KAPPA // 2): 2 ** -0.5, 2 * KAPPA: 17 ** -0.5}[det]
        assert abs(abs(H) - want) < 2e-3 * want, (spc, det, abs(H), want)
        if det:
            assert (cmath.phase(H) < 0) == (det > 0)             # the drive above the resonance lags
        assert dev <= LINE_TOL, (spc, det, hex(f_res), dev)
        assert 1e5 < peak < 2 ** 28
    print('worst |adc / d - H| / |H|:', {k: '{:.3e}'.format(v) for k, v in worst.items()}, 'LINE_TOL', LINE_TOL)


def test_gain_and_phase_on_resonance():
    adc, _, d, a, c, phi, _ = line_case((16, 4), 0, 0x0C345678, state=1, gain=0.5, phase=1.0)
    j0, j1 = pulse_span(d)
    lo = j0 + int(10 / (1 - abs(a))) + 1
    r = adc[lo:j1 + 1] / d[lo:j1 + 1]
    assert np.abs(r - 0.5 * cmath.exp(1j)).max() <= LINE_TOL * 0.5


def test_ring_up_and_ring_down(line_runs):
    """during the pulse |adc| / |d| follows |H| |1 - q^(k + 1)|, q = a e^{-i phi_d}, within LINE_TOL |H|; after
    the pulse's last sample the trace is nonzero and decays as |a|^k (within RING_ABS) where the existing
    stage's is exactly zero"""
    for (spc, det, f_res), (adc, old, d, a, c, phi, _) in line_runs.items():
        j0, j1 = pulse_span(d)
        q = a * cmath.exp(-1j * phi)
        H = c / (1 - q)
        k = np.arange(j1 - j0 + 1)
        want = abs(H) * np.abs(1 - q ** (k + 1))
        got = np.abs(adc[j0:j1 + 1]) / np.abs(d[j0:j1 + 1])
        assert np.abs(got - want).max() <= LINE_TOL * abs(H), (spc, det, np.abs(got - want).max() / abs(H))
        assert got[0] < 0.1 * abs(H) and abs(got[-1] - abs(H)) < 0.01 * abs(H)      # it does ring up
        tail, k = adc[j1 + 1:], np.arange(1, len(adc) - j1)
        assert len(tail) > 100 and not old[j1 + 1:].any() and old[j0:j1 + 1].all()
        assert np.abs(np.abs(tail) - abs(adc[j1]) * abs(a) ** k).max() <= RING_ABS
        n_tau = int(1 / (1 - abs(a)))
        assert abs(tail[0]) > 0.9 * abs(adc[j1]) and abs(tail[n_tau]) > 1000 and abs(tail[n_tau]) < 0.4 * abs(adc[j1])


# ---- dispersive readout through the statistics ----------------------------------------------------------------
CHI = KAPPA // 2
WINDOWS = (8, 160)                   # LO pulse words of 4 clocks: half a time constant (32 clocks) and ten (640)
DISP_F = [0x0C000000 + k * (2 ** 32 // 32) for k in (0, 3, 7)]    # tones whole turns per 32 clocks apart
DISP_DELAY = 20


def dispersive_case(window_words, seed=0xC0FFEE):
    """3 reading cores (a fourth idles) on one line per shot: core c's resonator at DISP_F[c] -+ CHI by state,
    its drive and LO midway at DISP_F[c]; a square 680-clock drive pulse, the LO window from its first returned
    clock; p1 = 0.5, no noise.  Returns (cfg, programs, frequency words, envelope, clocks)"""
    read = [dict(A=20000, ph_d=0, ph_lo=0, L_d=170, L_lo=window_words, lo_at=DISP_DELAY)]
    progs = [ro_program(read)] * 3 + [[isa.done_cmd()]]
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=16, meas_cap=4, meas_latency=32, seed=seed, p1=0.5,
                           lane_order=_abi.LANES_SHOT_MAJOR,
                           demod=dict(drv_elem=1, cpw=4, delay=DISP_DELAY, theta=(0.0, math.pi), sigma=0.0, axis=0.3))
    return cfg, progs, DISP_F + [DISP_F[0]], np.full(700, SQUARE, np.uint32), 720


def dispersive_f_res(cores):
    """f_res rows of ResonatorTable for pairs of these cores"""
    return [[(DISP_F[c % 3] - CHI) & 0xFFFFFFFF, (DISP_F[c % 3] + CHI) & 0xFFFFFFFF] for c in cores]


def predicted_acc(cfg, pairs, lines, tab, summary, events, iq_d, iq_l):
    """the float model of one readout per pair: member p's return is H (1 - q^(k + 1)) d_p at sample k of its one
    drive pulse (H, q of its state and DISP_F), the line's sum mixed with the pair's LO over readout 0's window"""
    summary, events = np.asarray(summary).view(np.uint32), np.asarray(events).view(np.uint32)
    iq_d, iq_l = np.asarray(iq_d).view(np.uint32), np.asarray(iq_l).view(np.uint32)
    n_lo = iq_l.shape[1]
    pred = np.zeros(len(pairs['lane']), np.complex128)
    for line in lines:
        total = np.zeros(n_lo, np.complex128)
        for p in line:
            d_i, d_q, st = resonator_ref.member_inputs(cfg, pairs, p, summary, events, iq_d, n_lo, cfg.meas_cap,
                                                       cfg.event_cap)
            d = d_i + 1j * d_q
            if not d.any():
                continue
            assert len(set(st.tolist())) == 1
            a, c = (complex(*tab.coef[p, st[0], q:q + 2]) / 2 ** 30 for q in (0, 2))
            spc_l = int(pairs['spc_lo'][p])
            q = a * cmath.exp(-2j * math.pi * DISP_F[int(pairs['core'][p])] / (2.0 ** 32 * spc_l))
            j0, j1 = pulse_span(d)
            k = np.arange(n_lo) - j0
            total += c / (1 - q) * (1 - q ** np.maximum(k + 1, 0)) * d       # (d is zero outside the pulse)
        for p in line:
            reads = feedline_ref.kept_readouts(cfg, summary, events, int(pairs['lane'][p]), cfg.meas_cap, cfg.event_cap)
            if not reads:
                continue
            spc_l = int(pairs['spc_lo'][p])
            t_lo, pe = reads[0]
            j = np.arange(t_lo * spc_l, (t_lo + ((pe >> 12) & 0xFFF) * cfg.ro_cpw) * spc_l)
            assert j[-1] < n_lo
            pred[p] = (total[j] * np.conj(cplx(iq_l[int(pairs['lo_row'][p])][j]))).sum() / (32768.0 * spc_l)
    return pred


def check_dispersive(cfg, pairs, tab, runs):
    """runs[window words] = (acc, result, predicted_acc).  Fidelity 1.0 at both windows; each class centroid at
    the angle the transient formula gives within the line-shape bound (LINE_TOL rad), which for the long
    window is that of H_s e^{-2 pi i f delay} (the return is the drive `delay` clocks late) within the
    transient's 0.06 rad; the short window's centroid separation over the long one's is the formula's ratio
    within the line-shape bound (LINE_TOL, relative), and less per sample.  Measured on the reference: angles
    within 3.2e-5 rad, ratios within 6.8e-5 -- the windows average the per-sample deviation the bound is for"""
    core, shot = np.asarray(pairs['core']), np.asarray(pairs['shot'])
    st = iq_stats_ref.states(cfg, shot, core, 0)
    sep, sep_want = {}, {}
    for w, (acc, res, pred) in runs.items():
        t, _ = iq_stats_ref.iq_stats(cfg, acc, res[:, 0], core=core, shot=shot)
        d = ReadoutStats(t, cfg).fit()
        assert d.fitted[:3].all()
        t, _ = iq_stats_ref.iq_stats(cfg, acc, res[:, 0], core=core, shot=shot, axis=d.axis_words, thr=d.thr)
        fid = ReadoutStats(t, cfg, axis=d.axis_words, thr=d.thr).fidelity()
        assert fid == 1.0, (w, fid)
        for c in range(3):
            cen, want = [], []
            for s_ in (0, 1):
                sel = (core == c) & (st == s_)
                assert sel.sum() > 10
                cen.append(complex(*acc[0, sel].astype(np.float64).mean(axis=0)))
                want.append(complex(pred[sel].mean()))
                assert abs(cen[-1]) > 20000 and abs(cmath.phase(cen[-1] / want[-1])) <= LINE_TOL, (w, c, s_)
                if w == WINDOWS[1]:
                    a, k = (complex(*tab.coef[c, s_, q:q + 2]) / 2 ** 30 for q in (0, 2))
                    spc_l = int(pairs['spc_lo'][c])
                    H = k / (1 - a * cmath.exp(-2j * math.pi * DISP_F[c] / (2.0 ** 32 * spc_l)))
                    rot = cmath.exp(-2j * math.pi * DISP_F[c] * DISP_DELAY / 2.0 ** 32)
                    assert abs(cmath.phase(cen[-1] / (H * rot))) < 0.06, (c, s_, cen[-1], H * rot)
            sep[w, c], sep_want[w, c] = abs(cen[1] - cen[0]), abs(want[1] - want[0])
    for c in range(3):
        got = sep[WINDOWS[0], c] / sep[WINDOWS[1], c]
        want = sep_want[WINDOWS[0], c] / sep_want[WINDOWS[1], c]
        print('core {}: centroid separation, short / long window {:.5f} (transient formula {:.5f})'.format(c, got, want))
        assert abs(got / want - 1) <= LINE_TOL, (c, got, want)
        assert got / (WINDOWS[0] / WINDOWS[1]) < 0.5             # per sample the short window separates less than half


def dispersive_lines(pairs):
    """one line per shot of its three reading cores, then the idle cores alone"""
    core, shot = np.asarray(pairs['core']), np.asarray(pairs['shot'])
    by_shot = {}
    for i in np.nonzero(core < 3)[0]:
        by_shot.setdefault(int(shot[i]), []).append(int(i))
    return list(by_shot.values()) + [[int(i)] for i in np.nonzero(core == 3)[0]]


def test_dispersive_readout_through_the_statistics():
    runs = {}
    for w in WINDOWS:
        cfg, progs, f, env, n_clks = dispersive_case(w)
        out, pairs, iq_d, iq_l = synth_cores(progs, cfg, f, f, (4, 4), (4, 4), env, n_clks, n_shots=64, shot0=500)
        lines = dispersive_lines(pairs)
        assert len(lines) == 128 and all(len(ln) == 3 for ln in lines[:64])
        tab = ResonatorTable(PT(pairs), dispersive_f_res(pairs['core']), KAPPA)
        adc = run_res(cfg, pairs, lines, tab, out, iq_d, iq_l.shape[1])
        assert max(np.abs(v).max() for v in iq16(adc)) < 32767
        acc, res = feedline_ref.demod_feedline(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l, cfg.meas_cap)
        runs[w] = (acc, res, predicted_acc(cfg, pairs, lines, tab, out['summary'], out['events'], iq_d, iq_l))
    check_dispersive(cfg, pairs, tab, runs)


# ---- converter noise ------------------------------------------------------------------------------------------
def test_converter_noise():
    """no drive pulse: adc = clamp(nu), the same whichever line composition its first member is in, different
    between shots, absent at adc_sigma 0; mean and variance of nu over 4,096 samples"""
    cfg = fl_cfg(2, meas_cap=2, seed=0xABCDEF)
    lo_only = [isa.pulse_reset(), isa.pulse_cmd(freq_word=0, phase_word=0, amp_word=0xFFFF, env_word=20 << 12,
                                                cfg_word=2, cmd_time=40), isa.done_cmd()]
    out, pairs, iq_d, iq_l = synth_cores([lo_only] * 2, cfg, [0x01000000] * 2, [0x01000000] * 2, (1, 1), (1, 1),
                                         np.full(100, SQUARE, np.uint32), 4096, n_shots=3, shot0=9)
    assert not iq_d.any() and iq_l.shape[1] == 4096
    pt = PT(pairs)
    coef = np.zeros((6, 2, 4), np.int64)
    coef[..., 0], coef[..., 2] = 900 << 20, 1 << 29
    sigma = 640
    tab = ResonatorTable.from_coefficients(pt, coef, sigma)

    def run(lines, t=tab):
        return run_res(cfg, pairs, lines, t, out, iq_d, 4096)
    a = run([[0, 1], [2, 3], [4, 5]])
    b = run([[4], [0, 3, 5], [2]])
    np.testing.assert_array_equal(a[0], b[1])                    # first member pair 0 = (shot 9, core 0)
    np.testing.assert_array_equal(a[1], b[2])
    np.testing.assert_array_equal(a[2], b[0])
    c = run([[1, 0]])                                            # first member (shot 9, core 1): another stream
    assert (a[0] != a[1]).mean() > 0.9 and (a[0] != c[0]).mean() > 0.9
    assert not run([[0, 1]], ResonatorTable.from_coefficients(pt, coef, 0)).any()
    nu_i, nu_q = resonator_ref.adc_noise(cfg.seed, 9, 0, 4096, sigma)
    np.testing.assert_array_equal(iq16(a[0])[0], np.clip(nu_i, -32767, 32767))
    np.testing.assert_array_equal(iq16(a[0])[1], np.clip(nu_q, -32767, 32767))
    # the state draws and the readout noise of the same (shot, core) use counters without the high bit
    from tests.demod_iq_ref import philox4
    assert resonator_ref.philox4_vec(cfg.seed, 9, 0, np.arange(3)).T.tolist() == \
        [philox4(cfg.seed, 9, 0, m) for m in range(3)]
    var_want = sigma ** 2 * (65536.0 ** 2 - 1) / (3 * 2.0 ** 32)
    for nu in (nu_i, nu_q):
        nu = nu.astype(np.float64)
        assert np.abs(nu).max() < 32767
        assert abs(nu.mean()) <= 5 * math.sqrt(var_want / 4096), nu.mean()
        assert abs(nu.var() / var_want - 1) <= 0.12, nu.var() / var_want
    # a huge sigma clips symmetrically
    big = run([[0]], ResonatorTable.from_coefficients(pt, coef, 2 ** 32 - 1))
    assert iq16(big[0])[0].min() == -32767 and iq16(big[0])[0].max() == 32767


# ---- the table ------------------------------------------------------------------------------------------------
def test_resonator_table():
    pt = PT(dict(lane=[0, 1], spc_lo=[4, 1]))
    # kappa = 2^32 / 64 per clock at spc_lo 4: |a| = exp(-pi / 256); f_res a quarter turn per clock: arg a = pi / 8
    tab = ResonatorTable(pt, [[2 ** 30, 0], [0, 2 ** 31]], 2 ** 26, gain=[[1.0, 0.5], [1.0, 1.0]],
                         phase=[[0.0, math.pi / 2], [0.0, 0.0]], adc_sigma=1.5)
    mag4, mag1 = math.exp(-math.pi / 256), math.exp(-math.pi / 64)
    want = [[[mag4 * math.cos(math.pi / 8), mag4 * math.sin(math.pi / 8), 1 - mag4, 0.0],
             [mag4, 0.0, 0.0, 0.5 * (1 - mag4)]],
            [[mag1, 0.0, 1 - mag1, 0.0], [-mag1, 0.0, 1 - mag1, 0.0]]]
    np.testing.assert_array_equal(tab.coef, np.rint(np.array(want) * 2 ** 30).astype(np.int32))
    assert tab.coef.dtype == np.int32 and tab.coef.shape == (2, 2, 4) and tab.coef.flags.c_contiguous
    # by hand (50-digit decimal series): 2^30 exp(-pi / 256) (cos, sin)(pi / 8) = 979908716.23, 405891480.15;
    # 2^30 (1 - exp(-pi / 256)) = 13096272.56, half of it 6548136.28; 2^30 exp(-pi / 64) = 1022307364.53
    assert tab.coef[0].tolist() == [[979908716, 405891480, 13096273, 0], [1060645551, 0, 0, 6548136]]
    assert tab.coef[1].tolist() == [[1022307365, 0, 51434459, 0], [-1022307365, 0, 51434459, 0]]
    assert tab.adc_sigma == 98304
    st = tab.struct()
    assert st.coef == tab.coef.ctypes.data and st.adc_sigma == 98304
    # a pole of f_res above 2^31 turns the unsigned way at spc_lo > 1
    up = ResonatorTable(pt, [[3 * 2 ** 30, 0], [0, 0]], 2 ** 26)
    assert up.coef[0, 0, 1] > 0 and abs(math.atan2(up.coef[0, 0, 1], up.coef[0, 0, 0]) - 3 * math.pi / 8) < 1e-6
    ok = np.zeros((2, 2, 4), np.int64)
    lim = (1 << 30) - (1 << 18)
    ok[0, 0, :2], ok[1, 1, :2], ok[0, 1, 2:], ok[1, 0, 2:] = (lim, 0), (0, -lim), (1 << 30, -(1 << 30)), (-(1 << 30), 0)
    assert ResonatorTable.from_coefficients(pt, ok, 2 ** 32 - 1).coef.tolist() == ok.tolist()
    for at, val, word in (((0, 0, 0), lim + 1, 'pole'), ((1, 1, 1), -lim - 1, 'pole'),
                          ((0, 1, 2), (1 << 30) + 1, 'coupling'),
                          ((1, 0, 3), -(1 << 30) - 1, 'coupling')):
        bad = ok.copy()
        bad[at] = val
        with pytest.raises(DpemuError, match=word):
            ResonatorTable.from_coefficients(pt, bad)
    bad = ok.copy()
    bad[0, 0, :2] = (760000000, 760000000)                   # each component inside, the magnitude outside
    with pytest.raises(DpemuError, match='pole'):
        ResonatorTable.from_coefficients(pt, bad)
    with pytest.raises(DpemuError, match='pairs'):
        ResonatorTable.from_coefficients(pt, ok[:1])
    with pytest.raises(DpemuError, match='adc_sigma'):
        ResonatorTable.from_coefficients(pt, ok, 2 ** 32)
    with pytest.raises(DpemuError, match='pole'):                 # kappa too small: |a| > 1 - 2^-12
        ResonatorTable(pt, [[0, 0], [0, 0]], 1000)
    with pytest.raises(DpemuError, match='coupling'):
        ResonatorTable(pt, [[0, 0], [0, 0]], 2 ** 31, gain=3.0)
    with pytest.raises(DpemuError, match='f_res'):
        ResonatorTable(pt, [0, 0], 2 ** 26)
    with pytest.raises(DpemuError, match='f_res'):
        ResonatorTable(pt, [[0, 2 ** 32], [0, 0]], 2 ** 26)
    with pytest.raises(DpemuError, match='kappa'):
        ResonatorTable(pt, [[0, 0], [0, 0]], -1)
