"""The averaged readout traces (dpemu_feedline_traces, include/dpemu.h; DESIGN.md
§2 "Averaged traces and matched filter") on the CPU: their numpy restatement
(tests/traces_ref.py) on the existing numpy pipeline (test_feedline.synth_cores,
resonator_ref, feedline_ref, iq_stats_ref) -- the sum identity with the
demodulator, the ring-up of the resonator stage seen bin by bin, the
matched-filter loop through the statistics, the Python-side ``ReadoutTraces``
-- and the proof, from the references alone, that the inputs of
tests/test_gpu_traces.py reach what they are for.  The GPU kernel is held to
the same restatement bit for bit in tests/test_gpu_traces.py.

Tolerances.  Ring-up: test_resonator.LINE_TOL, the project's per-sample
line-shape bound, relative to the trace's peak.  The matched-filter loop:
AXIS_TOL and GAIN_TOL, each twice the worst deviation measured on the numpy
reference over MF_SEEDS (the figures are in check_loop's docstring)."""

import cmath
import functools
import math

import numpy as np
import pytest

import oracle
from distributed_processor_amd import ResonatorTable, _abi, isa
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable
from distributed_processor_amd.hwconfig import DDSElementConfig
from distributed_processor_amd.readout import ReadoutStats, ReadoutTraces, axis_halves
from tests import feedline_ref, handbuilt as hb, iq_stats_ref, resonator_ref, traces_ref
from tests.demod_iq_ref import s16
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, freq_buffer
from tests.test_feedline import fl_cfg, synth_cores
from tests.test_resonator import (DISP_DELAY, DISP_F, KAPPA, LINE_TOL, PT, WINDOWS, cplx, dispersive_case,
                                  dispersive_f_res, dispersive_lines, pulse_span)

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


# ---- 1. the sum identity ---------------------------------------------------------------------------------------
def check_sum_identity(cfg, pairs, traces, acc, res, bin_clocks):
    """by_slot traces of pairs that are alone in their (slot, core, state) class: the sum of (w2, w3) over the bins
    is the demodulator's S, so acc = sat((S + 2^(h-1)) >> h) bit for bit (ro_sigma = 0); returns the classes seen"""
    assert cfg.ro_sigma == 0
    seen = 0
    for i in range(len(pairs['lane'])):
        core, shot = int(pairs['core'][i]), int(pairs['shot'][i])
        h = 15 + int(pairs['spc_lo'][i]).bit_length() - 1
        for m in range(int(res[i, 0])):
            row = traces[m, core, feedline_ref.state(cfg, shot, core, m)]
            assert row[:, 0].max() == 1                      # one readout in the class
            for comp in (0, 1):
                S = int(row[:, 2 + comp].sum())
                want = max(INT32_MIN, min(INT32_MAX, (S + (1 << (h - 1))) >> h))
                assert int(acc[m, i, comp]) == want, (i, m, comp)
            seen += 1
    return seen


def sum_identity_case(spc):
    """two cores, one shot, each pair alone on its line; windows of 1, 7 and 60 words (240 clocks)"""
    env = np.full(4 * 70, SQUARE, np.uint32)
    reads = [[dict(A=30000 + 9000 * c + 1000 * k, ph_d=9000 * k + c, ph_lo=555 * c, L_d=L, L_lo=L, lo_at=21 + c,
                   gap=400) for k, L in enumerate((1, 7, 60))] for c in range(2)]
    cfg = fl_cfg(2, delay=20, gain=(0.9, 0.7), sigma=0.0, p1=0.5)
    out, pairs, iq_d, iq_l = synth_cores([ro_program(r) for r in reads], cfg, [0x1234567, 0x7654321],
                                         [0x1234560, 0x7654300], spc, spc, env, 1100)
    return cfg, out, pairs, iq_d, iq_l


@pytest.mark.parametrize('spc', [(16, 4), (1, 1)], ids=['16_4', '1_1'])
def test_sum_identity(spc):
    cfg, out, pairs, iq_d, iq_l = sum_identity_case(spc)
    lines = [[0], [1]]
    adc, acc, res = feedline_ref.feedline(cfg, pairs, lines, out['summary'], out['events'], iq_d, iq_l, cfg.meas_cap)
    assert (res[:, 0] == 3).all() and np.abs(acc[2].astype(np.int64)).max() > 10 ** 5
    for bin_clocks, n_bins in ((1, 240), (3, 80), (7, 35)):
        tr = traces_ref.feedline_traces(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l, cfg.meas_cap,
                                        n_bins, bin_clocks, by_slot=True)
        assert n_bins * bin_clocks >= 240 and check_sum_identity(cfg, pairs, tr, acc, res, bin_clocks) == 6
        assert tr[..., 1].sum() == 2 * (4 + 28 + 240) * spc[1]
    # a table that does not cover the window drops samples: the identity needs the cover
    short = traces_ref.feedline_traces(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l, cfg.meas_cap, 100,
                                       1, by_slot=True)
    assert short[2, ..., 1].sum() == 2 * 100 * spc[1]


# ---- 2. ring-up ------------------------------------------------------------------------------------------------
def predicted_traces(cfg, pairs, lines, tab, summary, events, iq_d, iq_l, n_bins):
    """test_resonator.predicted_acc's float model, bin by bin: member p's return is H (1 - q^(k + 1)) d_p at
    sample k of its one drive pulse, the line's sum mixed with the pair's LO; the mean over the samples of
    readout 0 of every pair of a (core, state) class, per clock from the strobe.  complex [C, 2, n_bins]"""
    summary, events = np.asarray(summary).view(np.uint32), np.asarray(events).view(np.uint32)
    iq_d, iq_l = np.asarray(iq_d).view(np.uint32), np.asarray(iq_l).view(np.uint32)
    n_lo = iq_l.shape[1]
    tot = np.zeros((cfg.cores_per_shot, 2, n_bins), np.complex128)
    cnt = np.zeros((cfg.cores_per_shot, 2, n_bins))
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
            j0, _ = pulse_span(d)
            k = np.arange(n_lo) - j0
            total += c / (1 - q) * (1 - q ** np.maximum(k + 1, 0)) * d
        for p in line:
            core, shot = int(pairs['core'][p]), int(pairs['shot'][p])
            reads = feedline_ref.kept_readouts(cfg, summary, events, int(pairs['lane'][p]), cfg.meas_cap, cfg.event_cap)
            if not reads:
                continue
            spc_l = int(pairs['spc_lo'][p])
            t_lo, pe = reads[0]
            j = np.arange(t_lo * spc_l, (t_lo + ((pe >> 12) & 0xFFF) * cfg.ro_cpw) * spc_l)
            assert j[-1] < n_lo
            b = j // spc_l - t_lo
            keep = b < n_bins
            P = total[j] * np.conj(cplx(iq_l[int(pairs['lo_row'][p])][j]))
            s_ = feedline_ref.state(cfg, shot, core, 0)
            np.add.at(tot[core, s_], b[keep], P[keep])
            np.add.at(cnt[core, s_], b[keep], 1)
    with np.errstate(invalid='ignore'):
        return tot / cnt                                 # (nan for the idle core)


@functools.lru_cache(maxsize=None)
def ring_up_run(n_shots=16):
    cfg, progs, f, env, n_clks = dispersive_case(WINDOWS[1])
    out, pairs, iq_d, iq_l = synth_cores(progs, cfg, f, f, (4, 4), (4, 4), env, n_clks, n_shots=n_shots, shot0=500)
    lines = dispersive_lines(pairs)
    tab = ResonatorTable(PT(pairs), dispersive_f_res(pairs['core']), KAPPA)
    adc = resonator_ref.feedline_adc_res(cfg, pairs, lines, tab.coef, tab.adc_sigma, out['summary'], out['events'], iq_d,
                                         iq_l.shape[1], cfg.meas_cap)
    n_bins = 4 * WINDOWS[1]
    tr = traces_ref.feedline_traces(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l, cfg.meas_cap, n_bins)
    pred = predicted_traces(cfg, pairs, lines, tab, out['summary'], out['events'], iq_d, iq_l, n_bins)
    return cfg, pairs, tab, tr, pred


def test_ring_up():
    """dispersive_case's long window (ten time constants) at bin_clocks 1: each (core, state) mean trace follows the
    transient formula c / (1 - q) (1 - q^(k + 1)) d of every member of the line, mixed with the LO bin by bin,
    within LINE_TOL of the trace's peak; it does ring up; and over the last 32 clocks (a whole number of turns of
    every neighbour's tone) the two states' traces differ in angle by what H_1 / H_0 gives, within LINE_TOL rad"""
    cfg, pairs, tab, tr, pred = ring_up_run()
    rt = ReadoutTraces(tr, cfg)
    mean = rt.mean()[0]
    worst = 0.0
    for c in range(3):
        for s_ in (0, 1):
            assert rt.n[0, c, s_].min() >= 2 and (rt.samples[0, c, s_] == 4 * rt.n[0, c, s_]).all()
            peak = np.abs(mean[c, s_]).max()
            dev = np.abs(mean[c, s_] - pred[c, s_]).max() / peak
            worst = max(worst, dev)
            assert dev <= LINE_TOL, (c, s_, dev)
            # the core's own return rings up: whole 32-clock turns of the neighbours' tones averaged away
            blocks = mean[c, s_].reshape(-1, 32).mean(axis=1)
            assert abs(blocks[0]) < 0.35 * abs(blocks[-1]) and abs(abs(blocks[-2]) / abs(blocks[-1]) - 1) < 0.01
        H = []
        for s_ in (0, 1):
            a, k = (complex(*tab.coef[c, s_, q:q + 2]) / 2 ** 30 for q in (0, 2))
            H.append(k / (1 - a * cmath.exp(-2j * math.pi * DISP_F[c] / (2.0 ** 32 * 4))))
        last = [mean[c, s_, -32:].sum() for s_ in (0, 1)]
        got, want = cmath.phase(last[1] / last[0]), cmath.phase(H[1] / H[0])
        assert abs(want) > 1.0 and abs(got - want) <= LINE_TOL, (c, got, want)
    assert np.isnan(mean[3]).all() and not rt.n[0, 3].any()            # the idle core has no readouts
    print('worst |mean trace - transient formula| / peak: {:.3e} (LINE_TOL {})'.format(worst, LINE_TOL))


# ---- 3. the matched-filter loop --------------------------------------------------------------------------------
MF_DRIVE_WORDS = 16                  # a 64-clock drive pulse, one amplitude time constant ...
MF_LO_WORDS = 64                     # ... in a 256-clock LO window: ring-up, three time constants of ring-down
MF_CLKS = 300
MF_AMP = 2000                        # drive amplitude word: ~1,000 LSB per member, three members per line
MF_ADC_SIGMA = 4800                  # nu's std 0.577 adc_sigma = 2,770 LSB, its peak 9,600: nothing clips
MF_SHOTS = 512
MF_SEEDS = (0xC0FFEE, 11, 12, 13, 14)


def mf_case(seed):
    """dispersive_case's parts with a drive pulse much shorter than the LO window: the window holds the ring-up,
    the ring-down and then only noise.  ro_sigma = 0; the noise is the converter's (adc_sigma)"""
    cfg, _, f, env, _ = dispersive_case(MF_LO_WORDS, seed=seed)
    read = [dict(A=MF_AMP, ph_d=0, ph_lo=0, L_d=MF_DRIVE_WORDS, L_lo=MF_LO_WORDS, lo_at=DISP_DELAY)]
    progs = [ro_program(read)] * 3 + [[isa.done_cmd()]]
    assert cfg.ro_sigma == 0
    return cfg, progs, f, env[:4 * MF_LO_WORDS], MF_CLKS


def mf_envelope(e):
    """the rdlo envelope buffer of complex samples e (rdlo 4 samples per clock at interp 4: one per clock)"""
    return DDSElementConfig(samples_per_clk=4, interp_ratio=4).get_env_buffer(e)


def fitted_stats(cfg, pairs, acc, res, iq_stats=None):
    """fit on the statistics of (acc, res), measure again with the fitted per-core axes and thresholds:
    (snr [C], discriminator, fidelity over the reading cores, angle of centroid 1 - centroid 0 [C]).
    iq_stats(axis, thr) -> table; default: the reference"""
    core, shot = np.asarray(pairs['core']), np.asarray(pairs['shot'])
    if iq_stats is None:
        def iq_stats(axis, thr):
            return iq_stats_ref.iq_stats(cfg, acc, res[:, 0], core=core, shot=shot, axis=axis, thr=thr)[0]
    rs = ReadoutStats(iq_stats(None, None), cfg)
    d = rs.fit()
    assert d.fitted[:3].all()
    rs2 = ReadoutStats(iq_stats(d.axis_words, d.thr), cfg, axis=d.axis_words, thr=d.thr)
    conf = rs2.confusion[0, :3]
    fid = (int(conf[:, 0, 0].sum()) + int(conf[:, 1, 1].sum())) / int(conf.sum())
    m = rs.mean()[0]
    sep = m[:, 1] - m[:, 0]
    return rs.snr()[0], d, fid, np.arctan2(sep[:, 1], sep[:, 0])


def check_loop(before, after, gains):
    """before / after = fitted_stats of the boxcar run and of the rerun with the matched-filter envelopes,
    gains[c] = ReadoutTraces.predicted_gain(c).  Returns (worst |axis angle|, worst |ratio / gain - 1|).

    Measured on the numpy reference over MF_SEEDS at MF_SHOTS shots: boxcar SNR 2.88 .. 3.32, after the filter
    3.98 .. 4.68; predicted gains 1.40 .. 1.50; the centroid separation within 4.11e-6 rad of +I (the fitted axis
    word is exactly +I: its Q half rounds to 0); |measured ratio / predicted gain - 1| at most 6.74e-2; fidelity
    0.930 .. 0.941 before, 0.982 .. 0.988 after.  AXIS_TOL and GAIN_TOL are twice the worst seen.

    The filter is taken from the shots it is then applied to, as in the issue's loop: the part of the mean
    traces that is noise is fitted too, which raises SNR^2 after the filter by about 2 n_bins (1 / n_0 + 1 / n_1)
    = 4 of about 19 here (ten per cent of the SNR) -- in the measured ratio and, through the same noisy Delta, in
    predicted_gain alike.  The shot count and the window are chosen to keep that part small: at 128 shots and a
    640-clock window the same loop "predicts" and "measures" gains of 7 to 10 that are all fitted noise."""
    snr0, _, fid0, _ = before
    snr1, d1, fid1, angle = after
    worst_axis = worst_ratio = 0.0
    for c in range(3):
        assert np.isfinite(snr0[c]) and np.isfinite(snr1[c]) and snr1[c] > snr0[c] > 0, (c, snr0[c], snr1[c])
        a_i, a_q = axis_halves(d1.axis_words[c])
        # the centroid separation itself, and the axis word fitted to it (the angle rounded to 1 / 32767 rad)
        worst_axis = max(worst_axis, abs(float(angle[c])), abs(math.atan2(a_q, a_i)))
        worst_ratio = max(worst_ratio, abs(snr1[c] / snr0[c] / gains[c] - 1))
        assert gains[c] >= 1.0
    assert fid0 < 1.0 and fid1 >= fid0, (fid0, fid1)
    return worst_axis, worst_ratio


AXIS_TOL = 8.3e-6
GAIN_TOL = 0.135


def resynth_lo(cfg, out, pairs, f_lo, envs, n_clks):
    """the LO rows again, core c's channel with the envelope table envs[c] (rdlo 4 / 4)"""
    C_ = cfg.cores_per_shot
    offs = np.concatenate([[0], np.cumsum([len(e) for e in envs])])
    fbs = [freq_buffer(int(f_lo[c]), 4) for c in range(C_)]
    desc = [(int(lane), RDLO, 4, 4, int(offs[c]), len(envs[c]), 16 * c, 16)
            for lane, c in zip(pairs['lane'], pairs['core'])]
    return oracle.dds(desc, out['summary'], out['events'], np.concatenate(envs), np.concatenate(fbs), n_clks * 4,
                      cfg.event_cap)


def mf_loop_ref(seed, n_shots=MF_SHOTS):
    """the whole loop on the numpy reference: (before, after, gains, ReadoutTraces)"""
    cfg, progs, f, env, n_clks = mf_case(seed)
    out, pairs, iq_d, iq_l = synth_cores(progs, cfg, f, f, (4, 4), (4, 4), env, n_clks, n_shots=n_shots, shot0=500)
    lines = dispersive_lines(pairs)
    tab = ResonatorTable(PT(pairs), dispersive_f_res(pairs['core']), KAPPA, adc_sigma=MF_ADC_SIGMA / 65536.0)
    assert tab.adc_sigma == MF_ADC_SIGMA
    adc = resonator_ref.feedline_adc_res(cfg, pairs, lines, tab.coef, tab.adc_sigma, out['summary'], out['events'], iq_d,
                                         iq_l.shape[1], cfg.meas_cap)
    assert max(np.abs(s16(adc)).max(), np.abs(s16(adc >> 16)).max()) < 32767          # nothing clips
    n_bins = 4 * MF_LO_WORDS
    tr = traces_ref.feedline_traces(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l, cfg.meas_cap, n_bins)
    rt = ReadoutTraces(tr, cfg)
    acc, res = feedline_ref.demod_feedline(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l, cfg.meas_cap)
    before = fitted_stats(cfg, pairs, acc, res)
    envs = [mf_envelope(rt.matched_filter(c)) for c in range(3)] + [env]
    assert all(len(e) == n_bins for e in envs[:3])
    iq_l2 = resynth_lo(cfg, out, pairs, f, envs, n_clks)
    acc2, res2 = feedline_ref.demod_feedline(cfg, pairs, lines, out['summary'], out['events'], adc, iq_l2, cfg.meas_cap)
    after = fitted_stats(cfg, pairs, acc2, res2)
    return before, after, [rt.predicted_gain(c) for c in range(3)], rt


@pytest.mark.parametrize('seed', MF_SEEDS)
def test_matched_filter_loop(seed):
    """traces with a square LO -> matched_filter per core -> the rdlo envelopes -> DDS -> the same ADC traces ->
    demod_feedline -> iq_stats -> fit: the fitted axis is +I, every reading core's SNR rises by the ratio the
    traces predict, and the fidelity does not fall (figures and tolerances: check_loop)"""
    before, after, gains, rt = mf_loop_ref(seed)
    worst_axis, worst_ratio = check_loop(before, after, gains)
    print('seed {:#x}: snr {} -> {}, predicted gains {}, fidelity {:.4f} -> {:.4f}, axis {:.2e} rad, ratio dev {:.3e}'
          .format(seed, np.round(before[0][:3], 3), np.round(after[0][:3], 3), np.round(gains, 3), before[2],
                  after[2], worst_axis, worst_ratio))
    assert before[2] < 1.0 and all(np.isfinite(before[0][:3]))
    assert worst_axis <= AXIS_TOL and worst_ratio <= GAIN_TOL
    # the window holds the ring-up and the ring-down: the filter (noisy, bin by bin) peaks around the drive's end at
    # clock 64 and weighs the first half of the window more than the second
    for c in range(3):
        e = np.abs(rt.matched_filter(c))
        assert abs(e.max() - 1.0) < 1e-12 and 32 <= int(e.argmax()) < 128 and e[:128].sum() > e[128:].sum()


# ---- 4. ReadoutTraces ------------------------------------------------------------------------------------------
def table_of(means, counts, spb=4):
    """a [S, C = 1, 2, n_bins, 4] table with the given complex mean traces [S, 2, n_bins] (integer parts) and
    readout counts [S, 2]"""
    means, counts = np.asarray(means), np.asarray(counts)
    S, _, n_bins = means.shape
    t = np.zeros((S, 1, 2, n_bins, 4), np.int64)
    for s_ in range(S):
        for st in (0, 1):
            n = int(counts[s_, st])
            t[s_, 0, st, :, 0], t[s_, 0, st, :, 1] = n, n * spb
            t[s_, 0, st, :, 2] = np.real(means[s_, st]).astype(np.int64) * n * spb
            t[s_, 0, st, :, 3] = np.imag(means[s_, st]).astype(np.int64) * n * spb
    return t


def test_readout_traces_unit():
    cfg = fl_cfg(1)
    m = np.array([[[100 + 10j, 200 - 20j, 300 + 0j], [500 + 50j, 100 - 20j, 300 + 40j]],
                  [[-100 + 0j, 0 + 0j, 60 + 60j], [900 - 30j, 40 + 0j, 60 - 60j]]])
    t = table_of(m, [[2, 3], [10, 1]])
    rt = ReadoutTraces(t, cfg, by_slot=True)
    assert rt.n.shape == rt.samples.shape == (2, 1, 2, 3) and (rt.samples == 4 * rt.n).all()
    np.testing.assert_array_equal(rt.sums[0], t[..., 2])
    np.testing.assert_allclose(rt.mean()[:, 0], m)
    np.testing.assert_allclose(rt.difference(0, slot=1), m[1, 1] - m[1, 0])
    # pooling over slots is by sums, not by means: weights 2 : 10 and 3 : 1
    pooled = (3 * m[0, 1] + 1 * m[1, 1]) / 4 - (2 * m[0, 0] + 10 * m[1, 0]) / 12
    np.testing.assert_allclose(rt.difference(0), pooled)
    assert not np.allclose(pooled, (m[0, 1] + m[1, 1]) / 2 - (m[0, 0] + m[1, 0]) / 2)
    e = rt.matched_filter(0)
    np.testing.assert_allclose(e, pooled / np.abs(pooled).max())
    assert abs(np.abs(e).max() - 1.0) < 1e-12
    # an empty bin: nan in the mean, 0 in the filter, left out of the gain
    t2 = t.copy()
    t2[:, 0, 1, 1] = 0
    rt2 = ReadoutTraces(t2, cfg, by_slot=True)
    assert np.isnan(rt2.mean()[:, 0, 1, 1]).all() and not np.isnan(rt2.mean()[:, 0, 0]).any()
    assert np.isnan(rt2.difference(0)[1]) and rt2.matched_filter(0)[1] == 0 and rt2.matched_filter(0)[0] != 0
    d = pooled[[0, 2]]
    assert abs(rt2.predicted_gain(0) - math.sqrt(2 * (np.abs(d) ** 2).sum()) / abs(d.sum())) < 1e-12
    # the ValueError cases: a state without readouts, identical traces
    t3 = t.copy()
    t3[:, 0, 0] = 0
    for call in (ReadoutTraces(t3, cfg, by_slot=True).matched_filter, ReadoutTraces(t3, cfg, by_slot=True).predicted_gain):
        with pytest.raises(ValueError, match='state 0'):
            call(0)
    same = table_of([[m[0, 0], m[0, 0]]], [[2, 3]])
    with pytest.raises(ValueError, match='do not differ'):
        ReadoutTraces(same, cfg).matched_filter(0)
    # a constant difference: the boxcar is the matched filter, the gain is 1
    const = table_of([[m[0, 0], m[0, 0] + (30 - 40j)]], [[5, 7]])
    rc = ReadoutTraces(const, cfg)
    assert rc.predicted_gain(0) == pytest.approx(1.0, abs=1e-12)
    np.testing.assert_allclose(rc.matched_filter(0), np.full(3, (30 - 40j) / 50))
    assert ReadoutTraces(t, cfg, by_slot=True).predicted_gain(0) > 1.0
    # the constructor's checks
    for bad, kw in ((t, {}), (t.astype(np.int32), dict(by_slot=True)), (t[:, :, :1], dict(by_slot=True)),
                    (t[..., :3], dict(by_slot=True)), (t, dict(by_slot=True, bin_clocks=0))):
        with pytest.raises(ValueError):
            ReadoutTraces(bad, cfg, **kw)
    with pytest.raises(ValueError, match='core'):
        rt.difference(1)
    with pytest.raises(ValueError, match='slot'):
        rt.difference(0, slot=2)


# ---- 5. the inputs of tests/test_gpu_traces.py reach what they are for --------------------------------------------
EXACT_BINS = 250                     # n_bins of the exact cases, at bin_clocks 1 and 3
EXACT_CLKS = 1204
HB_TRACE_CASES = ('scan_16_4', 'scan_1_1', 'full_range_oct01', 'clamp', 'edge_four_samples')


def exact_lines(n_shots):
    return [ln for s_ in range(n_shots) for ln in ([4 * s_ + 2, 4 * s_, 4 * s_ + 1], [4 * s_ + 3])]


def hb_trace_inputs(name):
    """(case, adc trace, n_bins, bin_clocks) of a hand-built case: the caller-made trace where the case has one"""
    c = hb.case(name)
    adc = c.adc_in if c.adc_in is not None else hb.reference(name)['adc_res']
    return c, adc, {'clamp': 4096}.get(name, 300), {'clamp': 8}.get(name, 1)


def hb_trace_reference(name, by_slot):
    c, adc, n_bins, bin_clocks = hb_trace_inputs(name)
    return traces_ref.feedline_traces(c.cfg, c.pt.cols, c.lines, c.summary, c.events, adc, c.iq_lo, c.cfg.meas_cap,
                                      n_bins, bin_clocks, by_slot=by_slot)


def coverage(cfg, pairs, summary, events, n_lo, n_bins, bin_clocks, traces):
    """what a by_slot = 0 input set reaches, from the kept readouts and the reference's table"""
    summary, events = np.asarray(summary).view(np.uint32), np.asarray(events).view(np.uint32)
    got = set()
    for i in range(len(pairs['lane'])):
        lane, spc_l = int(pairs['lane'][i]), int(pairs['spc_lo'][i])
        reads = feedline_ref.kept_readouts(cfg, summary, events, lane, cfg.meas_cap, cfg.event_cap)
        all_reads = feedline_ref.kept_readouts(cfg, summary, events, lane, 1 << 20, cfg.event_cap)
        if len(all_reads) > cfg.meas_cap:
            got.add('more readouts than meas_cap')
        if not reads:
            got.add('pair without readouts')
        for t_lo, pe in reads:
            clks = ((pe >> 12) & 0xFFF or 4096) * cfg.ro_cpw
            if t_lo * spc_l < n_lo:
                if clks > n_bins * bin_clocks and (t_lo + n_bins * bin_clocks) * spc_l < n_lo:
                    got.add('samples dropped')
                if clks <= (n_bins - 1) * bin_clocks:
                    got.add('window ends before the last bin')
                if (t_lo + clks) * spc_l > n_lo:
                    got.add('clipped by n_samples_lo')
                if (t_lo * spc_l) % 4:
                    got.add('unaligned window start')
    n0 = traces[0, :, :, :, 0]
    if (n0[:, :, -1] < n0[:, :, 0]).any():
        got.add('word 0 below the readout count in the last bin')
    reading = n0[:, :, 0].sum(axis=1) > 0
    if reading.any() and (n0[reading][:, :, 0] > 0).all():
        got.add('both states in every reading core')
    return got


@functools.lru_cache(maxsize=None)
def exact_inputs_cpu(spc, lane_order):
    """test_gpu_traces' exact case on the CPU models (oracle.fast_run, oracle.dds, resonator_ref)"""
    from tests.test_gpu_feedline import exact_case
    from tests.test_gpu_resonator import random_table
    ps, cfg = exact_case(spc, lane_order, 7200 + 16 * spc[0] + spc[1])
    out = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, 1000, 3, want=('summary', 'events'),
                          ro=ps.readout_freqs(RDRV, RDLO))
    who = [(1000 + s_, c) for s_ in range(3) for c in range(4)]
    params = {RDRV: (spc[0], spc[0]), RDLO: (spc[1], spc[1])}
    drv = ChannelPlan(ps, cfg, 1000, 3, [(s_, c, RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, 1000, 3, [(s_, c, RDLO) for s_, c in who], params)
    iq_d = oracle.dds(drv.desc, out['summary'], out['events'], drv.env, drv.freq, EXACT_CLKS * spc[0], cfg.event_cap)
    iq_l = oracle.dds(lo.desc, out['summary'], out['events'], lo.env, lo.freq, EXACT_CLKS * spc[1], cfg.event_cap)
    pt = DemodPairTable(cfg, drv, lo)
    tab = random_table(pt, 87 + spc[0])
    lines = exact_lines(3)
    adc = resonator_ref.feedline_adc_res(cfg, pt.cols, lines, tab.coef, tab.adc_sigma, out['summary'], out['events'],
                                         iq_d, iq_l.shape[1], cfg.meas_cap)
    return cfg, pt, lines, out, adc, iq_l


@pytest.mark.parametrize('spc', [(16, 4), (1, 1)], ids=['16_4', '1_1'])
def test_exact_case_coverage(spc):
    """the exact case reaches: dropped samples, windows that end before the last bin (word 0 below the class's
    readout count there), a window clipped by n_samples_lo, a lane with more readouts than meas_cap, both states
    in every reading core's class, and at 1:1 window starts that are no multiple of 4"""
    for lane_order in (_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR):
        cfg, pt, lines, out, adc, iq_l = exact_inputs_cpu(spc, lane_order)
        for bin_clocks in (1, 3):
            tr = traces_ref.feedline_traces(cfg, pt.cols, lines, out['summary'], out['events'], adc, iq_l,
                                            cfg.meas_cap, EXACT_BINS, bin_clocks)
            got = coverage(cfg, pt.cols, out['summary'], out['events'], iq_l.shape[1], EXACT_BINS, bin_clocks, tr)
            want = {'samples dropped', 'window ends before the last bin', 'clipped by n_samples_lo',
                    'more readouts than meas_cap', 'word 0 below the readout count in the last bin',
                    'both states in every reading core'} | ({'unaligned window start'} if spc[1] == 1 else set())
            assert want <= got, (lane_order, bin_clocks, want - got)
            assert tr[..., 1].sum() > 0 and (tr[..., 0] <= tr[..., 1]).all()


def test_handbuilt_case_coverage():
    """the hand-built cases add: a pair without readouts and 32 slots (scan), a product P_I = 2^31 (full range: LO
    row 0x80008000 under a caller's ADC row 0x80008000), a 4,096-word window of 32,768 samples in bins of 8 clocks
    (clamp), and rows of four samples"""
    scan = hb.case('scan_1_1')
    tr = hb_trace_reference('scan_1_1', False)
    got = coverage(scan.cfg, scan.pt.cols, scan.summary, scan.events, scan.n_lo, 300, 1, tr)
    assert {'pair without readouts', 'unaligned window start', 'window ends before the last bin'} <= got
    assert hb_trace_reference('scan_16_4', True).shape[0] == 32
    c, adc, n_bins, _ = hb_trace_inputs('full_range_oct01')
    assert adc is c.adc_in
    p = 3
    lo = c.iq_lo[int(c.pt.cols['lo_row'][p])]
    a = adc[[l for l, ln in enumerate(c.lines) if p in ln][0]]
    assert (lo == 0x80008000).all() and (a == 0x80008000).all()
    j0, j1 = c.windows(p)[0]
    P_i = s16(a[j0:j1]) * s16(lo[j0:j1]) + s16(a[j0:j1] >> 16) * s16(lo[j0:j1] >> 16)
    assert j1 > j0 and (P_i == 2 ** 31).all()
    tr = hb_trace_reference('full_range_oct01', True)
    core, st = int(c.pt.cols['core'][p]), feedline_ref.state(c.cfg, int(c.pt.cols['shot'][p]), int(c.pt.cols['core'][p]), 0)
    others = [q for q in range(c.pt.n_pairs) if q != p and int(c.pt.cols['core'][q]) == core and c.reads(q)
              and feedline_ref.state(c.cfg, int(c.pt.cols['shot'][q]), core, 0) == st]
    if not others:                                           # pair 3 alone in its slot-0 class: 4 samples of 2^31 per bin
        assert tr[0, core, st, 0, 2] == 4 * 2 ** 31
    got = coverage(c.cfg, c.pt.cols, c.summary, c.events, c.n_lo, n_bins, 1, hb_trace_reference('full_range_oct01', False))
    assert 'clipped by n_samples_lo' in got
    tr = hb_trace_reference('clamp', False)
    assert tr[..., 2].max() == 8 * 2 ** 31 and tr[..., 1].max() == 8 and tr[..., 1].sum() == 4 * 32768
    assert hb.case('edge_four_samples').n_lo == 4 and hb_trace_reference('edge_four_samples', False)[..., 1].sum() > 0


# ---- the host-side checks ------------------------------------------------------------------------------------
def test_check_trace_tensors():
    """stage_tensors.check_trace_tensors: the bins, the int64 sums' bound and the traces tensor's shape, before the C
    ABI sees a pointer; _abi.TraceBins mirrors dpemu_trace_bins (three uint32)"""
    import ctypes
    import torch
    from distributed_processor_amd._native import DpemuError
    from distributed_processor_amd.stage_tensors import check_trace_tensors
    from tests.test_output_checks import _dev
    assert ctypes.sizeof(_abi.TraceBins) == 12
    assert [f for f, _ in _abi.TraceBins._fields_] == ['n_bins', 'bin_clocks', 'by_slot']
    assert (_abi.TRACE_WORDS, _abi.TRACE_BINS_MAX) == (traces_ref.TRACE_WORDS, traces_ref.BINS_MAX) == (4, 4096)
    c = hb.case('edge_four_samples')
    cfg = c.cfg

    def z(shape, dtype=torch.int32):
        return _dev(torch.zeros(shape, dtype=dtype))
    out = {'summary': z(c.summary.shape), 'events': z(c.events.shape)}
    iq_l, adc = z(c.iq_lo.shape), z((len(c.lines), c.n_lo))
    tr = z((cfg.meas_cap, 4, 2, 10, 4), torch.int64)
    assert check_trace_tensors(c.ft, cfg, out, 0, iq_l, adc, 10, 3, True, tr) is tr
    assert check_trace_tensors(c.ft, cfg, out, 0, iq_l, adc, 4096, 1, False) is None
    top = 2 ** 31 // (c.pt.n_pairs * cfg.meas_cap * 16)
    assert traces_ref.check_bound(c.pt.n_pairs, cfg.meas_cap, top)
    assert not traces_ref.check_bound(c.pt.n_pairs, cfg.meas_cap, top + 1)
    check_trace_tensors(c.ft, cfg, out, 0, iq_l, adc, 10, top, False)
    for kw, word in ((dict(n_bins=0), 'n_bins'), (dict(n_bins=4097), 'n_bins'), (dict(bin_clocks=0), 'bin_clocks'),
                     (dict(bin_clocks=top + 1), '2\\^31'), (dict(by_slot=False), 'traces'), (dict(n_bins=11), 'traces'),
                     (dict(adc=None), 'adc'), (dict(iq_lo=None), 'iq_lo'), (dict(adc=z((1, c.n_lo))), 'adc')):
        a = dict(iq_lo=iq_l, adc=adc, n_bins=10, bin_clocks=3, by_slot=True)
        a.update(kw)
        with pytest.raises(DpemuError, match=word):
            check_trace_tensors(c.ft, cfg, out, 0, a['iq_lo'], a['adc'], a['n_bins'], a['bin_clocks'], a['by_slot'], tr)
