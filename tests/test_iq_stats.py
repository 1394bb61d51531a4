"""Readout statistics and discriminator fit on the CPU (dpemu_iq_stats'
specification, tests/iq_stats_ref.py, and distributed_processor_amd/readout.py):
the reference's state labels against the oracle's Philox, the limb
reconstruction of the second moments, the fit on noise-free and noisy
centroids, Discriminator.apply, and the reference's outcome bits against a
DEMOD run of oracle_fast.  The GPU kernel is held to the same reference bit
for bit in tests/test_gpu_iq_stats.py."""

import math
import random

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, workloads
from distributed_processor_amd.emulator import ProgramSet
from distributed_processor_amd.readout import Discriminator, ReadoutStats, axis_halves
from tests import demod_iq_ref, iq_stats_ref

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def test_state_labels_equal_the_oracles_draw():
    """philox_word0 is demod_iq_ref.philox4's word 0 and the oracle's draw, and
    states() is draw < thr (always 1 at 0xFFFFFFFF) -- shots beyond 2^32 included"""
    rng = random.Random(11)
    thrs = [0, 0xFFFFFFFF, 1 << 31, rng.getrandbits(32)]
    cfg = _abi.make_config(4, seed=0xC0FFEE1234567)
    for c, t in enumerate(thrs):
        cfg.p1_threshold[c] = t
    shots = [0, 1, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 7, 2 ** 63 + 5, 2 ** 64 - 1] + [rng.getrandbits(64) for _ in range(60)] \
        + [rng.getrandbits(20) for _ in range(40)]
    trip = [(s_, rng.randrange(4), rng.randrange(32)) for s_ in shots for _ in range(3)]
    assert len(trip) > 300
    shot = np.array([t[0] for t in trip], np.uint64)
    core = np.array([t[1] for t in trip], np.uint32)
    m = np.array([t[2] for t in trip], np.uint32)
    w0 = iq_stats_ref.philox_word0(cfg.seed, shot, core, m)
    st = iq_stats_ref.states(cfg, shot, core, m)
    L = oracle.lib()
    for k, (s_, c, mm) in enumerate(trip):
        draw = L.oracle_philox_u32(cfg.seed, s_, c, mm)
        assert int(w0[k]) == draw == demod_iq_ref.philox4(cfg.seed, s_, c, mm)[0]
        assert int(st[k]) == int(thrs[c] == 0xFFFFFFFF or draw < thrs[c])
    assert not st[core == 0].any() and st[core == 1].all() and 0 < st[core == 2].mean() < 1


def test_limb_reconstruction_is_exact():
    """sum I^2, sum Q^2, sum I Q rebuilt from the table's limb sums equal the
    direct Python-integer sums, int32 extremes included"""
    rng = np.random.default_rng(5)
    n, cap = 400, 3
    acc = rng.integers(INT32_MIN, INT32_MAX, size=(cap, n, 2), endpoint=True).astype(np.int32)
    ext = [INT32_MIN, INT32_MAX, -1, 0]
    for k, (a, b) in enumerate((a, b) for a in ext for b in ext):
        acc[k % cap, k, :] = (a, b)
    cfg = _abi.make_config(1, p1=1.0, seed=3)
    table, _ = iq_stats_ref.iq_stats(cfg, acc, np.full(n, cap))
    rs = ReadoutStats(table, cfg)
    ii, qq, iq = rs.second_moments()
    I = [int(v) for v in acc[..., 0].ravel()]
    Q = [int(v) for v in acc[..., 1].ravel()]
    assert rs.n[0, 0].tolist() == [0, cap * n]
    assert int(rs.sum_i[0, 0, 1]) == sum(I) and int(rs.sum_q[0, 0, 1]) == sum(Q)
    assert ii[0, 0, 1] == sum(v * v for v in I)
    assert qq[0, 0, 1] == sum(v * v for v in Q)
    assert iq[0, 0, 1] == sum(a * b for a, b in zip(I, Q))
    assert ii[0, 0, 1] > 2 ** 63                                 # beyond int64: why the limbs are there
    assert not table[..., 13:].any()
    # and the floats follow: mean and covariance against numpy on the same data
    np.testing.assert_allclose(rs.mean()[0, 0, 1], [np.mean(I), np.mean(Q)], rtol=1e-12, atol=1e-3)
    np.testing.assert_allclose(rs.cov()[0, 0, 1], np.cov(np.array([I, Q], float), bias=True), rtol=1e-9)


def centroid_acc(cfg, cent, n_shots, cap, noise_sigma=0):
    """acc (cap, n_shots * C, 2) of the run layout: cent[core][state] (+ the
    DEMOD model's own noise draw of the readout), every column with `cap` readouts"""
    C_ = cfg.cores_per_shot
    core, shot = iq_stats_ref.run_columns(cfg, n_shots * C_)
    acc = np.zeros((cap, n_shots * C_, 2), np.int32)
    for m in range(cap):
        st = iq_stats_ref.states(cfg, shot, core, m)
        for col in range(n_shots * C_):
            z = demod_iq_ref.noise(cfg.seed, int(shot[col]), int(core[col]), m, noise_sigma)[1:] if noise_sigma else (0, 0)
            c = cent[int(core[col])][int(st[col])]
            acc[m, col] = (c[0] + z[0], c[1] + z[1])
    return acc


def polar(r, phi):
    return np.array([r * math.cos(phi), r * math.sin(phi)])


@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR])
def test_noise_free_fit(lane_order):
    """two exact centroids per core: an axis perpendicular to the separation
    gives every readout one outcome (fidelity = that state's share); the fitted
    discriminator assigns every readout right.  Core 2 has unequal gains at
    one phase -- both centroids on one side of the origin -- so its fitted
    threshold is far from zero and fidelity 1.0 needs it.  Core 3 has
    coincident centroids: not fitted."""
    phis = [0.3, 2.5, -1.2, 0.9]
    cent = []
    for c, phi in enumerate(phis):
        u, perp = polar(1.0, phi), polar(1.0, phi + math.pi / 2)
        if c == 2:
            pts = (3.0e6 * u, 1.0e7 * u)                        # gains 0.3 / 1.0, theta equal
        elif c == 3:
            pts = (5.0e6 * u, 5.0e6 * u)
        else:
            pts = (4.0e6 * perp - 6.0e6 * u, 4.0e6 * perp + 6.0e6 * u)
        cent.append([tuple(int(round(v)) for v in p) for p in pts])
    cfg = _abi.make_config(4, p1=0.5, seed=77, lane_order=lane_order, meas_cap=2,
                           demod=dict(drv_elem=1, axis=[p + math.pi / 2 for p in phis], thr=0))
    n_shots, cap = 150, 2
    acc = centroid_acc(cfg, cent, n_shots, cap)
    counts = np.full(n_shots * 4, cap)
    table, bits = iq_stats_ref.iq_stats(cfg, acc, counts)
    rs = ReadoutStats(table, cfg)
    assert rs.n.sum() == n_shots * 4 * cap and rs.n.min() > 100
    for c in (0, 1):                                            # perpendicular axis: one outcome for all
        conf = rs.confusion[0, c]
        assert not conf[:, 0].any() and conf[:, 1].sum() == n_shots * cap
        assert rs.fidelity(core=c) == conf[1, 1] / (n_shots * cap)
        assert 0.3 < rs.fidelity(core=c) < 0.7
    d = rs.fit()
    assert d.fitted.tolist() == [True, True, True, False]
    assert d.axis_words[3] == cfg.ro_axis[3] and d.thr[3] == 0
    for c in range(3):
        a_i, a_q = axis_halves(d.axis_words[c])
        assert abs(math.remainder(math.atan2(a_q, a_i) - phis[c], 2 * math.pi)) < 1e-4
    assert abs(d.thr[0]) < 100 and abs(d.thr[1]) < 100
    assert 6.4e6 < d.thr[2] < 6.6e6                             # the midpoint of 3e6 and 1e7 along the axis
    t2, b2 = iq_stats_ref.iq_stats(cfg, acc, counts, axis=d.axis_words, thr=d.thr)
    r2 = ReadoutStats(t2, cfg, axis=d.axis_words, thr=d.thr)
    for c in range(3):
        assert r2.fidelity(core=c) == 1.0
    # the unequal-gain core: the fitted axis alone (threshold 0) calls every readout 1
    thr0 = d.thr.copy()
    thr0[2] = 0
    r3 = ReadoutStats(iq_stats_ref.iq_stats(cfg, acc, counts, axis=d.axis_words, thr=thr0)[0], cfg)
    assert r3.fidelity(core=2) == rs.n[0, 2, 1] / (n_shots * cap) < 0.7
    assert math.isinf(r2.snr()[0, 0]) and math.isnan(r2.snr()[0, 3])
    # by_slot: the classes split by slot and add up to the table above
    ts, bs = iq_stats_ref.iq_stats(cfg, acc, counts, by_slot=True, axis=d.axis_words, thr=d.thr)
    assert ts.shape[0] == cap and np.array_equal(ts.sum(axis=0), t2[0]) and np.array_equal(bs, b2)
    assert ReadoutStats(ts, cfg, by_slot=True).fidelity(slot=1, core=0) == 1.0


def test_noisy_fit():
    """centroids + the DEMOD model's noise, |d| = 20 sigma, >= 2000 readouts per
    class: the fitted angle is within five standard errors of the centroid
    difference, 5 sigma sqrt(1 / n0 + 1 / n1) / |d|, of the true one, and the
    fitted discriminator's fidelity is at least the true one's on the same draws"""
    sigma_q16 = 40 << 16
    sigma = sigma_q16 / 2 ** 16 * 37837.6                        # dpemu.h ro_sigma
    phis = [1.1, -2.7]
    cent = [[tuple(int(round(v)) for v in polar(2.0e6, p + 1.0) + s_ * polar(10 * sigma, p)) for s_ in (-1, 1)]
            for p in phis]
    cfg = _abi.make_config(2, p1=0.5, seed=0xABCDEF, meas_cap=3, demod=dict(drv_elem=1, axis=0.0, thr=0))
    n_shots, cap = 1500, 3
    acc = centroid_acc(cfg, cent, n_shots, cap, noise_sigma=sigma_q16)
    counts = np.full(2 * n_shots, cap)
    rs = ReadoutStats(iq_stats_ref.iq_stats(cfg, acc, counts)[0], cfg)
    assert rs.n.min() >= 2000
    d = rs.fit()
    assert d.fitted.all()
    for c, phi in enumerate(phis):
        n0, n1 = int(rs.n[0, c, 0]), int(rs.n[0, c, 1])
        a_i, a_q = axis_halves(d.axis_words[c])
        err = abs(math.remainder(math.atan2(a_q, a_i) - phi, 2 * math.pi))
        bound = 5 * sigma * math.sqrt(1 / n0 + 1 / n1) / (20 * sigma)
        print('core', c, 'angle error', err, 'bound', bound)
        assert err <= bound
        # the measured noise is the model's: sigma per quadrature
        np.testing.assert_allclose(np.sqrt(np.diag(rs.cov()[0, c, 0])), [sigma, sigma], rtol=0.1)
        assert 17 < rs.snr()[0, c] < 23
    true_axis = [_abi.axis_word(p) for p in phis]
    true_thr = []
    for c in range(2):
        a_i, a_q = axis_halves(true_axis[c])
        mid = [(cent[c][0][k] + cent[c][1][k]) for k in (0, 1)]
        true_thr.append((mid[0] * a_i + mid[1] * a_q) // (2 << 15))
    f_true = ReadoutStats(iq_stats_ref.iq_stats(cfg, acc, counts, axis=true_axis, thr=true_thr)[0], cfg)
    f_fit = ReadoutStats(iq_stats_ref.iq_stats(cfg, acc, counts, axis=d.axis_words, thr=d.thr)[0], cfg)
    for c in range(2):
        print('core', c, 'fidelity fitted', f_fit.fidelity(core=c), 'true', f_true.fidelity(core=c))
        assert f_fit.fidelity(core=c) >= f_true.fidelity(core=c) > 0.99


def test_apply():
    cfg = _abi.make_config(4, demod=dict(drv_elem=1, axis=[0.1, 0.2, 0.3, 0.4], thr=17))
    before = [cfg.ro_axis[c] for c in range(4)]
    words = [_abi.axis_word(a) for a in (1.0, 2.0, 3.0, -1.0)]
    d = Discriminator(words, [100, 131, 10 ** 9, 90], [True, True, False, True])
    with pytest.raises(ValueError) as e:
        d.apply(cfg, tol=40)                                    # 131 - 90 = 41
    assert 'core 1: 131' in str(e.value) and 'core 3: 90' in str(e.value) and 'core 2' not in str(e.value)
    assert [cfg.ro_axis[c] for c in range(4)] == before and cfg.ro_thr == 17      # untouched
    assert d.apply(cfg, tol=41) is cfg
    assert cfg.ro_thr == (90 + 131) // 2
    assert [cfg.ro_axis[c] for c in range(4)] == [words[0], words[1], before[2], words[3]]
    # negative thresholds: the floor midpoint; no fitted core: nothing happens
    Discriminator(words[:2], [-8, -3], [True, True]).apply(cfg, tol=5)
    assert cfg.ro_thr == -6
    Discriminator(words, [1, 2, 3, 4], [False] * 4).apply(cfg, tol=0)
    assert cfg.ro_thr == -6


def test_reference_bits_equal_a_demod_run():
    """a DEMOD run of oracle_fast (config 3's active reset, 4 cores): the
    reference's bits with cfg's own axis and threshold are the run's meas_bits,
    and word 1 over all classes is their popcount"""
    ps = ProgramSet(workloads.config3_active_reset(4))
    cfg = _abi.make_config(4, max_cycles=50000, event_cap=16, meas_cap=4, meas_latency=workloads.CONFIG3_DEMOD_LATENCY,
                           demod=workloads.config3_demod(ps))
    n_shots, shot0 = 96, 5000
    out = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, shot0, n_shots,
                          ro=ps.readout_freqs(workloads.RDRV, workloads.RDLO))
    s = _abi.unpack_summary(out['summary'])
    count = np.minimum(s['n_meas'], cfg.meas_cap)
    assert (count == 2).all()
    table, bits = iq_stats_ref.iq_stats(cfg, out['acc'], s['n_meas'], shot_begin=shot0)
    want = s['meas_bits'] & ((1 << count.astype(np.uint64)) - 1).astype(np.uint32)
    np.testing.assert_array_equal(bits, want)
    assert int(table[..., 1].sum()) == sum(bin(int(b)).count('1') for b in want)
    assert int(table[..., 0].sum()) == int(count.sum())
    # the prepared state is the one the run discriminated: the calibrated readout is ~99 % right
    rs = ReadoutStats(table, cfg)
    assert rs.fidelity() > 0.95 and rs.n.min() > 20


# ---- the 32-slot inputs of tests/test_gpu_iq_stats.py reach slot 31 ----------------------------------------------

def test_32_slot_cases_reach_slot_31():
    """from the references alone: an outcome bit 31, class rows of slot 31 in both states, a thread that takes
    several columns, state words that differ from the draws at bit 31 -- and read modulo 16 (the low half in both
    halves of the word) they give another table, so a shift that wraps is seen"""
    from tests import qsim_meas_ref
    from tests.test_gpu_iq_stats import SLOTS32, slots32_case
    for which in SLOTS32:
        cfg, kw, acc, counts, cnt, states = slots32_case(which)
        n = len(cnt)
        assert cfg.meas_cap == 32 == acc.shape[0] and set(cnt.tolist()) == set(range(34))
        assert set(states[[3, 40, 77, 130]].tolist()) == {0, 0xFFFFFFFF, 0x80000000, 0x55555555}
        assert (cnt[[3, 40, 77, 130]] >= 32).all()
        base_t, base_b = iq_stats_ref.iq_stats(cfg, acc, cnt, by_slot=True, **kw)
        assert (base_b >> 31).any() and not (base_b >> 31).all()
        assert (base_t[31, :, :, 0].sum(axis=1) > 0).all() and base_t[31, :, :, 0].sum(axis=0).all() and base_t[31, :, :, 1].any()
        flat_t, flat_b = iq_stats_ref.iq_stats(cfg, acc, cnt, **kw)
        np.testing.assert_array_equal(flat_b, base_b)
        np.testing.assert_array_equal(flat_t[0], base_t.sum(axis=0))
        # row 0 counts its own slot alone
        assert base_t[0, :, :, 0].sum() == (cnt > 0).sum() < np.minimum(cnt, 32).sum() == base_t[..., 0].sum()
        st_t, st_b = qsim_meas_ref.iq_stats_st(states, cfg, acc, cnt, by_slot=True, **kw)
        np.testing.assert_array_equal(st_b, base_b)
        assert all((st_t[m] != base_t[m]).any() for m in (0, 2, 3, 16, 31))
        wrapped = (states & 0xFFFF) | ((states & 0xFFFF) << 16)
        wr_t, _ = qsim_meas_ref.iq_stats_st(wrapped, cfg, acc, cnt, by_slot=True, **kw)
        np.testing.assert_array_equal(wr_t[:16], st_t[:16])
        assert all((wr_t[m] != st_t[m]).any() for m in range(16, 32))
        if 'core' not in kw:
            assert n == cfg.cores_per_shot * SLOTS32[which][2] > 2 * 256        # more columns than two workgroups
