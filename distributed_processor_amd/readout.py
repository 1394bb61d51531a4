"""Readout calibration from accumulated {I, Q}: what a QubiC user does first
with an accumulator buffer -- run calibration shots, find the two centroids of
every core, derive the discriminator axis and threshold.

``Emulator.iq_stats`` (``dpemu_iq_stats``, include/dpemu.h) reduces an
accumulator buffer on the GPU to a small integer table, 16 words per (slot,
core, prepared state) class; :class:`ReadoutStats` reads that table --
confusion matrix, assignment fidelity, exact sums, centroids, covariances,
signal-to-noise ratio -- and :meth:`ReadoutStats.fit` turns it into a
:class:`Discriminator`.  The recipe::

    stats, _ = emu.iq_stats(cfg, out['acc'], out['summary'])
    rs = ReadoutStats(stats.cpu().numpy(), cfg)
    rs.fit().apply(cfg, tol=...)        # then run again with the fitted cfg

Everything up to the floats of ``mean`` / ``cov`` / ``snr`` is exact integer
arithmetic (Python integers where int64 would not do).

The second thing a user does with a readout line is average the demodulated
trace per prepared state, look at the ring-up, and load the difference of the
two mean traces as the rdlo envelope -- the matched filter, which weights every
clock of the accumulation by how much it separates the states.
``Emulator.feedline_traces`` (``dpemu_feedline_traces``) reduces the ADC traces
to per-class, per-bin sums of the baseband product adc conj(lo);
:class:`ReadoutTraces` reads that table.  The recipe::

    tr = emu.feedline_traces(cfg, lines, iq_lo, out, adc, n_bins)   # taken with a square rdlo envelope
    rt = ReadoutTraces(tr.cpu().numpy(), cfg)
    env = DDSElementConfig.get_env_buffer(rt.matched_filter(c))     # per reading core c
    # reassemble core c's program with env as its rdlo envelope, then
    # run, synthesize, feedline_adc, demodulate_feedline, iq_stats, fit again

One bin must be one envelope sample: ``bin_clocks * spc_lo = interp`` of the
rdlo element (the DDS plays one envelope sample per ``interp`` output
samples).  For channel_config's rdlo, 4 samples per clock at interp 4, that is
``bin_clocks`` = 1.

Why the sign is right: the rdlo output becomes carrier e, so the product of
the rerun is P' = adc conj(carrier e) = P conj(e).  With e = Delta / max|Delta|,
Delta the difference of the two states' mean traces, the state separation of
the accumulator becomes sum_b Delta_b conj(e_b) = sum |Delta|^2 / max|Delta|:
real and positive.  After the filter the fitted discriminator axis is +I.  For
white per-sample noise (``adc_sigma``) no other envelope gives a larger ratio
of separation to noise; noise added after the accumulator (``ro_sigma``) does
not see the envelope.
"""

from __future__ import annotations

import math

import numpy as np

from . import _abi

W_N, W_N1, W_SI, W_SQ = 0, 1, 2, 3      # words of a class (include/dpemu.h)
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def axis_halves(word):
    """(axis_I, axis_Q): the int16 halves of a Q15 axis word"""
    w = int(word)
    return ((w & 0xFFFF) ^ 0x8000) - 0x8000, (((w >> 16) & 0xFFFF) ^ 0x8000) - 0x8000


class Discriminator:
    """Per-core discriminator: ``axis_words[c]`` (Q15 cos | sin << 16, as
    dpemu_config.ro_axis), ``thr[c]`` and ``fitted[c]`` -- False where the
    statistics could not place the core (a state without readouts, coincident
    centroids): such a core keeps the axis and threshold the statistics were
    taken with.

    The per-core thresholds apply as they are through
    ``Emulator.iq_stats(axis=d.axis_words, thr=d.thr)`` and its outcome bits.
    A run has ONE threshold for all cores (``dpemu_config.ro_thr``): that is
    the limit of :meth:`apply`."""

    def __init__(self, axis_words, thr, fitted):
        self.axis_words = np.asarray(axis_words, np.uint32)
        self.thr = np.asarray(thr, np.int64)
        self.fitted = np.asarray(fitted, bool)
        if not (self.axis_words.shape == self.thr.shape == self.fitted.shape) or self.thr.ndim != 1:
            raise ValueError('axis_words, thr and fitted must be equally long 1-d sequences')

    def apply(self, cfg, tol):
        """Write the fitted cores' axes into ``cfg.ro_axis`` and set the single
        ``cfg.ro_thr`` to the integer midpoint of the fitted cores' smallest
        and largest threshold.  dpemu_config has one threshold for all cores:
        when the fitted thresholds differ by more than ``tol`` (max - min >
        tol) no single value serves them and this raises ValueError, listing
        the per-core values, without touching cfg.  Unfitted cores are left
        alone; with no fitted core cfg is unchanged.  Returns cfg."""
        cores = [c for c in range(len(self.thr)) if self.fitted[c]]
        if not cores:
            return cfg
        thr = [int(self.thr[c]) for c in cores]
        lo, hi = min(thr), max(thr)
        if hi - lo > tol:
            raise ValueError('the fitted thresholds span {} > tol {}, and dpemu_config.ro_thr is one value for all '
                             'cores: {}'.format(hi - lo, tol, ', '.join('core {}: {}'.format(c, t)
                                                                       for c, t in zip(cores, thr))))
        for c in cores:
            cfg.ro_axis[c] = int(self.axis_words[c])
        cfg.ro_thr = (lo + hi) // 2
        return cfg


class ReadoutStats:
    """The table of ``dpemu_iq_stats``: ``table`` int64 [S, C, 2, 16] (a host
    copy of ``Emulator.iq_stats``'s stats; S = the slots with ``by_slot``, else
    1), ``cfg`` the config it was taken with.  ``axis`` / ``thr``: the per-core
    axis words / thresholds given to ``iq_stats``, when they were (default:
    cfg.ro_axis and cfg.ro_thr) -- what an unfitted core keeps."""

    def __init__(self, table, cfg, by_slot=False, axis=None, thr=None):
        C_ = cfg.cores_per_shot
        t = np.asarray(table)
        if t.dtype != np.int64 or t.ndim != 4 or t.shape[1:] != (C_, 2, _abi.IQ_STAT_WORDS):
            raise ValueError('table must be int64 [S, {}, 2, {}]'.format(C_, _abi.IQ_STAT_WORDS))
        if not by_slot and t.shape[0] != 1:
            raise ValueError('table has {} slots but by_slot is off'.format(t.shape[0]))
        self.table, self.cfg, self.by_slot = t, cfg, bool(by_slot)
        self.n_slots, self.n_cores = t.shape[0], C_
        self.axis_words = np.array([cfg.ro_axis[c] for c in range(C_)] if axis is None else axis, np.uint32)
        self.thr = np.array([cfg.ro_thr] * C_ if thr is None else thr, np.int64)
        if self.axis_words.shape != (C_,) or self.thr.shape != (C_,):
            raise ValueError('axis and thr hold one value per core')

    # ---- counts ----
    @property
    def n(self):
        """readouts per class, int64 [S, C, 2]"""
        return self.table[..., W_N]

    @property
    def confusion(self):
        """int64 [slot, core, prepared state, outcome]"""
        n1 = self.table[..., W_N1]
        return np.stack([self.n - n1, n1], axis=-1)

    def fidelity(self, core=None, slot=None):
        """assignment fidelity (n00 + n11) / n over the chosen core(s) and
        slot(s) (None: all); nan without readouts"""
        c = self.confusion
        c = c[slice(None) if slot is None else [slot]][:, slice(None) if core is None else [core]]
        n = int(c.sum())
        return (int(c[..., 0, 0].sum()) + int(c[..., 1, 1].sum())) / n if n else float('nan')

    # ---- sums ----
    @property
    def sum_i(self):
        """exact sum of I per class, int64 [S, C, 2]"""
        return self.table[..., W_SI]

    @property
    def sum_q(self):
        return self.table[..., W_SQ]

    def second_moments(self):
        """(sum I^2, sum Q^2, sum I Q) per class, object arrays [S, C, 2] of
        Python integers, rebuilt from the 16-bit limb sums of the table:
        sum X^2 = 2^32 sum a^2 + 2^17 sum a b + sum b^2 (X = 65536 a + b)"""
        t = self.table.astype(object)
        ii = (t[..., 4] << 32) + (t[..., 5] << 17) + t[..., 6]
        qq = (t[..., 7] << 32) + (t[..., 8] << 17) + t[..., 9]
        iq = (t[..., 10] << 32) + (t[..., 11] << 16) + t[..., 12]
        return ii, qq, iq

    # ---- floats ----
    def mean(self):
        """centroids, float [S, C, 2, 2] (last axis I, Q); nan for an empty class"""
        n = self.n.astype(float)
        with np.errstate(invalid='ignore', divide='ignore'):
            return np.stack([self.sum_i / n, self.sum_q / n], axis=-1)

    def cov(self):
        """population covariance of {I, Q} per class, float [S, C, 2, 2, 2]:
        (n sum XY - sum X sum Y) / n^2, the numerator in exact integers"""
        ii, qq, iq = self.second_moments()
        n, si, sq = self.n.astype(object), self.sum_i.astype(object), self.sum_q.astype(object)
        out = np.full(self.n.shape + (2, 2), np.nan)
        for idx in np.ndindex(*self.n.shape):
            k = int(n[idx])
            if not k:
                continue
            cii, cqq = k * ii[idx] - si[idx] * si[idx], k * qq[idx] - sq[idx] * sq[idx]
            ciq = k * iq[idx] - si[idx] * sq[idx]
            out[idx] = [[cii / k ** 2, ciq / k ** 2], [ciq / k ** 2, cqq / k ** 2]]
        return out

    def snr(self):
        """|centroid 1 - centroid 0| / sqrt((v0 + v1) / 2) per (slot, core),
        v_s the variance of state s along the separation; float [S, C], nan
        where a class is empty or the centroids coincide, inf without noise"""
        m, cv = self.mean(), self.cov()
        d = m[..., 1, :] - m[..., 0, :]
        dist = np.hypot(d[..., 0], d[..., 1])
        with np.errstate(invalid='ignore', divide='ignore'):
            u = d / dist[..., None]
            v = [np.einsum('...i,...ij,...j->...', u, cv[..., s_, :, :], u) for s_ in (0, 1)]
            return dist / np.sqrt((v[0] + v[1]) / 2)

    # ---- fit ----
    def fit(self):
        """The discriminator that separates every core's two centroids (its
        readouts of all slots together).  Per core, in exact integers:
        d = (sum I1 n0 - sum I0 n1, sum Q1 n0 - sum Q0 n1), the centroid
        difference times n0 n1; axis = _abi.axis_word(atan2(dQ, dI)); the
        threshold is the midpoint of the centroids pushed through the
        discriminator's own arithmetic,
        floor((MI axis_I + MQ axis_Q) / (2 n0 n1 2^15)), MI = sum I0 n1 +
        sum I1 n0 (MQ likewise), clipped to int32.  A core with n0 = 0, n1 =
        0 or d = 0 is not fitted and keeps this table's axis and threshold."""
        axis, thr, fitted = self.axis_words.copy(), self.thr.copy(), np.zeros(self.n_cores, bool)
        for c in range(self.n_cores):
            n0, n1 = (int(self.n[:, c, s_].sum()) for s_ in (0, 1))
            i0, i1 = (sum(int(v) for v in self.sum_i[:, c, s_]) for s_ in (0, 1))
            q0, q1 = (sum(int(v) for v in self.sum_q[:, c, s_]) for s_ in (0, 1))
            d_i, d_q = i1 * n0 - i0 * n1, q1 * n0 - q0 * n1
            if n0 == 0 or n1 == 0 or (d_i == 0 and d_q == 0):
                continue
            word = _abi.axis_word(math.atan2(d_q, d_i))
            a_i, a_q = axis_halves(word)
            m_i, m_q = i0 * n1 + i1 * n0, q0 * n1 + q1 * n0
            t = (m_i * a_i + m_q * a_q) // (2 * n0 * n1 * 2 ** 15)
            axis[c], thr[c], fitted[c] = word, max(INT32_MIN, min(INT32_MAX, t)), True
        return Discriminator(axis, thr, fitted)


T_N, T_SAMPLES, T_SI, T_SQ = 0, 1, 2, 3  # words of a class and bin of dpemu_feedline_traces (include/dpemu.h)


class ReadoutTraces:
    """The table of ``dpemu_feedline_traces``: ``table`` int64 [S, C, 2, n_bins,
    4] (a host copy of ``Emulator.feedline_traces``'s tensor; S = the slots
    with ``by_slot``, else 1), ``cfg`` the config it was taken with,
    ``bin_clocks`` the clocks per bin.  Axis 2 is the prepared state."""

    def __init__(self, table, cfg, bin_clocks=1, by_slot=False):
        C_ = cfg.cores_per_shot
        t = np.asarray(table)
        if t.dtype != np.int64 or t.ndim != 5 or t.shape[1:3] != (C_, 2) or t.shape[4] != _abi.TRACE_WORDS \
                or t.shape[3] < 1:
            raise ValueError('table must be int64 [S, {}, 2, n_bins, {}]'.format(C_, _abi.TRACE_WORDS))
        if not by_slot and t.shape[0] != 1:
            raise ValueError('table has {} slots but by_slot is off'.format(t.shape[0]))
        if int(bin_clocks) < 1:
            raise ValueError('bin_clocks must be >= 1')
        self.table, self.cfg, self.by_slot, self.bin_clocks = t, cfg, bool(by_slot), int(bin_clocks)
        self.n_slots, self.n_cores, self.n_bins = t.shape[0], C_, t.shape[3]

    @property
    def n(self):
        """readouts with at least one sample in the bin, int64 [S, C, 2, n_bins]"""
        return self.table[..., T_N]

    @property
    def samples(self):
        """samples summed per class and bin, int64 [S, C, 2, n_bins]"""
        return self.table[..., T_SAMPLES]

    @property
    def sums(self):
        """(sum P_I, sum P_Q), exact, int64 [S, C, 2, n_bins] each"""
        return self.table[..., T_SI], self.table[..., T_SQ]

    def mean(self):
        """mean baseband sample per class and bin, complex [S, C, 2, n_bins]:
        (w2 + i w3) / w1; nan for an empty bin"""
        w = self.samples.astype(float)
        with np.errstate(invalid='ignore', divide='ignore'):
            return (self.table[..., T_SI] / w) + 1j * (self.table[..., T_SQ] / w)

    def _pooled(self, core, slot):
        """core's words [2, n_bins, 4] of one slot, or of all slots pooled by sums (the bound of
        dpemu_feedline_traces covers the readouts of all slots together: int64 holds the pooled sums)"""
        if not 0 <= int(core) < self.n_cores:
            raise ValueError('core {} not in [0, {})'.format(core, self.n_cores))
        if slot is None:
            return self.table[:, int(core)].sum(axis=0)
        if not 0 <= int(slot) < self.n_slots:
            raise ValueError('slot {} not in [0, {})'.format(slot, self.n_slots))
        return self.table[int(slot), int(core)]

    def difference(self, core, slot=None):
        """mean trace of state 1 minus that of state 0, complex [n_bins]; with
        ``slot`` None all slots are pooled by their sums, not by their means.
        nan where either state has no sample in the bin"""
        t = self._pooled(core, slot)
        w = t[..., T_SAMPLES].astype(float)
        with np.errstate(invalid='ignore', divide='ignore'):
            m = t[..., T_SI] / w + 1j * (t[..., T_SQ] / w)
        return m[1] - m[0]

    def _delta(self, core, slot):
        t = self._pooled(core, slot)
        for s_ in (0, 1):
            if not t[s_, :, T_N].any():
                raise ValueError('core {}: no readouts of prepared state {}'.format(core, s_))
        d = self.difference(core, slot)
        have = ~np.isnan(d)
        d = np.where(have, d, 0.0)
        if not np.abs(d).max() > 0:
            raise ValueError('core {}: the two mean traces do not differ'.format(core))
        return d, have

    def matched_filter(self, core, slot=None):
        """The complex rdlo envelope samples e(b) = Delta(b) / max|Delta|, one
        per bin (|e| <= 1, as DDSElementConfig.get_env_buffer takes them); 0
        where either state has no sample in the bin.  Raises ValueError when a
        state has no readouts or Delta is identically 0: there is no filter
        then, and unlike an unfitted discriminator an envelope cannot be left
        as it was."""
        d, _ = self._delta(core, slot)
        return d / np.abs(d).max()

    def predicted_gain(self, core, slot=None):
        """For white per-sample noise, the predicted ratio of the
        matched-filter SNR to the boxcar (square envelope) SNR over the bins
        that have samples of both states: sqrt(N sum |Delta_b|^2) / |sum
        Delta_b|, >= 1 by Cauchy-Schwarz; inf when the boxcar sum vanishes"""
        d, have = self._delta(core, slot)
        d = d[have]
        tot = abs(d.sum())
        if tot == 0:
            return float('inf')
        return math.sqrt(len(d) * float((np.abs(d) ** 2).sum())) / tot
