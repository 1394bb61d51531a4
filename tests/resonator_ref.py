"""CPU reference of the resonator stage (dpemu_feedline_adc_res, include/dpemu.h;
DESIGN.md §2 "Resonator response"): a numpy restatement of the specification on
tests/feedline_ref.py's helpers, vectorised over all members of all lines in int64
(every intermediate fits: |y| < 2^28, |coefficient| <= 2^30, two products and
the rounding constant stay below 2^60) and looping over the samples.  Not test
code of its own: tests/test_resonator.py validates the specification with it on
the CPU, tests/test_gpu_resonator.py holds the kernel to it bit for bit.

``coef`` is int [n_pairs, 2 states, 4] = pole_re, pole_im, coup_re, coup_im
(Q30); ``pairs`` / ``lines`` are feedline_ref's."""

import numpy as np

from tests.demod_iq_ref import M32, s16
from tests.feedline_ref import _views, kept_readouts, state

HALF = 1 << 29
CORE_ADC = 0x80000000            # the high bit of the noise draws' core word


def philox4_vec(seed, shot, core, m):
    """Philox4x32-10 of demod_iq_ref.philox4 for an array of counters m: (4, len(m)) uint64"""
    m = np.asarray(m, np.uint64)
    c = [np.full(m.shape, v, np.uint64) for v in (shot & M32, (shot >> 32) & M32, core & M32)] + [m & np.uint64(M32)]
    k0, k1 = seed & M32, (seed >> 32) & M32
    lo = np.uint64(M32)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & lo, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & lo]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return np.stack(c)


def adc_noise(seed, shot, core, n_lo, sigma):
    """(nu_I, nu_Q) int64 [n_lo]: the converter noise of a line whose first member is (shot, core)"""
    r = philox4_vec(seed, shot, CORE_ADC | core, np.arange(n_lo)).astype(np.int64)
    u0, u1, u2, u3 = r[1] & 0xFFFF, r[1] >> 16, r[2] & 0xFFFF, r[2] >> 16
    return ((u0 + u1 - u2 - u3) * int(sigma)) >> 16, ((u0 - u1 + u2 - u3) * int(sigma)) >> 16


def member_inputs(cfg, pairs, p, summary, events, iq_drv, n_lo, meas_cap, event_cap):
    """(d_I, d_Q, state) of member p at every LO sample: feedline_ref.feedline_adc's d_p and s_p(n)"""
    n_drv = iq_drv.shape[1]
    j = np.arange(n_lo, dtype=np.int64)
    spc_d, spc_l = int(pairs['spc_drv'][p]), int(pairs['spc_lo'][p])
    lane, core, shot = int(pairs['lane'][p]), int(pairs['core'][p]), int(pairs['shot'][p])
    n, k = j // spc_l, j % spc_l
    di = (n - cfg.ro_delay) * spc_d + k * (spc_d // spc_l)
    ok = (n >= cfg.ro_delay) & (di < n_drv)
    d = np.where(ok, iq_drv[int(pairs['drv_row'][p])][np.where(ok, di, 0)], 0)
    reads = kept_readouts(cfg, summary, events, lane, meas_cap, event_cap)
    seen = np.zeros(n_lo, np.int64)
    for t_lo, _ in reads:
        seen += t_lo <= n
    st = np.array([state(cfg, shot, core, q) for q in range(max(len(reads), 1))], np.int64)[np.maximum(seen, 1) - 1]
    return s16(d), s16(d >> 16), st


def feedline_adc_res(cfg, pairs, lines, coef, adc_sigma, summary, events, iq_drv, n_lo, meas_cap, event_cap=None,
                     y_peak=None):
    """adc uint32 (n_lines, n_lo): words {I16 low, Q16 high}.  ``y_peak``: a list that receives max |y| component"""
    summary, events, event_cap = _views(summary, events, event_cap)
    iq_drv = np.asarray(iq_drv).view(np.uint32)
    coef = np.asarray(coef, np.int64)
    members = np.array([p for line in lines for p in line])
    first = np.concatenate([[0], np.cumsum([len(line) for line in lines])[:-1]])
    ins = [member_inputs(cfg, pairs, p, summary, events, iq_drv, n_lo, meas_cap, event_cap) for p in members]
    x_i, x_q = (np.ascontiguousarray(np.stack([m[q] for m in ins]).T) for q in (0, 1))      # [n_lo, members]
    k = coef[members[:, None], np.stack([m[2] for m in ins])]                               # [members, n_lo, 4]
    a_re, a_im, c_re, c_im = (np.ascontiguousarray(k[..., q].T) for q in range(4))
    y_i, y_q = np.zeros(len(members), np.int64), np.zeros(len(members), np.int64)
    g_i, g_q = np.zeros((n_lo, len(members)), np.int64), np.zeros((n_lo, len(members)), np.int64)
    peak = 0
    for j in range(n_lo):                                # all members of all lines at once, sample by sample
        y_i, y_q = (x_i[j] + ((a_re[j] * y_i - a_im[j] * y_q + HALF) >> 30),
                    x_q[j] + ((a_re[j] * y_q + a_im[j] * y_i + HALF) >> 30))
        g_i[j] = (c_re[j] * y_i - c_im[j] * y_q + HALF) >> 30
        g_q[j] = (c_re[j] * y_q + c_im[j] * y_i + HALF) >> 30
        if y_peak is not None:
            peak = max(peak, int(np.abs(y_i).max()), int(np.abs(y_q).max()))
    tot_i = np.add.reduceat(np.clip(g_i, -32767, 32767), first, axis=1).T                   # [n_lines, n_lo]
    tot_q = np.add.reduceat(np.clip(g_q, -32767, 32767), first, axis=1).T
    if adc_sigma:
        for l, line in enumerate(lines):
            nu_i, nu_q = adc_noise(cfg.seed, int(pairs['shot'][line[0]]), int(pairs['core'][line[0]]), n_lo, adc_sigma)
            tot_i[l] += nu_i
            tot_q[l] += nu_q
    tot_i, tot_q = np.clip(tot_i, -32767, 32767), np.clip(tot_q, -32767, 32767)
    if y_peak is not None:
        y_peak.append(peak)
    return ((tot_i & 0xFFFF) | ((tot_q & 0xFFFF) << 16)).astype(np.uint32)


def degenerate_coef(cfg, n_pairs):
    """the coefficients at which the stage is dpemu_feedline_adc at unit gains: pole 0, coupling the Q15
    rotation of ro_theta[s] << 15"""
    import oracle
    lut = oracle.dds_sin_lut().astype(np.int64)
    coef = np.zeros((n_pairs, 2, 4), np.int64)
    for s in (0, 1):
        ti = ((cfg.ro_theta[s] + (1 << 19)) >> 20) & 4095
        coef[:, s, 2], coef[:, s, 3] = int(lut[(ti + 1024) & 4095]) << 15, int(lut[ti]) << 15
    return coef
