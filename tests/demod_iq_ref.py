"""CPU reference of the waveform demodulation stage (dpemu_demod_iq,
include/dpemu.h; DESIGN.md §2 "Waveform demodulation"): a plain numpy / Python
restatement of the specification, sample by sample in Python integers and
int64 arrays.  Not test code of its own: tests/test_demod_iq.py validates the
specification with it on the CPU, tests/test_gpu_demod_iq.py holds the kernel
to it bit for bit."""

import numpy as np

import oracle

M32 = 0xFFFFFFFF


def philox4(seed, shot, core, m):
    """Philox4x32-10, counter (shot low, shot high, core, m), key = seed"""
    c = [shot & M32, (shot >> 32) & M32, core & M32, m & M32]
    k0, k1 = seed & M32, (seed >> 32) & M32
    for _ in range(10):
        p0, p1 = c[0] * 0xD2511F53, c[2] * 0xCD9E8D57
        c = [(p1 >> 32) ^ c[1] ^ k0, p1 & M32, (p0 >> 32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c


def s16(v):
    """the int16 values of the low halves of an array of words"""
    return ((np.asarray(v, np.int64) & 0xFFFF) ^ 0x8000) - 0x8000


def symsat_q15(x):
    """symsat((x + 2^14) >> 15): floor shift, clamp to [-32767, 32767]"""
    return np.clip((x + (1 << 14)) >> 15, -32767, 32767)


def noise(seed, shot, core, m, sigma):
    """(state draw word, z_I * sigma >> 16, z_Q * sigma >> 16) of readout m"""
    r = philox4(seed, shot, core, m)
    u0, u1, u2, u3 = r[1] & 0xFFFF, r[1] >> 16, r[2] & 0xFFFF, r[2] >> 16
    return r[0], ((u0 + u1 - u2 - u3) * sigma) >> 16, ((u0 - u1 + u2 - u3) * sigma) >> 16


def wrap32(v):
    return ((int(v) + (1 << 31)) & M32) - (1 << 31)


def demod_iq(cfg, pairs, summary, events, iq_drv, iq_lo, meas_cap, event_cap=None):
    """pairs: dict of equal-length sequences lane, core, shot, drv_row, lo_row,
    spc_drv, spc_lo; summary (n_lanes, 8), events (slots, n_lanes, 4) and the
    two iq arrays (rows, n_samples) as the run and dpemu_dds wrote them.
    Returns acc int32 (meas_cap, n_pairs, 2), result uint32 (n_pairs, 2)."""
    lut = oracle.dds_sin_lut().astype(np.int64)
    summary = np.asarray(summary).view(np.uint32)
    events = np.asarray(events).view(np.uint32)
    iq_drv = np.asarray(iq_drv).view(np.uint32)
    iq_lo = np.asarray(iq_lo).view(np.uint32)
    event_cap = events.shape[0] if event_cap is None else int(event_cap)
    n_pairs = len(pairs['lane'])
    n_drv, n_lo = iq_drv.shape[1], iq_lo.shape[1]
    acc = np.zeros((meas_cap, n_pairs, 2), np.int32)
    result = np.zeros((n_pairs, 2), np.uint32)
    for i in range(n_pairs):
        lane, core, shot = int(pairs['lane'][i]), int(pairs['core'][i]), int(pairs['shot'][i])
        spc_d, spc_l = int(pairs['spc_drv'][i]), int(pairs['spc_lo'][i])
        assert spc_l & (spc_l - 1) == 0 and spc_d % spc_l == 0
        drv, lo = iq_drv[int(pairs['drv_row'][i])], iq_lo[int(pairs['lo_row'][i])]
        ev = events[:min(int(summary[lane, 2]), event_cap), lane]
        reads = [(int(e[0]), int(e[1])) for e in ev if e[1] >> 28 == 0 and (e[1] >> 24) & 3 == cfg.meas_elem]
        count = min(len(reads), meas_cap)
        bits = 0
        for m in range(count):
            t_lo, pe = reads[m]
            words = (pe >> 12) & 0xFFF or 4096
            j = np.arange(min(t_lo * spc_l, n_lo), min((t_lo + words * cfg.ro_cpw) * spc_l, n_lo), dtype=np.int64)
            n, k = j // spc_l, j % spc_l
            di = (n - cfg.ro_delay) * spc_d + k * (spc_d // spc_l)
            ok = (n >= cfg.ro_delay) & (di < n_drv)
            d = np.where(ok, drv[np.where(ok, di, 0)], 0)
            d_i, d_q = s16(d), s16(d >> 16)
            thr = cfg.p1_threshold[core]
            draw, zi, zq = noise(cfg.seed, shot, core, m, cfg.ro_sigma)
            s = 1 if (thr == M32 or draw < thr) else 0
            ti = ((cfg.ro_theta[s] + (1 << 19)) >> 20) & 4095
            c, s_ = int(lut[(ti + 1024) & 4095]), int(lut[ti])
            r_i, r_q = symsat_q15(d_i * c - d_q * s_), symsat_q15(d_i * s_ + d_q * c)
            lo_i, lo_q = s16(lo[j]), s16(lo[j] >> 16)
            S = (int((r_i * lo_i + r_q * lo_q).sum()), int((r_q * lo_i - r_i * lo_q).sum()))
            h = 15 + spc_l.bit_length() - 1
            out = []
            for S_c, z in zip(S, (zi, zq)):
                T = (S_c + (1 << (h - 1))) >> h
                sig = max(-2 ** 31, min(2 ** 31 - 1, (T * cfg.ro_gain[s] + (1 << 15)) >> 16))
                out.append(wrap32(sig + z))
            acc[m, i] = out
            ax = cfg.ro_axis[core]
            x = (out[0] * int(s16(ax)) + out[1] * int(s16(ax >> 16))) >> 15
            bits |= int(x > cfg.ro_thr) << m
        result[i] = (count, bits)
    return acc, result
