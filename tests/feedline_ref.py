"""CPU reference of the multiplexed readout stages (dpemu_feedline_adc and
dpemu_demod_feedline, include/dpemu.h; DESIGN.md §2 "Multiplexed readout"): a
plain numpy / Python-integer restatement of the specification on
tests/demod_iq_ref.py's helpers.  Not test code of its own:
tests/test_feedline.py validates the specification with it on the CPU,
tests/test_gpu_feedline.py holds the kernels to it bit for bit.

``pairs`` is demod_iq_ref.demod_iq's dict of columns; ``lines`` a sequence of
sequences of pair indices."""

import numpy as np

import oracle
from tests.demod_iq_ref import M32, noise, philox4, s16, symsat_q15, wrap32


def kept_readouts(cfg, summary, events, lane, meas_cap, event_cap):
    """[(t_lo, env word)] of the lane's readouts dpemu_demod_iq keeps"""
    ev = events[:min(int(summary[lane, 2]), event_cap), lane]
    reads = [(int(e[0]), int(e[1])) for e in ev if e[1] >> 28 == 0 and (e[1] >> 24) & 3 == cfg.meas_elem]
    return reads[:meas_cap]


def state(cfg, shot, core, m):
    thr = cfg.p1_threshold[core]
    return 1 if (thr == M32 or philox4(cfg.seed, shot, core, m)[0] < thr) else 0


def _views(summary, events, event_cap):
    summary = np.asarray(summary).view(np.uint32)
    events = np.asarray(events).view(np.uint32)
    return summary, events, events.shape[0] if event_cap is None else int(event_cap)


def feedline_adc(cfg, pairs, lines, summary, events, iq_drv, n_lo, meas_cap, event_cap=None):
    """adc uint32 (n_lines, n_lo): words {I16 low, Q16 high}"""
    lut = oracle.dds_sin_lut().astype(np.int64)
    summary, events, event_cap = _views(summary, events, event_cap)
    iq_drv = np.asarray(iq_drv).view(np.uint32)
    n_drv = iq_drv.shape[1]
    rot = []
    for s in (0, 1):
        ti = ((cfg.ro_theta[s] + (1 << 19)) >> 20) & 4095
        rot.append((int(lut[(ti + 1024) & 4095]), int(lut[ti])))
    adc = np.zeros((len(lines), n_lo), np.uint32)
    j = np.arange(n_lo, dtype=np.int64)
    for l, line in enumerate(lines):
        tot_i, tot_q = np.zeros(n_lo, np.int64), np.zeros(n_lo, np.int64)
        spc_d, spc_l = int(pairs['spc_drv'][line[0]]), int(pairs['spc_lo'][line[0]])
        for p in line:
            assert (int(pairs['spc_drv'][p]), int(pairs['spc_lo'][p])) == (spc_d, spc_l)
            lane, core, shot = int(pairs['lane'][p]), int(pairs['core'][p]), int(pairs['shot'][p])
            n, k = j // spc_l, j % spc_l
            di = (n - cfg.ro_delay) * spc_d + k * (spc_d // spc_l)
            ok = (n >= cfg.ro_delay) & (di < n_drv)
            d = np.where(ok, iq_drv[int(pairs['drv_row'][p])][np.where(ok, di, 0)], 0)
            d_i, d_q = s16(d), s16(d >> 16)
            reads = kept_readouts(cfg, summary, events, lane, meas_cap, event_cap)
            seen = np.zeros(n_lo, np.int64)
            for t_lo, _ in reads:
                seen += t_lo <= n
            m = np.maximum(seen, 1) - 1
            st = np.array([state(cfg, shot, core, q) for q in range(max(len(reads), 1))], np.int64)[m]
            c = np.where(st == 1, rot[1][0], rot[0][0])
            s_ = np.where(st == 1, rot[1][1], rot[0][1])
            gain = np.where(st == 1, int(cfg.ro_gain[1]), int(cfg.ro_gain[0]))
            r_i, r_q = symsat_q15(d_i * c - d_q * s_), symsat_q15(d_i * s_ + d_q * c)
            tot_i += (r_i * gain + (1 << 15)) >> 16
            tot_q += (r_q * gain + (1 << 15)) >> 16
        tot_i, tot_q = np.clip(tot_i, -32767, 32767), np.clip(tot_q, -32767, 32767)
        adc[l] = ((tot_i & 0xFFFF) | ((tot_q & 0xFFFF) << 16)).astype(np.uint32)
    return adc


def demod_feedline(cfg, pairs, lines, summary, events, adc, iq_lo, meas_cap, event_cap=None):
    """acc int32 (meas_cap, n_pairs, 2), result uint32 (n_pairs, 2).  P = adc conj(lo) in int64 for every int16
    half of both words, -32768 included (a caller's trace may hold it; include/dpemu.h)"""
    summary, events, event_cap = _views(summary, events, event_cap)
    adc = np.asarray(adc).view(np.uint32)
    iq_lo = np.asarray(iq_lo).view(np.uint32)
    n_pairs, n_lo = len(pairs['lane']), iq_lo.shape[1]
    line_of = {p: l for l, line in enumerate(lines) for p in line}
    assert len(line_of) == n_pairs == sum(len(line) for line in lines)
    acc = np.zeros((meas_cap, n_pairs, 2), np.int32)
    result = np.zeros((n_pairs, 2), np.uint32)
    for i in range(n_pairs):
        lane, core, shot = int(pairs['lane'][i]), int(pairs['core'][i]), int(pairs['shot'][i])
        spc_l = int(pairs['spc_lo'][i])
        lo, a = iq_lo[int(pairs['lo_row'][i])], adc[line_of[i]]
        reads = kept_readouts(cfg, summary, events, lane, meas_cap, event_cap)
        bits = 0
        for m, (t_lo, pe) in enumerate(reads):
            words = (pe >> 12) & 0xFFF or 4096
            j = np.arange(min(t_lo * spc_l, n_lo), min((t_lo + words * cfg.ro_cpw) * spc_l, n_lo), dtype=np.int64)
            a_i, a_q = s16(a[j]), s16(a[j] >> 16)
            lo_i, lo_q = s16(lo[j]), s16(lo[j] >> 16)
            S = (int((a_i * lo_i + a_q * lo_q).sum()), int((a_q * lo_i - a_i * lo_q).sum()))
            h = 15 + spc_l.bit_length() - 1
            _, zi, zq = noise(cfg.seed, shot, core, m, cfg.ro_sigma)
            out = []
            for S_c, z in zip(S, (zi, zq)):
                T = (S_c + (1 << (h - 1))) >> h
                out.append(wrap32(max(-2 ** 31, min(2 ** 31 - 1, T)) + z))
            acc[m, i] = out
            ax = cfg.ro_axis[core]
            x = (out[0] * int(s16(ax)) + out[1] * int(s16(ax >> 16))) >> 15
            bits |= int(x > cfg.ro_thr) << m
        result[i] = (len(reads), bits)
    return acc, result


def feedline(cfg, pairs, lines, summary, events, iq_drv, iq_lo, meas_cap, event_cap=None):
    """both stages: (adc, acc, result)"""
    adc = feedline_adc(cfg, pairs, lines, summary, events, iq_drv, np.asarray(iq_lo).shape[1], meas_cap, event_cap)
    return (adc,) + demod_feedline(cfg, pairs, lines, summary, events, adc, iq_lo, meas_cap, event_cap)
