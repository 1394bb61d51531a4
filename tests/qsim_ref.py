"""CPU reference of the qubit-state stage (dpemu_qsim, include/dpemu.h; DESIGN.md
§2 "Qubit state from the drive pulses"): a plain Python-integer restatement of
the header's rules, row by row and gate by gate, independent of the C++.  Not
test code of its own: tests/test_qsim.py validates the specification with it
on the CPU, tests/test_gpu_qsim.py holds the kernel to it bit for bit."""

import functools

import numpy as np

from tests.demod_iq_ref import M32, philox4

ONE = 1 << 30
M64 = (1 << 64) - 1
LIM = (1 << 31) - 1
NO_CORE = 0xFFFFFFFF


@functools.lru_cache(maxsize=1)
def phase_lut():
    """int64 [768, 2]: {cos, sin} in Q30 of 2 pi i / 512 (512 coarse entries), then of 2 pi i / 2^17 (256 fine)"""
    i = np.arange(512, dtype=np.float64)
    a = np.concatenate([2 * np.pi * i / 512.0, 2 * np.pi * i[:256] / 131072.0])
    t = np.stack([np.rint(np.cos(a) * ONE), np.rint(np.sin(a) * ONE)], axis=1).astype(np.int64)
    for k, v in enumerate(((ONE, 0), (0, ONE), (-ONE, 0), (0, -ONE))):
        t[128 * k] = v
    t[512] = (ONE, 0)
    t.setflags(write=False)
    return t


def cmulr(p, x):
    """{(p_re x_re - p_im x_im + 2^29) >> 30, (p_re x_im + p_im x_re + 2^29) >> 30} on Python integers"""
    return ((p[0] * x[0] - p[1] * x[1] + (1 << 29)) >> 30, (p[0] * x[1] + p[1] * x[0] + (1 << 29)) >> 30)


def clamp(v):
    return max(-LIM, min(LIM, v))


def phase_factor(phi):
    lut = phase_lut()
    c, f = lut[phi >> 8], lut[512 + (phi & 255)]
    return cmulr((int(c[0]), int(c[1])), (int(f[0]), int(f[1])))


def rotated(m, w):
    """the 8 words of M under U = Rz(phi) M Rz(-phi): (a, b', c', d)"""
    a, b, c, d = ((int(m[2 * i]), int(m[2 * i + 1])) for i in range(4))
    return a, cmulr(b, (w[0], -w[1])), cmulr(c, w), d


def apply_pair(g, x0, x1):
    a, b, c, d = g
    p, q, r, s = cmulr(a, x0), cmulr(b, x1), cmulr(c, x0), cmulr(d, x1)
    return (clamp(p[0] + q[0]), clamp(p[1] + q[1])), (clamp(r[0] + s[0]), clamp(r[1] + s[1]))


def pauli_pair(code, x0, x1):
    if code == 1:
        return x1, x0
    if code == 2:
        return (x1[1], -x1[0]), (-x0[1], x0[0])
    if code == 3:
        return x0, (-x1[0], -x1[1])
    return x0, x1


# amplitude index pairs (bit 0, bit 1) of the first core's qubit (j = 2 b_first + b_second) and the second's
PAIRS = {0: ((0, 2), (1, 3)), 1: ((0, 1), (2, 3))}


def on_qubit(x, which, fn_lo, fn_hi=None):
    """fn on both pairs of qubit `which` (0 first core, 1 second); fn_hi for the second listed pair"""
    for n, (i, j) in enumerate(PAIRS[which]):
        x[i], x[j] = (fn_hi if (n and fn_hi is not None) else fn_lo)(x[i], x[j])


def lane_of(cfg, sl, core, n_shots):
    return sl * cfg.cores_per_shot + core if cfg.lane_order == 1 else core * n_shots + sl


def drive_strobes(summary, events, lane, event_cap, drv_elem):
    """[(t, slot, w1, w2, w3)] of the lane's drive strobes among its first min(n_events, event_cap) records"""
    out = []
    for k in range(min(int(summary[lane, 2]), event_cap)):
        t, w1, w2, w3 = (int(v) for v in events[k, lane])
        if w1 >> 28 == 0 and (w1 >> 24) & 3 == drv_elem:
            out.append((t, k, w1, w2, w3))
    return out


def merged(a, b):
    """two-way merge: the first list's head when t_first <= t_second; entries (which, record)"""
    out, i, j = [], 0, 0
    while i < len(a) or j < len(b):
        if j >= len(b) or (i < len(a) and a[i][0] <= b[j][0]):
            out.append((0, a[i]))
            i += 1
        else:
            out.append((1, b[j]))
            j += 1
    return out


def qsim(cfg, reg_core, gates, drv_elem, detune, summary, events, n_shots, shot_begin=0, event_cap=None, states=None):
    """reg_core: [(first, second or NO_CORE)]; gates: dicts core, freq, env, amp, kind, err_thr, m ([2][8] Q30 words);
    detune: per-core Q32 words or None; summary (n_lanes, 8) / events (slots, n_lanes, 4) as the run wrote them.
    Returns pops uint64 (n_regs, n_shots, 4), result uint32 (n_regs, n_shots, 4); ``states`` (a list), when
    given, receives every row's final amplitudes [(re, im)] * 4 in row order."""
    summary = np.asarray(summary).view(np.uint32).reshape(-1, 8)
    events = np.asarray(events).view(np.uint32)
    events = events.reshape(events.shape[0] if events.ndim == 3 else -1, summary.shape[0], 4)
    event_cap = cfg.event_cap if event_cap is None else int(event_cap)
    seed = int(cfg.seed)
    table = {(g['core'], g['freq'], g['env'], g['amp']): g for g in gates}
    n_regs = len(reg_core)
    pops = np.zeros((n_regs, n_shots, 4), np.uint64)
    result = np.zeros((n_regs, n_shots, 4), np.uint32)
    for r, (c_first, c_second) in enumerate(reg_core):
        cores = [int(c_first)] + ([int(c_second)] if int(c_second) != NO_CORE else [])
        for sl in range(n_shots):
            shot = shot_begin + sl
            lanes = [lane_of(cfg, sl, c, n_shots) for c in cores]
            ovf = any(int(summary[L, 2]) > event_cap for L in lanes)
            lists = [drive_strobes(summary, events, L, event_cap, drv_elem) for L in lanes] + [[]]
            x = [(ONE, 0), (0, 0), (0, 0), (0, 0)]
            n_gates = n_unmatched = n_errors = 0
            for q, (t, k, w1, w2, w3) in merged(lists[0], lists[1]):
                core = cores[q]
                g = table.get((core, w2 >> 17, w1 & 0xFFFFFF, w3 & 0xFFFF))
                if g is None:
                    n_unmatched += 1
                    continue
                n_gates += 1
                kind = g['kind']
                c_ph = cores[1] if kind == 1 else core
                det = int(detune[c_ph]) if detune is not None else 0
                phi = ((w2 & 0x1FFFF) + ((det * t) >> 15)) & 0x1FFFF
                w = phase_factor(phi)
                g0 = rotated(g['m'][0], w)
                if kind == 0:
                    on_qubit(x, q, functools.partial(apply_pair, g0))
                else:
                    on_qubit(x, 1, functools.partial(apply_pair, g0), functools.partial(apply_pair, rotated(g['m'][1], w)))
                if g['err_thr']:
                    rr = philox4(seed, shot, 0x40000000 | core, k)
                    if rr[0] < g['err_thr']:
                        n_errors += 1
                        if kind == 0:
                            on_qubit(x, q, functools.partial(pauli_pair, 1 + ((rr[1] * 3) >> 32)))
                        else:
                            idx = 1 + ((rr[1] * 15) >> 32)
                            on_qubit(x, 0, functools.partial(pauli_pair, idx >> 2))
                            on_qubit(x, 1, functools.partial(pauli_pair, idx & 3))
            P = [re * re + im * im for re, im in x]
            T = sum(P) & M64
            u = philox4(seed, shot, 0x20000000 | cores[0], 0)[0]
            v = u * (T >> 32) + ((u * (T & M32)) >> 32)
            run = [P[0] & M64, (P[0] + P[1]) & M64, (P[0] + P[1] + P[2]) & M64]
            j = sum(1 for s_ in run if s_ <= v)
            pops[r, sl] = P
            result[r, sl] = ((j >> 1) | ((j & 1) << 1), n_gates, n_unmatched, (n_errors & 0xFFFF) | (ovf << 31))
            if states is not None:
                states.append(list(x))
    return pops, result


def qsim_gateset(cfg, gs, summary, events, n_shots, shot_begin=0, event_cap=None, states=None):
    """qsim() on the tables of a distributed_processor_amd.qsim.GateSet"""
    return qsim(cfg, [tuple(int(v) for v in row) for row in gs.reg_core], gs.entries, gs.drv_elem,
                gs.detune_words(cfg.cores_per_shot), summary, events, n_shots, shot_begin, event_cap, states)
