"""CPU reference of the decaying qubit-state stage (dpemu_qsim_decay,
include/dpemu.h; DESIGN.md §2 "Decoherence"): a Python-integer restatement of
the header's rule on the helpers of tests/qsim_ref.py and
tests/qsim_meas_ref.py.  Not test code of its own: tests/test_qsim_decay.py
validates the specification with it on the CPU, tests/test_gpu_qsim_decay.py
holds the kernels to it bit for bit."""

import functools

import numpy as np

from tests.demod_iq_ref import M32, philox4
from tests.qsim_meas_ref import MEAS_CTR, kept_strobes, measure, shift_of
from tests.qsim_ref import (M64, NO_CORE, ONE, PAIRS, apply_pair, drive_strobes, lane_of, merged, on_qubit, pauli_pair,
                            phase_factor, rotated)

OWN_CTR, TARGET_CTR, FINAL_CTR = 0x08000000, 0x04000000, 0x02000000     # | core: the counter ranges of the decay draws


def span_factor(tab, dt):
    """F over the span dt from a 32-entry Q30 table: the entries of dt's set bits, ascending, each product rounded"""
    f = ONE
    for i in range(32):
        if (dt >> i) & 1:
            f = (f * int(tab[i]) + (1 << 29)) >> 30
    return f


def pop(c):
    return c[0] * c[0] + c[1] * c[1]


def int32(v):
    """v modulo 2^32 as an int32: what a component is where a wrapped total let the shift pass 2^31 (defined, not
    meaningful; a state within the gate rule's bounds never gets here)"""
    return ((v + (1 << 31)) & M32) - (1 << 31)


def decay_step(x, which, g, e, draw):
    """the damping step (g < 2^30 only), then the dephasing step, on qubit ``which`` of the amplitudes x (a list
    of 4 (re, im), changed in place) with the draw's words.  Returns (jumped, flipped)."""
    pairs = PAIRS[which]
    jumped = flipped = False
    if g < ONE:
        T = sum(pop(c) for c in x) & M64
        A = sum(pop(x[hi]) for _, hi in pairs) & M64
        y = {hi: tuple((g * v + (1 << 29)) >> 30 for v in x[hi]) for _, hi in pairs}
        A2 = sum(pop(c) for c in y.values()) & M64
        u = draw[0]
        v = u * (T >> 32) + ((u * (T & M32)) >> 32)
        jumped = v < ((A - A2) & M64)
        for lo, hi in pairs:
            if jumped:
                x[lo], x[hi] = x[hi], (0, 0)
            else:
                x[hi] = y[hi]
        s = shift_of(sum(pop(c) for c in x) & M64)
        for j in range(4):
            x[j] = (int32(x[j][0] << s), int32(x[j][1] << s))
    if draw[1] < ((ONE - e) << 1):
        flipped = True
        for _, hi in pairs:
            x[hi] = (int32(-x[hi][0]), int32(-x[hi][1]))
    return jumped, flipped


def qsim_decay(cfg, reg_core, gates, drv_elem, detune, damp, deph, summary, events, n_shots, shot_begin=0,
               event_cap=None, measure_readouts=False, t_final=0, amps=None, advances=None):
    """dpemu_qsim (``measure_readouts`` false) or dpemu_qsim_meas with the decay rule.  damp / deph: [C][32] Q30
    words.  Returns pops uint64 (n_regs, n_shots, 4), result uint32 (n_regs, n_shots, 4), states uint32 (n_lanes,)
    -- None without ``measure_readouts`` -- and counts uint32 (n_regs, n_shots, 4).  ``amps`` (a list) receives every
    row's final amplitudes, ``advances`` every advance with dt > 0 as (row, core, tag, n, dt, jumped, flipped)."""
    summary = np.asarray(summary).view(np.uint32).reshape(-1, 8)
    events = np.asarray(events).view(np.uint32)
    events = events.reshape(events.shape[0] if events.ndim == 3 else -1, summary.shape[0], 4)
    event_cap = cfg.event_cap if event_cap is None else int(event_cap)
    seed, meas_elem = int(cfg.seed), int(cfg.meas_elem)
    table = {(g['core'], g['freq'], g['env'], g['amp']): g for g in gates}
    n_regs = len(reg_core)
    pops = np.zeros((n_regs, n_shots, 4), np.uint64)
    result = np.zeros((n_regs, n_shots, 4), np.uint32)
    counts = np.zeros((n_regs, n_shots, 4), np.uint32)
    states = np.zeros(summary.shape[0], np.uint32) if measure_readouts else None
    for r, (c_first, c_second) in enumerate(reg_core):
        cores = [int(c_first)] + ([int(c_second)] if int(c_second) != NO_CORE else [])
        for sl in range(n_shots):
            shot, row = shot_begin + sl, r * n_shots + sl
            lanes = [lane_of(cfg, sl, c, n_shots) for c in cores]
            ovf = any(int(summary[L, 2]) > event_cap for L in lanes)
            if measure_readouts:
                lists = [kept_strobes(summary, events, L, event_cap, drv_elem, meas_elem) for L in lanes] + [[]]
            else:
                lists = [[s + (False,) for s in drive_strobes(summary, events, L, event_cap, drv_elem)] for L in lanes] + [[]]
            x = [(ONE, 0), (0, 0), (0, 0), (0, 0)]
            n_gates = n_unmatched = n_errors = 0
            n_read, tl = [0, 0], [0, 0]

            def advance(which, t, tag, n):
                if t <= tl[which]:
                    return
                dt, tl[which] = t - tl[which], t
                core = cores[which]
                g, e = span_factor(damp[core], dt), span_factor(deph[core], dt)
                j, f = decay_step(x, which, g, e, philox4(seed, shot, tag | core, n))
                counts[r, sl, 2 * which] += j
                counts[r, sl, 2 * which + 1] += f
                if advances is not None:
                    advances.append((row, core, tag, n, dt, j, f))

            for q, (t, k, w1, w2, w3, readout) in merged(lists[0], lists[1]):
                core = cores[q]
                if readout:
                    advance(q, t, OWN_CTR, k)
                    m = n_read[q]
                    b, _ = measure(x, q, philox4(seed, shot, MEAS_CTR | core, m)[0])
                    assert all(v == int32(v) for c in x for v in c)    # (qsim_meas_ref's shift is written for int32 states)
                    if m < 32:
                        states[lanes[q]] |= np.uint32(b << m)
                    n_read[q] += 1
                    continue
                g = table.get((core, w2 >> 17, w1 & 0xFFFFFF, w3 & 0xFFFF))
                if g is None:
                    n_unmatched += 1
                    continue
                n_gates += 1
                kind = g['kind']
                advance(q, t, OWN_CTR, k)
                if kind == 1:
                    advance(1, t, TARGET_CTR, k)
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
            if t_final:
                for which in range(len(cores)):
                    advance(which, t_final, FINAL_CTR, 0)
            P = [pop(c) for c in x]
            T = sum(P) & M64
            u = philox4(seed, shot, 0x20000000 | cores[0], 0)[0]
            v = u * (T >> 32) + ((u * (T & M32)) >> 32)
            run = [P[0] & M64, (P[0] + P[1]) & M64, (P[0] + P[1] + P[2]) & M64]
            j = sum(1 for s_ in run if s_ <= v)
            pops[r, sl] = P
            result[r, sl] = ((j >> 1) | ((j & 1) << 1), n_gates, n_unmatched, (n_errors & 0xFFFF) | (ovf << 31))
            if amps is not None:
                amps.append(list(x))
    return pops, result, states, counts


def decay_words(gs, cores_per_shot):
    """(damp, deph) uint32 [C, 32] of a qsim.GateSet, 2^30 where no decay is set"""
    damp, deph = (np.full((cores_per_shot, 32), ONE, np.uint32) for _ in range(2))
    for c, (a, b) in gs.decay.items():
        damp[c], deph[c] = a, b
    return damp, deph


def qsim_decay_gateset(cfg, gs, summary, events, n_shots, shot_begin=0, event_cap=None, measure_readouts=False,
                       t_final=0, amps=None, advances=None, tables=None):
    """qsim_decay() on the tables of a distributed_processor_amd.qsim.GateSet (``tables``: other (damp, deph))"""
    damp, deph = decay_words(gs, cfg.cores_per_shot) if tables is None else tables
    return qsim_decay(cfg, [tuple(int(v) for v in row) for row in gs.reg_core], gs.entries, gs.drv_elem,
                      gs.detune_words(cfg.cores_per_shot), damp, deph, summary, events, n_shots, shot_begin, event_cap,
                      measure_readouts, t_final, amps, advances)
