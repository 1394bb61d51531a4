"""CPU reference of the measuring qubit-state stage (dpemu_qsim_meas,
include/dpemu.h; DESIGN.md §2 "Measurement"): a Python-integer restatement of
the header's rule on tests/qsim_ref.py's helpers, and state-injected variants
of the numpy references of the readout stages (the *_st entry points): the
functions of feedline_ref / resonator_ref / traces_ref / iq_stats_ref with
their state draw replaced by a lookup in per-lane ``states`` words.  Not test
code of its own: tests/test_qsim_meas.py validates the specification with it
on the CPU, tests/test_gpu_qsim_meas.py holds the kernels to it bit for bit."""

import contextlib
import functools

import numpy as np

from tests import feedline_ref, iq_stats_ref, resonator_ref, traces_ref
from tests.demod_iq_ref import M32, philox4
from tests.qsim_ref import (M64, NO_CORE, ONE, apply_pair, lane_of, merged, on_qubit, pauli_pair, phase_factor,
                            rotated)

MEAS_CTR = 0x10000000                                   # | core: the counter range of the readout draws


def kept_strobes(summary, events, lane, event_cap, drv_elem, meas_elem):
    """[(t, slot, w1, w2, w3, is_readout)] of the lane's drive and readout strobes among its first
    min(n_events, event_cap) records, in record order"""
    out = []
    for k in range(min(int(summary[lane, 2]), event_cap)):
        t, w1, w2, w3 = (int(v) for v in events[k, lane])
        if w1 >> 28 == 0 and (w1 >> 24) & 3 in (drv_elem, meas_elem):
            out.append((t, k, w1, w2, w3, (w1 >> 24) & 3 == meas_elem))
    return out


def shift_of(t_rest):
    """s of the renormalising shift: 0 for T' = 0, else max(0, (59 - msb(T')) >> 1)"""
    return 0 if t_rest == 0 else max(0, (59 - (t_rest.bit_length() - 1)) >> 1)


def measure(x, which, u):
    """readout of qubit ``which`` (0: the first core's, 1: the second's) of the amplitudes x (a list of 4
    (re, im), changed in place) with the draw u.  Returns (b, s): the outcome and the shift applied."""
    P = [re * re + im * im for re, im in x]
    T = sum(P) & M64
    ones = [j for j in range(4) if (j >> (1 - which)) & 1]
    A = sum(P[j] for j in ones) & M64
    v = u * (T >> 32) + ((u * (T & M32)) >> 32)
    b = 1 if ((T - A) & M64) <= v else 0
    keep = [j for j in range(4) if ((j >> (1 - which)) & 1) == b]
    s = shift_of(sum(P[j] for j in keep) & M64)
    for j in range(4):
        x[j] = (x[j][0] << s, x[j][1] << s) if j in keep else (0, 0)
    return b, s


def qsim_meas(cfg, reg_core, gates, drv_elem, detune, summary, events, n_shots, shot_begin=0, event_cap=None,
              amps=None, shifts=None):
    """tests/qsim_ref.qsim with readout strobes (element cfg.meas_elem) measuring.  Returns pops uint64
    (n_regs, n_shots, 4), result uint32 (n_regs, n_shots, 4), states uint32 (n_lanes,).  ``amps`` (a list)
    receives every row's final amplitudes, ``shifts`` (a list) every readout's (row, core, m, b, s)."""
    summary = np.asarray(summary).view(np.uint32).reshape(-1, 8)
    events = np.asarray(events).view(np.uint32)
    events = events.reshape(events.shape[0] if events.ndim == 3 else -1, summary.shape[0], 4)
    event_cap = cfg.event_cap if event_cap is None else int(event_cap)
    seed, meas_elem = int(cfg.seed), int(cfg.meas_elem)
    assert meas_elem <= 3 and meas_elem != drv_elem
    table = {(g['core'], g['freq'], g['env'], g['amp']): g for g in gates}
    n_regs = len(reg_core)
    pops = np.zeros((n_regs, n_shots, 4), np.uint64)
    result = np.zeros((n_regs, n_shots, 4), np.uint32)
    states = np.zeros(summary.shape[0], np.uint32)
    for r, (c_first, c_second) in enumerate(reg_core):
        cores = [int(c_first)] + ([int(c_second)] if int(c_second) != NO_CORE else [])
        for sl in range(n_shots):
            shot = shot_begin + sl
            lanes = [lane_of(cfg, sl, c, n_shots) for c in cores]
            ovf = any(int(summary[L, 2]) > event_cap for L in lanes)
            lists = [kept_strobes(summary, events, L, event_cap, drv_elem, meas_elem) for L in lanes] + [[]]
            x = [(ONE, 0), (0, 0), (0, 0), (0, 0)]
            n_gates = n_unmatched = n_errors = 0
            n_read = [0, 0]
            for q, (t, k, w1, w2, w3, readout) in merged(lists[0], lists[1]):
                core = cores[q]
                if readout:
                    m = n_read[q]
                    b, s = measure(x, q, philox4(seed, shot, MEAS_CTR | core, m)[0])
                    if m < 32:
                        states[lanes[q]] |= np.uint32(b << m)
                    n_read[q] += 1
                    if shifts is not None:
                        shifts.append((r * n_shots + sl, core, m, b, s))
                    continue
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
            if amps is not None:
                amps.append(list(x))
    return pops, result, states


def qsim_meas_gateset(cfg, gs, summary, events, n_shots, shot_begin=0, event_cap=None, amps=None, shifts=None):
    """qsim_meas() on the tables of a distributed_processor_amd.qsim.GateSet"""
    return qsim_meas(cfg, [tuple(int(v) for v in row) for row in gs.reg_core], gs.entries, gs.drv_elem,
                     gs.detune_words(cfg.cores_per_shot), summary, events, n_shots, shot_begin, event_cap, amps,
                     shifts)


# ---- states into the readout stages ------------------------------------------
# The base references draw the prepared state of (shot, core, m) through one
# module-level function each (feedline_ref.state, imported by name into
# resonator_ref and traces_ref; iq_stats_ref.states, vectorised).  The injected
# variants run the same code with that function looking the bit up.

def _word_table(shot, core, words):
    return {(int(s), int(c)): int(w) for s, c, w in zip(shot, core, words)}


@contextlib.contextmanager
def _injected(table):
    def state(cfg, shot, core, m):
        return (table[(int(shot), int(core))] >> int(m)) & 1

    def states(cfg, shot, core, m):
        shot, core = np.broadcast_arrays(np.asarray(shot), np.asarray(core))
        w = np.array([table[(int(s), int(c))] for s, c in zip(shot.reshape(-1), core.reshape(-1))], np.int64)
        return ((w >> int(m)) & 1).reshape(shot.shape)
    saved = (feedline_ref.state, resonator_ref.state, traces_ref.state, iq_stats_ref.states)
    feedline_ref.state = resonator_ref.state = traces_ref.state = state
    iq_stats_ref.states = states
    try:
        yield
    finally:
        feedline_ref.state, resonator_ref.state, traces_ref.state, iq_stats_ref.states = saved


def _pair_table(pairs, states):
    st = np.asarray(states).view(np.uint32).reshape(-1)
    lane = np.asarray(pairs['lane'], np.int64)
    return _word_table(pairs['shot'], pairs['core'], st[lane])


def feedline_adc_st(states, cfg, pairs, *a, **kw):
    """feedline_ref.feedline_adc with pair p's state at readout m = (states[pairs['lane'][p]] >> m) & 1"""
    with _injected(_pair_table(pairs, states)):
        return feedline_ref.feedline_adc(cfg, pairs, *a, **kw)


def feedline_adc_res_st(states, cfg, pairs, *a, **kw):
    """resonator_ref.feedline_adc_res, likewise"""
    with _injected(_pair_table(pairs, states)):
        return resonator_ref.feedline_adc_res(cfg, pairs, *a, **kw)


def feedline_traces_st(states, cfg, pairs, *a, **kw):
    """traces_ref.feedline_traces, likewise"""
    with _injected(_pair_table(pairs, states)):
        return traces_ref.feedline_traces(cfg, pairs, *a, **kw)


def iq_stats_st(states, cfg, acc, counts, core=None, shot=None, shot_begin=0, **kw):
    """iq_stats_ref.iq_stats with the state of (col, m) = (states[col] >> m) & 1: states holds n_cols words"""
    st = np.asarray(states).view(np.uint32).reshape(-1)
    n_cols = np.asarray(acc).shape[1]
    assert st.size == n_cols
    c, s = iq_stats_ref.run_columns(cfg, n_cols, shot_begin) if core is None else (core, shot)
    with _injected(_word_table(s, c, st)):
        return iq_stats_ref.iq_stats(cfg, acc, counts, core=core, shot=shot, shot_begin=shot_begin, **kw)


def draw_words(cfg, shot, core, n_bits=32):
    """the packed Philox draws: per (shot, core) the word whose bit m is the base references' state draw of
    (shot, core, m) -- injected, every *_st reference equals its base"""
    out = np.zeros(len(shot), np.uint32)
    for i, (s, c) in enumerate(zip(shot, core)):
        for m in range(n_bits):
            out[i] |= np.uint32(feedline_ref.state(cfg, int(s), int(c), m) << m)
    return out
