"""Qubit-state simulation from the emulated drive pulses: the host side of
dpemu_qsim (include/dpemu.h is the definition; DESIGN.md §2 "Qubit state from
the drive pulses" states the conventions).

A :class:`GateSet` is the dictionary of calibrated pulses -- which (core, freq
index, env word, amp word) a drive strobe must carry to stand for which 2x2
matrix -- plus the qubit registers and the drive detunings.
``Emulator.simulate_gates`` runs it over the events of a run; :func:`survival`
and :func:`fit_decay` turn the sampled outcomes into an RB decay.  With
``measure=True`` (dpemu_qsim_meas) the readout strobes measure, and the
per-lane ``states`` words go into the readout stages; :func:`state_bits` and
:func:`readout_survival` read them, or the bits the readout chain discriminated.
``Emulator.cosimulate`` hands the same words back to the interpreter
(dpemu_run_states) until they reproduce themselves, so measurement-conditioned
branches follow the simulated qubit (DESIGN.md §2 "Co-simulation").
``GateSet.set_decay`` gives a core's qubit a T1 and a T2: the same calls then go
through dpemu_qsim_decay, where a qubit relaxes and dephases over the clocks
between the strobes that act on it (DESIGN.md §2 "Decoherence")."""

import ctypes as C

import numpy as np

from . import _abi

ONE = 1 << 30


def rotation(theta, axis_turns=0.0):
    """exp(-i theta / 2 (cos a X + sin a Y)), a = 2 pi axis_turns, complex128 [2, 2]"""
    a = 2 * np.pi * float(axis_turns)
    c, s = np.cos(theta / 2), np.sin(theta / 2)
    return np.array([[c, -1j * s * np.exp(-1j * a)], [-1j * s * np.exp(1j * a), c]], np.complex128)


def to_q30(m):
    """complex [2, 2] -> the 8 Q30 words {a_re, a_im, b_re, b_im, c_re, c_im, d_re, d_im}, rounded by np.rint"""
    m = np.asarray(m, np.complex128).reshape(4)
    return np.rint(np.stack([m.real, m.imag], axis=1).reshape(8) * ONE).astype(np.int64)


def err_threshold(p):
    """a probability as err_thr / 2^32 (0: no error draw)"""
    return int(min(max(np.rint(float(p) * 2.0 ** 32), 0), 0xFFFFFFFF))


def decay_tables(t1=None, t2=None):
    """(damp, deph), uint32 [32] each, of dpemu_qsim_decay for a qubit with relaxation time ``t1`` and coherence
    time ``t2`` in clocks (None: infinite; t1 alone: t2 = 2 t1): damp[i] = rint(2^30 e^(-2^i / (2 t1))), the |1>
    amplitude factor over 2^i clocks, and deph[i] = rint(2^30 e^(-2^i / tphi)) with 1 / tphi = 1 / t2 - 1 / (2 t1),
    the pure-dephasing coherence factor.  t2 > 2 t1 is no physical qubit and is refused."""
    rate1 = 0.0 if t1 is None else 1.0 / (2.0 * _positive('t1', t1))
    rate_phi = 0.0 if t2 is None else 1.0 / _positive('t2', t2) - rate1
    if rate_phi < -1e-12 * rate1:
        raise ValueError('t2 = {} exceeds 2 t1 = {}'.format(t2, 2.0 * float(t1)))
    span = 2.0 ** np.arange(32)
    return tuple(np.rint(np.exp(-span * max(r, 0.0)) * ONE).astype(np.uint32) for r in (rate1, rate_phi))


def _positive(name, v):
    v = float(v)
    if not v > 0 or not np.isfinite(v):
        raise ValueError('{} = {} must be a positive number of clocks'.format(name, v))
    return v


class GateSet:
    """The dictionary, registers and detunings of dpemu_qsim.

    ``entries``: dicts core, freq, env, amp, kind, err_thr, m (int64 [2, 8], the
    Q30 words) and u (complex128 [2, 2, 2], the matrices before rounding)."""

    def __init__(self, drv_elem=0):
        self.drv_elem = int(drv_elem)
        self.entries = []
        self.reg_core = np.zeros((0, 2), np.uint32)
        self.detune = {}                     # core -> turns per clock, Q32
        self.decay = {}                      # core -> (damp, deph) of decay_tables: dpemu_qsim_decay when not empty
        self._zx_target = {}                 # control core -> the target add_zx named

    def add_matrix(self, core, freq, env, amp, m0, m1=None, kind=0, err=0.0, err_thr=None):
        """an entry from its matrices: complex [2, 2], or the 8 Q30 words as integers"""
        ms = [m0, m0 if m1 is None else m1]
        q, u = np.zeros((2, 8), np.int64), np.zeros((2, 2, 2), np.complex128)
        for i, m in enumerate(ms):
            m = np.asarray(m)
            if m.shape == (8,):
                q[i] = m.astype(np.int64)
                u[i] = (q[i, 0::2] + 1j * q[i, 1::2]).reshape(2, 2) / ONE
            else:
                q[i], u[i] = to_q30(m), np.asarray(m, np.complex128)
        self.entries.append(dict(core=int(core), freq=int(freq), env=int(env), amp=int(amp), kind=int(kind),
                                 err_thr=err_threshold(err) if err_thr is None else int(err_thr), m=q, u=u))
        return self

    def add_rotation(self, core, freq, env, amp, theta, axis_turns=0.0, err=0.0):
        """a pulse of ``core`` on its own qubit: a rotation by theta about the axis at axis_turns (0: X) in
        the frame; the strobe's phase word turns the axis further"""
        return self.add_matrix(core, freq, env, amp, rotation(theta, axis_turns), err=err)

    def add_zx(self, control, target, freq, env, amp, theta, err=0.0):
        """a cross-resonance pulse on ``control``'s drive: exp(-i theta / 2 Z (x) X), Rx(theta) on the target
        when the control is 0 and Rx(-theta) when it is 1 (the target is the register's other core)"""
        self._zx_target[int(control)] = int(target)
        return self.add_matrix(control, freq, env, amp, rotation(theta), rotation(-theta), kind=1, err=err)

    def registers(self, pairs):
        """the qubit registers: (first core, second core) pairs, or a core / (core, None) for one qubit"""
        rows = []
        for p in pairs:
            a, b = (p, None) if np.isscalar(p) else p
            rows.append((int(a), _abi.QSIM_NO_CORE if b is None else int(b)))
        self.reg_core = np.array(rows, np.uint32).reshape(-1, 2)
        for c, t in self._zx_target.items():
            if not any(r[0] == c and r[1] == t for r in rows):
                raise ValueError('add_zx({}, {}): no register ({}, {})'.format(c, t, c, t))
        return self

    def set_detune(self, core, turns_per_clock):
        """drive detuning of ``core``'s qubit frame, in turns per clock (stored Q32, modulo one turn)"""
        self.detune[int(core)] = int(np.rint(float(turns_per_clock) * 2.0 ** 32)) & 0xFFFFFFFF
        return self

    def set_decay(self, core, t1=None, t2=None):
        """relaxation and coherence times of ``core``'s qubit in clocks (:func:`decay_tables`); with a decay on
        any core ``Emulator.simulate_gates`` and ``cosimulate`` go through dpemu_qsim_decay"""
        self.decay[int(core)] = decay_tables(t1, t2)
        return self

    def decay_struct(self, cfg, t_final=0):
        """(_abi.QsimDecay, the host arrays it points into): [cores_per_shot, 32] tables, 2^30 where no decay is set"""
        damp, deph = (np.full((cfg.cores_per_shot, 32), ONE, np.uint32) for _ in range(2))
        for c, (a, b) in self.decay.items():
            if not 0 <= c < cfg.cores_per_shot:
                raise ValueError('set_decay: core {} >= cores_per_shot {}'.format(c, cfg.cores_per_shot))
            damp[c], deph[c] = a, b
        if not 0 <= int(t_final) < 2 ** 32:
            raise ValueError('t_final {} is no uint32 clock'.format(t_final))
        st = _abi.QsimDecay()
        st.damp, st.deph, st.t_final = damp.ctypes.data, deph.ctypes.data, int(t_final)
        return st, (damp, deph)

    @property
    def n_regs(self):
        return len(self.reg_core)

    def keys(self):
        """{(core, freq, env, amp)} of the entries"""
        return {(e['core'], e['freq'], e['env'], e['amp']) for e in self.entries}

    def detune_words(self, cores_per_shot):
        """uint32 [cores_per_shot], or None when no core is detuned"""
        if not self.detune:
            return None
        d = np.zeros(cores_per_shot, np.uint32)
        for c, v in self.detune.items():
            d[c] = v
        return d

    def struct(self, cfg, n_shots, shot_begin, event_cap=None):
        """(_abi.Qsim, the host arrays it points into) for a run of n_shots shots from shot_begin under cfg"""
        gates = (_abi.QsimGate * max(len(self.entries), 1))()
        for g, e in zip(gates, self.entries):
            g.core, g.freq, g.env, g.amp, g.kind, g.err_thr = (e[k] for k in ('core', 'freq', 'env', 'amp', 'kind',
                                                                                'err_thr'))
            for i in range(2):
                for k in range(8):
                    v = int(e['m'][i, k])
                    if not -2 ** 31 <= v < 2 ** 31:
                        raise ValueError('matrix word {} does not fit int32'.format(v))
                    g.m[i][k] = v
        reg = np.ascontiguousarray(self.reg_core, np.uint32)
        det = self.detune_words(cfg.cores_per_shot)
        st = _abi.Qsim()
        st.n_regs, st.reg_core = len(reg), reg.ctypes.data if len(reg) else None
        st.n_gates, st.gates = len(self.entries), C.addressof(gates)
        st.drv_elem = self.drv_elem
        st.detune = det.ctypes.data if det is not None else None
        st.n_lanes = int(n_shots) * cfg.cores_per_shot
        st.event_cap = cfg.event_cap if event_cap is None else int(event_cap)
        st.shot_begin, st.n_shots = int(shot_begin), int(n_shots)
        return st, (gates, reg, det)


def survival(result, shots_per_group):
    """fraction of outcome 0 per run of ``shots_per_group`` consecutive shots (one RB sequence) of every
    register: result [n_regs, n_shots, 4] (a tensor or an array) -> float64 [n_regs, n_shots // shots_per_group]"""
    r = result.cpu().numpy() if hasattr(result, 'cpu') else np.asarray(result)
    n_regs, n_shots = r.shape[0], r.shape[1]
    spg = int(shots_per_group)
    if spg < 1 or n_shots % spg:
        raise ValueError('n_shots {} is not a whole number of groups of {}'.format(n_shots, spg))
    zero = r[:, :, 0] == 0
    return zero.reshape(n_regs, n_shots // spg, spg).mean(axis=2)


def _lane_major(words, cfg, n_shots):
    """per-lane words [n_lanes] (a tensor or an array) -> uint32 [C, n_shots] in either lane order"""
    w = words.cpu().numpy() if hasattr(words, 'cpu') else np.asarray(words)
    C_, n = cfg.cores_per_shot, int(n_shots)
    w = np.ascontiguousarray(w).reshape(-1).view(np.uint32)
    if w.size != C_ * n:
        raise ValueError('{} words for {} cores x {} shots'.format(w.size, C_, n))
    return w.reshape(n, C_).T.copy() if cfg.lane_order == _abi.LANES_SHOT_MAJOR else w.reshape(C_, n).copy()


def state_bits(states, cfg, n_shots):
    """the ``states`` words of ``Emulator.simulate_gates(measure=True)`` as uint32 [C, n_shots]: the
    post-measurement bit of readout m of (core, shot) in bit m, whatever cfg's lane order"""
    return _lane_major(states, cfg, n_shots)


def readout_survival(bits, reg_core, shots_per_group, slot=0):
    """:func:`survival` from discriminated outcome bits: the fraction of every sequence's shots whose
    registers all read 0 at readout ``slot``.  ``bits``: [C, n_shots] words, the outcome of readout m of
    (core, shot) in bit m -- :func:`state_bits` of ``iq_stats``' per-lane ``bits`` or of the bits word
    ``result[:, 1]`` of a ``demodulate_feedline`` whose pairs are the run's lanes -- or such a result
    table itself as [C, n_shots, 2].  ``reg_core``: the registers' (first, second or QSIM_NO_CORE)
    cores.  Returns float64 [n_shots // shots_per_group]."""
    b = bits.cpu().numpy() if hasattr(bits, 'cpu') else np.asarray(bits)
    if b.ndim == 3 and b.shape[2] == 2:                 # a result table [C, n_shots, 2]: the bits are word 1
        b = b[:, :, 1]
    b = b.view(np.uint32) if b.dtype == np.int32 else b.astype(np.uint32)
    if b.ndim != 2:
        raise ValueError('bits must be [C, n_shots] (state_bits brings per-lane words to it)')
    n_shots, spg = b.shape[1], int(shots_per_group)
    if spg < 1 or n_shots % spg:
        raise ValueError('n_shots {} is not a whole number of groups of {}'.format(n_shots, spg))
    cores = [int(c) for c in np.asarray(reg_core, np.uint32).reshape(-1) if int(c) != _abi.QSIM_NO_CORE]
    if not cores:
        raise ValueError('no register core')
    one = ((b[cores] >> np.uint32(slot)) & np.uint32(1)).any(axis=0)
    return (~one).reshape(n_shots // spg, spg).mean(axis=1)


def fit_decay(depths, surv, asymptote=0.25):
    """(A, p) of survival = A p^m + asymptote by least squares on log(survival - asymptote) over the depths m
    (points at or below the asymptote carry no logarithm and are left out)"""
    m, s = np.asarray(depths, np.float64), np.asarray(surv, np.float64) - float(asymptote)
    ok = s > 0
    if ok.sum() < 2:
        raise ValueError('fit_decay needs two depths above the asymptote')
    slope, icpt = np.polyfit(m[ok], np.log(s[ok]), 1)
    return float(np.exp(icpt)), float(np.exp(slope))
