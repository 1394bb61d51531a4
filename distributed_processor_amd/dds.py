"""DDS I/Q synthesis from emulated pulse events (hot-path row 4).

The reference stops at the pulse interface: each core drives
``pulse_iface`` {env_word, phase, freq, amp, cfg} plus ``cstrobe`` into the
external QubiC DSP (hdl/pulse_iface.sv:2-6, hdl/proc.sv:131-136), and the
assembler hands that DSP its per-element env / freq buffers
(assembler.py:472-476, asmparse.py:46-86).  This module plays the emulated
pulse timelines through a fixed-point DDS on the GPU (``dpemu_dds``,
csrc/dds.hip) so a caller gets sample-level I/Q per (shot, core, element)
channel.  The arithmetic is build-defined and pinned
bit-exactly by oracle/dds_ref.c.

Usage::

    plan = ChannelPlan(programs, cfg, shot_begin, n_shots,
                       [(shot, core, elem), ...], elem_params={0: (16, 1), 2: (4, 4)})
    iq = emu.synthesize(plan, device_outputs, n_samples)     # torch int32 [n_ch, n_samples]
"""

from __future__ import annotations

from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np

from . import _abi

DESC_FIELDS = ('ch_lane', 'ch_elem', 'spc', 'interp', 'env_off', 'env_len', 'freq_off', 'freq_len')


class ChannelPlan:
    """Channel descriptors and concatenated env / freq tables for one run.

    programs: the ProgramSet that was run (its ``buffers`` hold the
    assembler's env_buffers / freq_buffers of every (group, core));
    channels: (absolute shot, core, element) triples, all inside
    [shot_begin, shot_begin + n_shots); elem_params: element -> (samples per
    clock, interpolation ratio).  Tables shared by several channels are stored
    once.
    """

    def __init__(self, programs, cfg, shot_begin: int, n_shots: int,
                 channels: Iterable[Tuple[int, int, int]],
                 elem_params: Dict[int, Tuple[int, int]]):
        C_ = cfg.cores_per_shot
        spg, ng = max(int(cfg.shots_per_group), 1), max(int(cfg.n_groups), 1)
        envs, freqs = [], []
        env_at: Dict[bytes, Tuple[int, int]] = {}
        freq_at: Dict[bytes, Tuple[int, int]] = {}
        n_env = n_freq = 0

        def place(tab, store, at, n):
            key = tab.tobytes()
            if key not in at:
                at[key] = (n, len(tab))
                store.append(tab)
                n += len(tab)
            return at[key], n

        rows = []
        self.channels = []                  # row i's (shot, core, elem)
        for shot, core, elem in channels:
            shot, core, elem = int(shot), int(core), int(elem)
            self.channels.append((shot, core, elem))
            if not (shot_begin <= shot < shot_begin + n_shots) or not (0 <= core < C_):
                raise ValueError('channel ({}, {}, {}) outside the run'.format(shot, core, elem))
            if elem not in elem_params:
                raise ValueError('no (spc, interp) for element {}'.format(elem))
            g = (shot // spg) % ng
            env_l, freq_l = programs.buffers.get((g, core), ([], []))
            env = env_l[elem] if elem < len(env_l) else np.zeros(0, np.uint32)
            frq = freq_l[elem] if elem < len(freq_l) else np.zeros(0, np.uint32)
            (eo, el), n_env = place(np.ascontiguousarray(env, np.uint32), envs, env_at, n_env)
            (fo, fl), n_freq = place(np.ascontiguousarray(frq, np.uint32), freqs, freq_at, n_freq)
            spc, interp = elem_params[elem]
            lane = int(_abi.lane_index(shot - shot_begin, core, n_shots, C_, cfg.lane_order))
            rows.append((lane, elem, spc, interp, eo, el, fo, fl))
        self.desc = np.array(rows, np.uint32).reshape(-1, 8)
        self.env = np.concatenate(envs).astype(np.uint32) if n_env else np.zeros(1, np.uint32)
        self.freq = np.concatenate(freqs).astype(np.uint32) if n_freq else np.zeros(1, np.uint32)
        self.n_lanes = int(n_shots) * C_
        self.event_cap = int(cfg.event_cap)
        self._cols = {f: np.ascontiguousarray(self.desc[:, i]) for i, f in enumerate(DESC_FIELDS)}
        self._dev = None

    @property
    def n_channels(self):
        return self.desc.shape[0]

    def struct(self, n_samples: int) -> _abi.DDSChannels:
        s = _abi.DDSChannels(self.n_channels, self.n_lanes, int(n_samples), self.event_cap)
        for f in DESC_FIELDS:
            setattr(s, f, self._cols[f].ctypes.data)
        return s

    def device_tables(self, device='cuda'):
        """env / freq tables as device tensors (uploaded once per plan)."""
        if self._dev is None:
            import torch
            self._dev = (torch.from_numpy(self.env.view(np.int32)).to(device),
                         torch.from_numpy(self.freq.view(np.int32)).to(device))
        return self._dev


class DemodPairTable:
    """The (drive row, LO row) pairs of ``dpemu_demod_iq`` (include/dpemu.h).

    Pair i is row ``drv_rows[i]`` of ``drv_plan`` (a channel of element
    ``cfg.ro_drv_elem``) with row ``lo_rows[i]`` of ``lo_plan`` (element
    ``cfg.meas_elem``), both of one (shot, core); default rows: i with i.
    Raises DpemuError otherwise.  ``one_plan`` pairs the two channels of every
    (shot, core) that has both in a single plan (one iq buffer)."""

    FIELDS = ('lane', 'core', 'shot', 'drv_row', 'lo_row', 'spc_drv', 'spc_lo')

    def __init__(self, cfg, drv_plan: ChannelPlan, lo_plan: ChannelPlan, drv_rows=None, lo_rows=None):
        from ._native import DpemuError
        if drv_rows is None and lo_rows is None and drv_plan.n_channels != lo_plan.n_channels:
            raise DpemuError('drive plan has {} channels, LO plan {}'.format(drv_plan.n_channels,
                                                                             lo_plan.n_channels))
        drv_rows = list(range(drv_plan.n_channels)) if drv_rows is None else [int(r) for r in drv_rows]
        lo_rows = list(range(lo_plan.n_channels)) if lo_rows is None else [int(r) for r in lo_rows]
        if len(drv_rows) != len(lo_rows):
            raise DpemuError('{} drive rows but {} LO rows'.format(len(drv_rows), len(lo_rows)))
        if drv_plan.n_lanes != lo_plan.n_lanes or drv_plan.event_cap != lo_plan.event_cap:
            raise DpemuError('the two plans are of different runs (n_lanes / event_cap)')
        cols = {f: [] for f in self.FIELDS}
        for i, (rd, rl) in enumerate(zip(drv_rows, lo_rows)):
            if not (0 <= rd < drv_plan.n_channels and 0 <= rl < lo_plan.n_channels):
                raise DpemuError('pair {}: rows ({}, {}) outside the plans'.format(i, rd, rl))
            (sd, cd, ed), (sl, cl, el) = drv_plan.channels[rd], lo_plan.channels[rl]
            if (sd, cd) != (sl, cl) or drv_plan.desc[rd, 0] != lo_plan.desc[rl, 0]:
                raise DpemuError('pair {}: drive channel of (shot {}, core {}) but LO channel of (shot {}, core {})'
                                 .format(i, sd, cd, sl, cl))
            if ed != cfg.ro_drv_elem or el != cfg.meas_elem:
                raise DpemuError('pair {}: elements ({}, {}), want ro_drv_elem {} and meas_elem {}'.format(
                    i, ed, el, cfg.ro_drv_elem, cfg.meas_elem))
            spc_d, spc_l = int(drv_plan.desc[rd, 2]), int(lo_plan.desc[rl, 2])
            if spc_l < 1 or spc_l & (spc_l - 1) or spc_d % spc_l:
                raise DpemuError('pair {}: spc_lo {} must be a power of two dividing spc_drv {}'.format(
                    i, spc_l, spc_d))
            for f, v in zip(self.FIELDS, (int(drv_plan.desc[rd, 0]), cd, sd, rd, rl, spc_d, spc_l)):
                cols[f].append(v)
        self.cols = {f: np.array(v, np.uint64 if f == 'shot' else np.uint32) for f, v in cols.items()}
        self.n_pairs = len(drv_rows)
        self.n_lanes, self.event_cap = drv_plan.n_lanes, drv_plan.event_cap
        self.n_rows = (drv_plan.n_channels, lo_plan.n_channels)

    @classmethod
    def one_plan(cls, cfg, plan: ChannelPlan):
        at = {ch: i for i, ch in enumerate(plan.channels)}
        drv = [(i, at[(s_, c, cfg.meas_elem)]) for i, (s_, c, e) in enumerate(plan.channels)
               if e == cfg.ro_drv_elem and (s_, c, cfg.meas_elem) in at]
        return cls(cfg, plan, plan, [d for d, _ in drv], [l for _, l in drv])

    def struct(self, meas_cap: int, n_samples_drv: int, n_samples_lo: int) -> _abi.DemodPairs:
        s = _abi.DemodPairs(self.n_pairs, self.n_lanes, self.event_cap, int(meas_cap), int(n_samples_drv),
                            int(n_samples_lo))
        for f in self.FIELDS:
            setattr(s, f, self.cols[f].ctypes.data)
        return s


class FeedlineTable:
    """The feedlines of ``dpemu_feedline_adc`` / ``dpemu_demod_feedline``
    (include/dpemu.h): ``lines`` is a sequence of sequences of pair indices
    of ``pair_table`` (a DemodPairTable); default: one line per shot holding
    all of that shot's pairs, in table order, lines in order of first
    appearance.  Raises DpemuError for what the C side refuses: no line, an
    empty line, more than ``_abi.FEEDLINE_MAX`` members, a member outside the
    table, a pair in two lines, members of different sample rates.
    ``line_of[i]`` is pair i's line, -1 when it has none (the ADC stage
    ignores such a pair, the demodulator refuses it)."""

    def __init__(self, pair_table: DemodPairTable, lines=None):
        from ._native import DpemuError
        n = pair_table.n_pairs
        if lines is None:
            by_shot: Dict[int, list] = {}
            for i, s in enumerate(pair_table.cols['shot'].tolist()):
                by_shot.setdefault(s, []).append(i)
            lines = list(by_shot.values())
        lines = [[int(m) for m in ln] for ln in lines]
        if not lines:
            raise DpemuError('a feedline table needs at least one line')
        line_of = np.full(n, -1, np.int64)
        for l, ln in enumerate(lines):
            if not 1 <= len(ln) <= _abi.FEEDLINE_MAX:
                raise DpemuError('line {} has {} members, want 1..{}'.format(l, len(ln), _abi.FEEDLINE_MAX))
            for m in ln:
                if not 0 <= m < n:
                    raise DpemuError('line {}: member {} outside the pair table ({} pairs)'.format(l, m, n))
                if line_of[m] >= 0:
                    raise DpemuError('pair {} is in two lines ({} and {})'.format(m, line_of[m], l))
                line_of[m] = l
                for f in ('spc_drv', 'spc_lo'):
                    if pair_table.cols[f][m] != pair_table.cols[f][ln[0]]:
                        raise DpemuError('line {}: pairs {} and {} differ in {}'.format(l, ln[0], m, f))
        self.pairs = pair_table
        self.lines = lines
        self.n_lines = len(lines)
        self.line_of = line_of
        self.line_first = np.concatenate([[0], np.cumsum([len(ln) for ln in lines])]).astype(np.uint32)
        self.member = np.array([m for ln in lines for m in ln], np.uint32)

    def struct(self) -> _abi.Feedlines:
        return _abi.Feedlines(self.n_lines, self.line_first.ctypes.data, self.member.ctypes.data)


class ResonatorTable:
    """The readout resonators of ``dpemu_feedline_adc_res`` (include/dpemu.h):
    per pair of ``pair_table`` (a DemodPairTable) and prepared state a one-pole
    response y' = x + a y with return c y', both Q30.

    ``f_res`` [n_pairs, 2]: the resonator frequency in state 0 and state 1 --
    32-bit unsigned words in the unit of a freq buffer's word 0 (turns per clock
    / 2^32, the DDS's convention); ``kappa``: the full linewidth
    in the same unit (one value, one per pair, or [n_pairs, 2]).  Per LO sample
    a = exp((-pi kappa + 2 pi i f_res) / (2^32 spc_lo)) and c = gain
    exp(i phase) (1 - |a|), so a drive on resonance returns gain exp(i phase)
    times itself in the steady state; ``gain`` / ``phase`` broadcast against
    f_res likewise.  ``adc_sigma``: the per-sample converter noise scale (a
    float stored Q16, as the configuration's sigmas are).  Raises DpemuError
    for what the C side refuses: a pole beyond |a| <= 1 - 2^-12, a coupling
    component beyond +-2^30.  ``from_coefficients`` takes the integer words."""

    POLE_MAX = (1 << 30) - (1 << 18)

    def __init__(self, pair_table: DemodPairTable, f_res, kappa, gain=1.0, phase=0.0, adc_sigma=0.0):
        from ._native import DpemuError
        n = pair_table.n_pairs
        try:
            f = np.broadcast_to(np.asarray(f_res, np.float64), (n, 2))
            kap = np.asarray(kappa, np.float64)
            kap = np.broadcast_to(kap[:, None] if kap.ndim == 1 else kap, (n, 2))      # [n]: one per pair
            g = np.broadcast_to(np.asarray(gain, np.float64), (n, 2))
            ph = np.broadcast_to(np.asarray(phase, np.float64), (n, 2))
        except ValueError as e:
            raise DpemuError('f_res must be [{} pairs, 2 states]; kappa, gain and phase broadcast to it ({})'
                             .format(n, e))
        if np.asarray(f_res).shape != (n, 2) or (f < 0).any() or (f >= 2.0 ** 32).any() or (f != np.floor(f)).any():
            raise DpemuError('f_res must hold [{}, 2] unsigned 32-bit frequency words'.format(n))
        if (kap < 0).any():
            raise DpemuError('kappa must be >= 0')
        spc_lo = pair_table.cols['spc_lo'].astype(np.float64)[:, None]
        a = np.exp((-np.pi * kap + 2j * np.pi * f) / (2.0 ** 32 * spc_lo))
        c = g * np.exp(1j * ph) * (1.0 - np.abs(a))
        coef = np.stack([a.real, a.imag, c.real, c.imag], axis=-1) * 2.0 ** 30
        sig = int(round(float(adc_sigma) * 65536))
        self._set(pair_table, np.rint(coef), sig)

    @classmethod
    def from_coefficients(cls, pair_table: DemodPairTable, coef, adc_sigma: int = 0):
        """``coef`` [n_pairs, 2 states, 4] = pole_re, pole_im, coup_re, coup_im as Q30 integers; ``adc_sigma``
        the noise scale word itself"""
        self = cls.__new__(cls)
        self._set(pair_table, coef, adc_sigma)
        return self

    def _set(self, pair_table, coef, adc_sigma):
        from ._native import DpemuError
        n = pair_table.n_pairs
        coef = np.asarray(coef)
        if coef.shape != (n, 2, 4):
            raise DpemuError('coef must be [{} pairs, 2 states, 4], got {}'.format(n, list(coef.shape)))
        if not np.isfinite(coef.astype(np.float64)).all() or (coef != np.floor(coef)).any() or \
                (np.abs(coef) >= 2.0 ** 62).any():
            raise DpemuError('coef must hold integers')
        coef = coef.astype(np.int64)
        pole = np.minimum(np.abs(coef[..., :2]), 1 << 31)         # (clipped: the squares stay inside int64)
        bad = np.argwhere(pole[..., 0] ** 2 + pole[..., 1] ** 2 > self.POLE_MAX ** 2)
        if len(bad):
            p, s = bad[0]
            raise DpemuError('pair {} state {}: pole ({}, {}) outside |a| <= 2^30 - 2^18 (1 - 2^-12)'.format(
                p, s, coef[p, s, 0], coef[p, s, 1]))
        bad = np.argwhere(np.abs(coef[..., 2:]).max(axis=-1) > 2 ** 30)
        if len(bad):
            p, s = bad[0]
            raise DpemuError('pair {} state {}: coupling ({}, {}) outside +-2^30'.format(p, s, coef[p, s, 2],
                                                                                         coef[p, s, 3]))
        if int(adc_sigma) != adc_sigma or not 0 <= int(adc_sigma) < 2 ** 32:
            raise DpemuError('adc_sigma word {} is not a uint32'.format(adc_sigma))
        self.pairs = pair_table
        self.coef = np.ascontiguousarray(coef.astype(np.int32))
        self.adc_sigma = int(adc_sigma)

    def struct(self) -> _abi.Resonators:
        return _abi.Resonators(self.coef.ctypes.data, self.adc_sigma)


class SynthesisPipeline:
    """DDS synthesis of successive batches with ``depth`` batches in flight.

    One ``dpemu_dds`` call runs ``dds_index_kernel`` (the per-channel event
    index, latency-bound: ~15 us at config 5) and then ``dds_tile_kernel`` on
    one stream, so the index cannot overlap its own batch's tiles -- but it
    can overlap the previous batch's.  The pipeline holds ``depth`` library
    contexts (each owns its event index, so their calls are independent),
    one stream and one I/Q buffer per context, and sends batch k to context
    k % depth: batch k + 1's index kernel runs beside batch k's tile kernel.
    On the builder's box that measured 0.329 -> 0.317 ms per config-5 step
    (``profiles/r03_dds_pipe.json``), but the driver's round-4 record has the
    8-deep pipeline SLOWER than one context (0.3377 vs 0.3283 ms); ``bench.py``
    measures one context and depth 2 on the same line (``--dds-depth 2``) and
    reports the faster (round 5: 0.312 vs 0.327 ms, ``profiles/r05_dds_depth.json``).

    Streams beyond the process's hardware queues (``GPU_MAX_HW_QUEUES``, 4 by
    default) share them: at most 4 batches execute at once, the others wait
    on their queue behind one; depth 8 keeps every queue's
    next batch ready.

    ``synthesize`` makes its stream wait for the caller's current stream (the
    producer of ``outputs``) and returns (iq, stream): iq is valid on that
    stream, and is overwritten by the call ``depth`` batches later, so a
    consumer runs on ``stream`` (or waits for it) before then.  ``drain()``
    waits for every batch.
    """

    def __init__(self, device: int = 0, depth: int = 2, lib_path: Optional[str] = None, streams=None):
        import torch
        from .emulator import Emulator
        if depth < 1:
            raise ValueError('depth must be >= 1')
        if streams is not None and len(streams) < depth:
            raise ValueError('need {} streams, got {}'.format(depth, len(streams)))
        self.device = torch.device('cuda', device)
        self.emus = []
        try:
            for _ in range(depth):
                self.emus.append(Emulator(device, lib_path=lib_path))
        except Exception:
            self.close()
            raise
        # streams: the caller's (e.g. created once at start-up, each on its own
        # hardware queue: streams that share a queue run their kernels in turn)
        self.streams = list(streams[:depth]) if streams is not None else \
            [torch.cuda.Stream(device=self.device) for _ in range(depth)]
        self.iq = [None] * depth
        self.k = 0

    def synthesize(self, plan: ChannelPlan, outputs: dict, n_samples: int):
        import torch
        j = self.k % len(self.emus)
        shape = (plan.n_channels, int(n_samples))
        if self.iq[j] is None or tuple(self.iq[j].shape) != shape:
            self.streams[j].synchronize()           # the old buffer's last batch is done with it
            self.iq[j] = torch.empty(shape, dtype=torch.int32, device=self.device)
        s = self.streams[j]
        s.wait_stream(torch.cuda.current_stream(self.device))
        self.emus[j].synthesize(plan, outputs, n_samples, self.iq[j], s)
        self.k += 1
        return self.iq[j], s

    def drain(self):
        for s in self.streams:
            s.synchronize()

    def kernel_timing(self, on: bool):
        for e in self.emus:
            e.kernel_timing(on)

    def close(self):
        for e in self.emus:
            e.close()
        self.emus = []
        self.iq = [None] * len(self.iq) if hasattr(self, 'iq') else []


def split_iq(iq_u32: np.ndarray):
    """(I, Q) int16 arrays of dpemu_dds output words (I low half, Q high half)."""
    v = np.asarray(iq_u32).view(np.uint32)
    return (v & 0xFFFF).astype(np.uint16).view(np.int16), (v >> 16).astype(np.uint16).view(np.int16)
