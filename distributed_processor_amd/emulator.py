"""Host front end: run assembled distproc programs on the MI355X emulator.

Drop-in for the reference simulation path: where the reference loads one
``cmd_buf`` into a Verilator ``toplevel_sim`` and clocks it from cocotb
(cocotb/proc/test_proc.py:29-38, sim_modules/toplevel_sim.sv:13-33), here the
output of ``GlobalAssembler.get_assembled_program()`` (assembler.py:623-641)
-- ``{core_ind: {'cmd_buf': bytes, 'env_buffers': [...], 'freq_buffers': [...]}}``
-- or raw command words go to :class:`Emulator`, which runs n_shots x C
cores on the GPU through libdpemu.so and returns pulse events, register
traces, measurements and outcome histograms.
"""

from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, List, Optional, Sequence, Union

import numpy as np

from . import _abi, isa
from ._native import DpemuError, check, load_library
from .stage_tensors import (check_demod_tensors, check_feedline_tensors, check_iq_stats_tensors, check_qsim_tensors,
                            check_run_inputs, check_states_tensor, check_trace_tensors, dds_specs, qsim_decay_specs,
                            tensor_or_new)
from .stage_tensors import check_tensor as _check_tensor        # (run_device's name for it since before the move)

ProgramLike = Union[bytes, Sequence[int], np.ndarray]


def _to_u32(prog: ProgramLike) -> np.ndarray:
    if isinstance(prog, (bytes, bytearray)):
        return isa.cmd_buf_to_u32(bytes(prog))
    if isinstance(prog, np.ndarray) and prog.dtype == np.uint32:
        return np.ascontiguousarray(prog.reshape(-1, 4))
    return isa.words_to_u32([int(w) for w in prog])


def _next_pow2(n: int) -> int:
    c = 1
    while c < n:
        c <<= 1
    return c


def _shot_programs(shot):
    """one shot's programs: assembler dict {core: {'cmd_buf': ..., 'env_buffers':
    [...], 'freq_buffers': [...]}}, dict {core: words}, or a list (index = core).
    Returns ({core: (n, 4) u32}, {core: (env_buffers, freq_buffers)})."""
    progs, bufs = {}, {}
    items = shot.items() if isinstance(shot, dict) else enumerate(shot)
    for k, v in items:
        if isinstance(v, dict):
            bufs[int(k)] = ([np.frombuffer(bytes(b), '<u4').astype(np.uint32) for b in v.get('env_buffers', [])],
                            [np.frombuffer(bytes(b), '<u4').astype(np.uint32) for b in v.get('freq_buffers', [])])
            v = v['cmd_buf']
        progs[int(k)] = _to_u32(v)
    return progs, bufs


class ProgramSet:
    """cmd_mem images for every (group, core), packed for the device.

    groups: list of shots' programs (see ``_shot_programs``); group g runs for
    shots with (shot // shots_per_group) % n_groups == g.  Identical programs
    are stored once.
    """

    def __init__(self, groups: Sequence, cores_per_shot: Optional[int] = None):
        if isinstance(groups, dict):
            groups = [groups]
        parsed = [_shot_programs(g) for g in groups]
        per_group = [p for p, _ in parsed]
        # env / freq buffers of (group, core), when the programs came from an assembler
        self.buffers = {(g, c): b for g, (_, bs) in enumerate(parsed) for c, b in bs.items()}
        if not per_group:
            raise ValueError('no programs')
        ncore = max((max(g) + 1 if g else 1) for g in per_group)
        C_ = cores_per_shot or _next_pow2(ncore)
        if C_ < ncore or C_ & (C_ - 1) or C_ > _abi.MAX_CORES:
            raise ValueError('cores_per_shot must be a power of two >= {}'.format(ncore))
        uniq: Dict[bytes, int] = {}
        blobs: List[np.ndarray] = []
        table = np.zeros(len(per_group) * C_, np.uint32)
        empty = np.zeros((0, 4), np.uint32)
        for g, progs in enumerate(per_group):
            for c in range(C_):
                p = progs.get(c, empty)
                key = p.tobytes()
                if key not in uniq:
                    uniq[key] = len(blobs)
                    blobs.append(p)
                table[g * C_ + c] = uniq[key]
        self.cores_per_shot = C_
        self.n_groups = len(per_group)
        self.n_instr = np.array([len(b) for b in blobs], np.uint32)
        self.offsets = np.concatenate([[0], np.cumsum(self.n_instr)[:-1]]).astype(np.uint32)
        self.words = (np.concatenate(blobs) if sum(self.n_instr) else np.zeros((1, 4), np.uint32)).astype(np.uint32)
        self.words = np.ascontiguousarray(self.words)
        self.table = table

    @classmethod
    def from_arrays(cls, words, offsets, n_instr, table, n_groups, cores_per_shot, buffers=None):
        """A ProgramSet from packed arrays (the dpemu_load_programs layout):
        words (n, 4) u32, program p = words[offsets[p]:offsets[p] + n_instr[p]],
        table[g * C + c] = program of core c in group g.  For program tables
        too large to pass through assembler dicts (config 4: 2 * 10^5
        programs, workloads.config4_rb_set)."""
        self = cls.__new__(cls)
        C_ = int(cores_per_shot)
        if C_ < 1 or C_ & (C_ - 1) or C_ > _abi.MAX_CORES:
            raise ValueError('cores_per_shot must be a power of two in [1, 64]')
        self.words = np.ascontiguousarray(np.asarray(words, np.uint32).reshape(-1, 4))
        self.offsets = np.ascontiguousarray(offsets, np.uint32)
        self.n_instr = np.ascontiguousarray(n_instr, np.uint32)
        self.table = np.ascontiguousarray(table, np.uint32).reshape(-1)
        if len(self.offsets) != len(self.n_instr) or len(self.table) != int(n_groups) * C_:
            raise ValueError('offsets / n_instr / table sizes disagree')
        if len(self.n_instr) and (self.offsets.astype(np.uint64) + self.n_instr).max() > len(self.words):
            raise ValueError('a program runs past the end of words')
        if len(self.table) and self.table.max() >= len(self.n_instr):
            raise ValueError('table names a program that does not exist')
        self.cores_per_shot = C_
        self.n_groups = int(n_groups)
        self.buffers = buffers if buffers is not None else {}
        return self

    def program(self, group: int, core: int) -> np.ndarray:
        """(n, 4) u32 machine code of core ``core`` in group ``group``"""
        p = int(self.table[group * self.cores_per_shot + core])
        o = int(self.offsets[p])
        return self.words[o:o + int(self.n_instr[p])]

    @property
    def n_programs(self):
        return len(self.n_instr)

    def readout_freqs(self, drv_elem: int, lo_elem: int):
        """The DEMOD readout model's frequency tables (dpemu_load_readout_freqs):
        per program, word 0 of every entry of the readout drive element's and
        the LO element's freq_buffer (f / f_clk * 2^32, asmparse.py:64-86), from
        the assembler buffers of a (group, core) that runs it.  Returns (words,
        drv_off, drv_len, lo_off, lo_len); a program without buffers gets empty
        tables (its frequency words read 0)."""
        owner = {}
        for i, pr in enumerate(self.table):
            owner.setdefault(int(pr), (i // self.cores_per_shot, i % self.cores_per_shot))
        words, cache = [], {}
        off = np.zeros((2, self.n_programs), np.uint32)
        ln = np.zeros((2, self.n_programs), np.uint32)
        n = 0
        for pr in range(self.n_programs):
            b = self.buffers.get(owner[pr]) if pr in owner else None
            for k, e in enumerate((drv_elem, lo_elem)):
                f = b[1][e] if b is not None and e < len(b[1]) else np.zeros(0, np.uint32)
                key = (id(f), k) if len(f) else None
                if key is not None and key in cache:
                    off[k, pr], ln[k, pr] = cache[key]
                    continue
                fw = np.asarray(f, np.uint32)[0::16]
                off[k, pr], ln[k, pr] = n, len(fw)
                if key is not None:
                    cache[key] = (n, len(fw))
                words.append(fw)
                n += len(fw)
        w = np.concatenate(words).astype(np.uint32) if n else np.zeros(0, np.uint32)
        return w, off[0], ln[0], off[1], ln[1]


class EmulationResult:
    """Host copies of a run's outputs (layouts as in include/dpemu.h)."""

    def __init__(self, cfg, n_shots, shot_begin, arrays):
        self.cfg = cfg
        self.n_shots = n_shots
        self.shot_begin = shot_begin
        self.arrays = arrays
        self.summary = _abi.unpack_summary(arrays['summary'])

    @property
    def n_lanes(self):
        return self.n_shots * self.cfg.cores_per_shot

    def lane(self, shot, core):
        """output lane of (absolute shot, core) in the run's lane order (include/dpemu.h)"""
        return int(_abi.lane_index(shot - self.shot_begin, core, self.n_shots, self.cfg.cores_per_shot,
                                   self.cfg.lane_order))

    def events(self, shot, core) -> np.ndarray:
        """structured events of one lane: t, env_word, cfg, kind, phase, freq, amp"""
        L = self.lane(shot, core)
        n = min(int(self.summary['n_events'][L]), self.cfg.event_cap)
        return decode_events(self.arrays['events'][:n, L])

    def status_counts(self):
        st, n = np.unique(self.summary['status'], return_counts=True)
        return {_abi.STATUS_NAMES.get(int(s), str(s)): int(c) for s, c in zip(st, n)}

    @property
    def histogram(self):
        return self.arrays.get('hist')


def decode_events(ev) -> np.ndarray:
    """structured view of event records (..., 4) u32: t, env_word, cfg, kind,
    phase, freq, amp (the pulse_iface fields, hdl/pulse_iface.sv:2-6)"""
    ev = np.asarray(ev).view(np.uint32)
    out = np.zeros(ev.shape[:-1], dtype=[('t', 'u4'), ('env_word', 'u4'), ('cfg', 'u1'), ('kind', 'u1'),
                                         ('phase', 'u4'), ('freq', 'u2'), ('amp', 'u2')])
    out['t'] = ev[..., 0]
    out['env_word'] = ev[..., 1] & 0xFFFFFF
    out['cfg'] = (ev[..., 1] >> 24) & 0xF
    out['kind'] = ev[..., 1] >> 28
    out['phase'] = ev[..., 2] & 0x1FFFF
    out['freq'] = ev[..., 2] >> 17
    out['amp'] = ev[..., 3] & 0xFFFF
    return out


class Emulator:
    """One context per GPU (one process per device)."""

    def __init__(self, device: int = 0, lib_path: Optional[str] = None):
        self._L = load_library(lib_path) if lib_path else load_library()
        h = C.c_void_p()
        rc = self._L.dpemu_create(int(device), C.byref(h))
        if rc != 0:
            raise DpemuError('dpemu_create(device={}) failed ({}): no usable HIP device'.format(device, rc))
        self._h = h
        self.device = device
        self.lib_path = lib_path          # None: the in-tree build
        self.programs: Optional[ProgramSet] = None
        self._ro_key = None               # (drv_elem, lo_elem) of the loaded DEMOD tables

    def close(self):
        if getattr(self, '_h', None):
            self._L.dpemu_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # ---- measurement (dpemu_set_kernel_timing / dpemu_kernel_times) ----
    def kernel_timing(self, enable: bool = True):
        """record a HIP event pair around every main-kernel launch (interpreter, DDS)"""
        check(self._h, self._L.dpemu_set_kernel_timing(self._h, int(bool(enable))), 'dpemu_set_kernel_timing',
              self._L)

    def kernel_times(self, max_n: int = 4096):
        """elapsed ms of the launches recorded since the last call (waits for them)"""
        buf = np.zeros(max_n, np.float32)
        n = C.c_int(0)
        check(self._h, self._L.dpemu_kernel_times(self._h, buf.ctypes.data, int(max_n), C.byref(n)),
              'dpemu_kernel_times', self._L)
        return [float(x) for x in buf[:n.value]]

    def last_kernel(self) -> str:
        """the interpreter variant the last run launched"""
        return self._L.dpemu_last_kernel(self._h).decode()

    # -------------------------------------------------------------- programs
    def load(self, programs, cores_per_shot: Optional[int] = None) -> ProgramSet:
        ps = programs if isinstance(programs, ProgramSet) else ProgramSet(programs, cores_per_shot)
        rc = self._L.dpemu_load_programs(self._h, ps.words.ctypes.data, int(ps.words.shape[0]),
                                         ps.offsets.ctypes.data,
                                         ps.n_instr.ctypes.data, ps.n_programs, ps.table.ctypes.data,
                                         ps.n_groups, ps.cores_per_shot)
        check(self._h, rc, 'dpemu_load_programs', self._L)
        self.programs = ps
        self._ro_key = None                                 # load_programs clears the DEMOD tables
        return ps

    def load_readout_freqs(self, drv_elem: int, lo_elem: int, tables=None):
        """dpemu_load_readout_freqs: the DEMOD model's per-program frequency
        words -- ``tables`` = (words, drv_off, drv_len, lo_off, lo_len), default
        ProgramSet.readout_freqs(drv_elem, lo_elem) of the loaded programs"""
        if self.programs is None:
            raise DpemuError('load() programs first')
        t = tables if tables is not None else self.programs.readout_freqs(drv_elem, lo_elem)
        w = np.ascontiguousarray(t[0], np.uint32)
        arrs = [np.ascontiguousarray(a, np.uint32) for a in t[1:5]]
        if any(len(a) != self.programs.n_programs for a in arrs):
            raise DpemuError('readout tables need one entry per loaded program')
        rc = self._L.dpemu_load_readout_freqs(self._h, w.ctypes.data if len(w) else None, len(w),
                                              *[a.ctypes.data for a in arrs])
        check(self._h, rc, 'dpemu_load_readout_freqs', self._L)
        self._ro_key = (int(drv_elem), int(lo_elem)) if tables is None else ('caller', id(tables))

    def _demod_tables(self, cfg):
        """a DEMOD run reads the loaded programs' own frequency tables unless the
        caller loaded others"""
        if cfg.meas_model == _abi.MEAS_DEMOD and (self._ro_key is None or (
                self._ro_key[0] != 'caller' and self._ro_key != (cfg.ro_drv_elem, cfg.meas_elem))):
            self.load_readout_freqs(cfg.ro_drv_elem, cfg.meas_elem)

    def config(self, **kw) -> _abi.Config:
        if self.programs is None:
            raise DpemuError('load() programs first')
        kw.setdefault('n_groups', self.programs.n_groups)
        return _abi.make_config(self.programs.cores_per_shot, **kw)

    # -------------------------------------------------------------- running
    def _call(self, name, args, stream, states=None):
        """the asynchronous entry point ``name``(ctx, *args, stream); stream: torch.cuda.Stream / raw handle /
        None.  With ``states`` (a checked tensor) it is the ``_st`` entry point, which takes that tensor's
        pointer (null for an empty one) before the stream."""
        if states is not None:
            name, args = name + '_st', (*args, states.data_ptr() if states.numel() else None)
        s = getattr(stream, 'cuda_stream', stream)
        rc = getattr(self._L, name)(self._h, *args, C.c_void_p(s) if s else None)
        check(self._h, rc, name, self._L)

    def run(self, n_shots: int, shot_begin: int = 0, cfg: Optional[_abi.Config] = None,
            outputs: Iterable[str] = ('summary', 'events', 'meas', 'hist'), **cfg_kw) -> EmulationResult:
        """Emulate shots [shot_begin, shot_begin + n_shots); results copied to host."""
        cfg = cfg or self.config(**cfg_kw)
        self._demod_tables(cfg)
        want = set(outputs) | {'summary'}
        arrays = _abi.alloc_host_outputs(cfg, n_shots, want)
        o = _abi.outputs_struct(arrays)
        rc = self._L.dpemu_run_host(self._h, C.addressof(cfg), int(shot_begin), int(n_shots), C.addressof(o))
        check(self._h, rc, 'dpemu_run_host', self._L)
        return EmulationResult(cfg, n_shots, shot_begin, arrays)

    def run_device(self, cfg: _abi.Config, n_shots: int, shot_begin: int, outputs: dict, stream=None, states=None):
        """Asynchronous run into caller-owned device buffers: torch tensors
        {name: tensor} shaped as alloc_device_outputs makes them (checked: the
        C ABI takes bare pointers); stream: torch.cuda.Stream / raw handle / None.
        With ``states`` (dpemu_run_states; ``simulate_gates(measure=True)``'s
        int32 tensor [n_shots * C], or any in that layout) the prepared state of
        a lane's readout m is bit m of its word instead of the p1_threshold
        draw; DEMOD configs are refused."""
        if states is not None:                  # None: dpemu_run
            check_states_tensor(states, int(n_shots) * cfg.cores_per_shot, self.device)
            if cfg.meas_model == _abi.MEAS_DEMOD:
                raise DpemuError('dpemu_run_states: meas_model DEMOD with states (the *_st readout stages take the '
                                 'states of a DEMOD chain)')
        unknown = set(outputs) - set(_abi.OUTPUT_NAMES)
        if unknown:
            raise DpemuError('unknown outputs {}'.format(sorted(unknown)))
        want = device_output_specs(cfg, n_shots)
        o = _abi.Outputs()
        for name, _ in _abi.Outputs._fields_:
            t = outputs.get(name)
            if t is not None:
                _check_tensor(name, t, want[name], self.device)
            setattr(o, name, None if t is None else t.data_ptr())
        self._demod_tables(cfg)
        args = (C.addressof(cfg), int(shot_begin), int(n_shots), C.addressof(o))
        if states is None:
            self._call('dpemu_run', args, stream)
        else:                                   # (not an _st name: the states pointer goes the same place)
            self._call('dpemu_run_states', (*args, states.data_ptr() if states.numel() else None), stream)

    def cosimulate(self, cfg: _abi.Config, gateset, outputs: dict, n_shots: int, shot_begin: int = 0, states=None,
                   max_passes: Optional[int] = None, stream=None, t_final: int = 0):
        """Co-simulation of interpreter and qubits (DESIGN.md §2 "Co-simulation"):
        alternate ``run_device(states=)`` -- the interpreter with every readout's
        prepared state taken from a states buffer -- and
        ``simulate_gates(measure=True)`` -- the qubits under the pulses that run
        played, which writes the post-measurement states -- until the buffer
        reproduces itself.  That fixed point is unique, does not depend on the
        starting buffer (``states``, default zeros; not modified) and is reached
        within (distinct readout strobe times of a shot) + 1 passes;
        ``max_passes`` defaults to 32 * C + 1, one more than the state bits a
        shot has, and exceeding it raises DpemuError.  ``outputs``: the run's
        device tensors, ``summary`` and ``events`` among them; with ``hist``
        cfg.hist_assign must be 1 (every pass assigns, the last stands).
        A ``gateset`` with a decay (``GateSet.set_decay``) takes the qubit half
        through dpemu_qsim_decay, ``t_final`` with it; the fixed point and its
        bound are the same (an advance reads only records up to its own time).
        Returns (pops, result, states, passes): ``outputs`` holds the final
        run, which used the returned ``states``, and pops / result / states are
        ``simulate_gates(measure=True)``'s of that run."""
        import torch
        for k in ('summary', 'events'):
            if outputs.get(k) is None:
                raise DpemuError('cosimulate needs the {} output'.format(k))
        if outputs.get('hist') is not None and not cfg.hist_assign:
            raise DpemuError('cosimulate with a hist output needs cfg.hist_assign = 1: every pass counts the whole run')
        if cfg.meas_model == _abi.MEAS_DEMOD:
            raise DpemuError('dpemu_run_states: meas_model DEMOD with states (the *_st readout stages take the '
                             'states of a DEMOD chain)')
        n = int(n_shots) * cfg.cores_per_shot
        bound = 32 * cfg.cores_per_shot + 1 if max_passes is None else int(max_passes)
        if states is None:
            cur = torch.zeros((n,), dtype=torch.int32, device=torch.device('cuda', self.device))
        else:
            cur = check_states_tensor(states, n, self.device).clone()
        nxt = torch.empty_like(cur)
        pops = result = None
        # the buffers above and the compare below are torch's work: on the
        # caller's torch stream where it is one, else ordered by waiting
        on_torch = isinstance(stream, torch.cuda.Stream)
        raw = not on_torch and bool(getattr(stream, 'cuda_stream', stream))
        if on_torch:
            stream.wait_stream(torch.cuda.current_stream(cur.device))
        elif raw:
            torch.cuda.synchronize(self.device)
        for passes in range(1, bound + 1):
            self.run_device(cfg, n_shots, shot_begin, outputs, stream, states=cur)
            pops, result, nxt = self.simulate_gates(cfg, gateset, outputs, n_shots, shot_begin, pops, result, stream,
                                                    measure=True, states=nxt, t_final=t_final)
            if on_torch:
                with torch.cuda.stream(stream):
                    same = torch.equal(cur, nxt)
            else:
                if raw:
                    torch.cuda.synchronize(self.device)
                same = torch.equal(cur, nxt)
            if same:
                return pops, result, cur, passes
            cur, nxt = nxt, cur
        raise DpemuError('cosimulate: no fixed point within {} passes'.format(bound))

    def synthesize(self, plan, outputs: dict, n_samples: int, iq=None, stream=None):
        """DDS I/Q of every channel of ``plan`` (dds.ChannelPlan) from a device
        run's outputs (summary / ev_main / ev_amp tensors of run_device).
        Returns (or fills) an int32 device tensor [n_channels, n_samples]
        whose words hold I in the low and Q in the high 16 bits."""
        check_run_inputs('synthesize needs', outputs, plan.n_lanes, plan.event_cap, self.device)
        iq = tensor_or_new('iq', iq, dds_specs(plan, n_samples)['iq'], self.device)
        env, freq = plan.device_tables(outputs['summary'].device)
        ch = plan.struct(n_samples)
        self._call('dpemu_dds', (C.addressof(ch), outputs['summary'].data_ptr(), outputs['events'].data_ptr(),
                                 env.data_ptr(), freq.data_ptr(), iq.data_ptr()), stream)
        return iq

    def demodulate(self, cfg: _abi.Config, drv_plan, iq_drv, lo_plan, iq_lo, outputs: dict, acc=None, result=None,
                   stream=None, pairs=None):
        """Accumulated {I, Q} of every readout from the synthesised waveforms
        (dpemu_demod_iq, include/dpemu.h): row i of ``drv_plan`` / ``iq_drv``
        (the readout drive channels, element cfg.ro_drv_elem) is paired with
        row i of ``lo_plan`` / ``iq_lo`` (the LO channels, element
        cfg.meas_elem) of the same (shot, core); ``outputs`` are the run's
        summary / events device tensors.  ``pairs``: a dds.DemodPairTable
        built once for the two plans (default: built here).  Returns (acc int32
        [meas_cap, n_pairs, 2], result int32 [n_pairs, 2] = count, outcome
        bits) as device tensors."""
        from .dds import DemodPairTable
        pt = pairs if pairs is not None else DemodPairTable(cfg, drv_plan, lo_plan)
        acc, result = check_demod_tensors(pt, cfg, iq_drv, iq_lo, outputs, acc, result, self.device, alloc=True)
        st = pt.struct(cfg.meas_cap, iq_drv.shape[1], iq_lo.shape[1])
        self._call('dpemu_demod_iq', (C.addressof(cfg), C.addressof(st), outputs['summary'].data_ptr(),
                                      outputs['events'].data_ptr(), iq_drv.data_ptr(), iq_lo.data_ptr(),
                                      acc.data_ptr(), result.data_ptr()), stream)
        return acc, result

    def demodulate_plan(self, cfg: _abi.Config, plan, iq, outputs: dict, acc=None, result=None, stream=None):
        """``demodulate`` for one plan whose iq buffer holds both channels of
        every pair (dds.DemodPairTable.one_plan)."""
        from .dds import DemodPairTable
        return self.demodulate(cfg, plan, iq, plan, iq, outputs, acc, result, stream,
                               pairs=DemodPairTable.one_plan(cfg, plan))

    def feedline_adc(self, cfg: _abi.Config, lines, iq_drv, outputs: dict, n_samples_lo: int, adc=None, stream=None,
                     resonators=None, states=None):
        """The ADC trace of every feedline of ``lines`` (a dds.FeedlineTable;
        dpemu_feedline_adc, include/dpemu.h): the members' rotated, scaled
        drive returns from ``iq_drv`` (the drive plan's dpemu_dds rows),
        summed and clipped, one {I16 low, Q16 high} word per LO-rate sample.
        ``outputs`` are the run's summary / events device tensors.  With
        ``resonators`` (a dds.ResonatorTable of the same pair table) every
        member's return passes its state-dependent one-pole resonator and the
        converter adds per-sample noise (dpemu_feedline_adc_res).  With
        ``states`` (``simulate_gates(measure=True)``'s int32 tensor [n_lanes])
        the prepared state of readout m of a pair is bit m of its lane's word
        instead of the p1_threshold draw (the *_st entry points).  Returns
        (or fills) the int32 device tensor [n_lines, n_samples_lo]."""
        pt = lines.pairs
        if resonators is not None and resonators.pairs is not pt:
            raise DpemuError('the resonator table is of another pair table than the feedlines')
        adc = check_feedline_tensors(lines, cfg, outputs, self.device, iq_drv=iq_drv, adc=adc,
                                     n_samples_lo=n_samples_lo, alloc=True)[0]
        if states is not None:                  # None: the base entry points
            check_states_tensor(states, pt.n_lanes, self.device)
        st, ls = pt.struct(cfg.meas_cap, iq_drv.shape[1], int(n_samples_lo)), lines.struct()
        rs = resonators.struct() if resonators is not None else None
        self._call('dpemu_feedline_adc' if rs is None else 'dpemu_feedline_adc_res',
                   (C.addressof(cfg), C.addressof(st), C.addressof(ls), *([] if rs is None else [C.addressof(rs)]),
                    outputs['summary'].data_ptr(), outputs['events'].data_ptr(), iq_drv.data_ptr(), adc.data_ptr()),
                   stream, states)
        return adc

    def demodulate_feedline(self, cfg: _abi.Config, lines, iq_lo, outputs: dict, iq_drv=None, adc=None, acc=None,
                            result=None, stream=None, resonators=None, states=None):
        """``demodulate`` on the shared stream of every feedline of ``lines``
        (a dds.FeedlineTable; dpemu_demod_feedline, include/dpemu.h): each
        pair's LO row of ``iq_lo`` against its line's row of ``adc``, which
        this call makes with ``feedline_adc`` from ``iq_drv`` when no ``adc``
        tensor is passed (through ``resonators``, a dds.ResonatorTable, when
        one is given; ``states`` is passed on to that ADC stage -- the
        demodulator itself reads no state).  Returns (acc, result) as ``demodulate`` does; they
        feed ``iq_stats(..., pairs=lines.pairs)`` unchanged."""
        import torch
        pt = lines.pairs
        if adc is None:
            if iq_drv is None:
                raise DpemuError('demodulate_feedline needs the adc tensor or iq_drv to make it from')
            if not isinstance(iq_lo, torch.Tensor) or iq_lo.dim() != 2:
                raise DpemuError('iq_lo must be an int32 tensor [{}, n_samples]'.format(pt.n_rows[1]))
            adc = self.feedline_adc(cfg, lines, iq_drv, outputs, iq_lo.shape[1], stream=stream, resonators=resonators,
                                    states=states)
        elif resonators is not None or states is not None:
            raise DpemuError('resonators and states shape the adc trace this call makes: pass iq_drv, not adc')
        _, acc, result = check_feedline_tensors(lines, cfg, outputs, self.device, iq_lo=iq_lo, adc=adc, acc=acc,
                                                result=result, alloc=True)
        st, ls = pt.struct(cfg.meas_cap, 0, iq_lo.shape[1]), lines.struct()
        self._call('dpemu_demod_feedline', (C.addressof(cfg), C.addressof(st), C.addressof(ls),
                                            outputs['summary'].data_ptr(), outputs['events'].data_ptr(),
                                            adc.data_ptr(), iq_lo.data_ptr(), acc.data_ptr(), result.data_ptr()),
                   stream)
        return acc, result

    def feedline_traces(self, cfg: _abi.Config, lines, iq_lo, outputs: dict, adc, n_bins: int, bin_clocks: int = 1,
                        by_slot: bool = False, traces=None, stream=None, states=None):
        """Per-class sums of the demodulated readout traces (dpemu_feedline_traces,
        include/dpemu.h; read them with readout.ReadoutTraces): every LO
        sample of every kept readout's window, ``adc`` (the feedline traces of
        ``feedline_adc``, or a caller's) times the conjugate of the pair's LO
        row of ``iq_lo``, summed per (slot, core, prepared state) and bin of
        ``bin_clocks`` clocks from the readout's strobe.  ``lines`` is
        ``demodulate_feedline``'s dds.FeedlineTable, ``outputs`` the run's
        summary / events device tensors.  Returns (or fills) the int64 device
        tensor [S, C, 2, n_bins, TRACE_WORDS], S = meas_cap if by_slot else 1;
        it is assigned, not accumulated.  ``states``: as ``feedline_adc``'s --
        the classes' prepared states from the int32 tensor [n_lanes]
        (dpemu_feedline_traces_st)."""
        pt = lines.pairs
        traces = check_trace_tensors(lines, cfg, outputs, self.device, iq_lo, adc, n_bins, bin_clocks, by_slot, traces,
                                     alloc=True)
        if states is not None:                  # None: the base entry point
            check_states_tensor(states, pt.n_lanes, self.device)
        st, ls = pt.struct(cfg.meas_cap, 0, iq_lo.shape[1]), lines.struct()
        tb = _abi.TraceBins(int(n_bins), int(bin_clocks), 1 if by_slot else 0)
        self._call('dpemu_feedline_traces', (C.addressof(cfg), C.addressof(st), C.addressof(ls), C.addressof(tb),
                                             outputs['summary'].data_ptr(), outputs['events'].data_ptr(),
                                             adc.data_ptr(), iq_lo.data_ptr(), traces.data_ptr()), stream, states)
        return traces

    def iq_stats(self, cfg: _abi.Config, acc, counts, n_cols: Optional[int] = None, shot_begin: int = 0, pairs=None,
                 by_slot: bool = False, axis=None, thr=None, stats=None, bits=None, stream=None, states=None):
        """Per-class sums of an accumulator buffer (dpemu_iq_stats,
        include/dpemu.h; read them with readout.ReadoutStats).  ``acc``: int32
        device tensor [meas_cap, n_cols, 2] -- a DEMOD run's ``acc`` output or
        ``demodulate``'s.  ``counts``: the run's ``summary`` tensor [n_cols, 8]
        (its n_meas word) or a ``demodulate`` result tensor [n_cols, 2].
        Columns are the lanes of a run of n_cols / C shots from ``shot_begin``
        in cfg's lane order, or with ``pairs`` (a dds.DemodPairTable) the
        table's (shot, core) pairs.  ``axis`` / ``thr``: per-core Q15 axis
        words / thresholds (cores_per_shot each) instead of cfg.ro_axis and
        the single cfg.ro_thr.  ``bits``: None = no outcome bits, True = a new
        tensor, or an int32 tensor [n_cols] to fill.  ``states``: the classes'
        prepared states from an int32 tensor instead of the p1_threshold draw
        (dpemu_iq_stats_st), readout m in bit m -- [n_cols] words, a column
        being a lane; with ``pairs`` the run layout's [pairs.n_lanes] words
        (``simulate_gates(measure=True)``'s tensor as it is), gathered to the
        pairs' lanes here.  Returns (stats int64
        [S, C, 2, IQ_STAT_WORDS] with S = meas_cap if by_slot else 1, bits or
        None) as device tensors; stats is assigned, not accumulated."""
        import torch
        C_ = cfg.cores_per_shot
        n, stats, bits = check_iq_stats_tensors(cfg, acc, counts, n_cols, pairs, by_slot, stats, bits, self.device,
                                                alloc=True)
        st = _abi.IQColumns(n, int(acc.shape[0]), 1 if by_slot else 0, int(counts.shape[1]))
        st.shot_begin = int(shot_begin)
        keep = []                                           # host arrays the struct points into
        if pairs is not None:
            keep += [np.ascontiguousarray(pairs.cols['core'], np.uint32),
                     np.ascontiguousarray(pairs.cols['shot'], np.uint64)]
            st.core, st.shot = keep[0].ctypes.data, keep[1].ctypes.data
        for name, v, dt in (('axis', axis, np.uint32), ('thr', thr, np.int32)):
            if v is None:
                continue
            a = np.asarray(v, np.int64)
            if a.shape != (C_,) or a.min() < np.iinfo(dt).min or a.max() > np.iinfo(dt).max:
                raise DpemuError('{} must hold cores_per_shot = {} {} values'.format(name, C_, np.dtype(dt).name))
            keep.append(np.ascontiguousarray(a, dt))
            setattr(st, name, keep[-1].ctypes.data)
        off = 5 if counts.shape[1] == 8 else 0              # summary: n_meas is word 5; result: the count is word 0
        if states is not None:                  # None: the base entry point
            if pairs is not None:               # the run layout's words: gather the pairs' lanes
                check_states_tensor(states, pairs.n_lanes, self.device)
                lanes = torch.as_tensor(np.ascontiguousarray(pairs.cols['lane'], np.int64), device=states.device)
                states = states[lanes].contiguous()
            check_states_tensor(states, n, self.device)
        self._call('dpemu_iq_stats', (C.addressof(cfg), C.addressof(st), acc.data_ptr() if n else None,
                                      counts.data_ptr() + 4 * off if n else None, stats.data_ptr(),
                                      bits.data_ptr() if bits is not None and n else None), stream, states)
        return stats, bits

    def simulate_gates(self, cfg: _abi.Config, gateset, outputs: dict, n_shots: int, shot_begin: int = 0, pops=None,
                       result=None, stream=None, measure: bool = False, states=None, t_final: int = 0,
                       decay_counts=None):
        """Qubit states from the drive pulses of a run (dpemu_qsim,
        include/dpemu.h): every (register, shot) row's state vector evolved
        through the gates ``gateset`` (a qsim.GateSet: dictionary, registers,
        detunings) assigns to the drive strobes in ``outputs`` -- the summary /
        events device tensors of the run of ``n_shots`` shots from
        ``shot_begin`` under ``cfg``.  Returns (or fills) the device tensors
        pops int64 [n_regs, n_shots, 4] (Q60 populations of |b_first
        b_second>) and result int32 [n_regs, n_shots, 4] = {sampled outcome,
        n_gates, n_unmatched, n_errors mod 2^16 | overflow << 31}.  With
        ``measure`` (dpemu_qsim_meas) the strobes of element cfg.meas_elem
        measure their core's qubit -- sample, collapse, renormalise -- and the
        call returns (pops, result, states): ``states`` int32 [n_lanes], the
        post-measurement bit of a lane's readout m in bit m, which the readout
        stages take as ``states=``.  A ``gateset`` with a decay
        (``GateSet.set_decay``) takes the call through dpemu_qsim_decay: every
        qubit relaxes and dephases over the clocks between the strobes that
        act on it and, with ``t_final`` != 0, up to that clock before pops are
        taken; ``decay_counts``, an int32 device tensor [n_regs, n_shots, 4],
        receives every row's {jumps, flips} of its first and second qubit.
        The returned tuple is the same."""
        import torch
        if states is not None and not measure:
            raise DpemuError('states is the output of measure=True')
        decay = bool(getattr(gateset, 'decay', None))
        if not decay and (int(t_final) or decay_counts is not None):
            raise DpemuError('t_final and decay_counts need a gate set with a decay (GateSet.set_decay)')
        pops, result = check_qsim_tensors(cfg, gateset, outputs, n_shots, self.device, pops, result, alloc=True)
        if measure:
            states = check_states_tensor(states, int(n_shots) * cfg.cores_per_shot, self.device, alloc=True)
        if decay_counts is not None and int(n_shots):
            _check_tensor('decay_counts', decay_counts, qsim_decay_specs(gateset.n_regs, int(n_shots))['counts'],
                          self.device)
        st, keep = gateset.struct(cfg, n_shots, shot_begin)     # (keep: the host arrays st points into)
        if int(n_shots):
            ptrs = [outputs['summary'].data_ptr(), outputs['events'].data_ptr(), pops.data_ptr(), result.data_ptr()]
            if measure:
                ptrs.append(states.data_ptr())
        else:                                   # nothing is read or written: the tables are checked all the same
            hold = torch.empty((4,), dtype=torch.int32, device=torch.device('cuda', self.device))
            ptrs = [hold.data_ptr()] * (5 if measure else 4)
        if decay:                               # dec after qs; states (NULL: no readouts) and counts before the stream
            dec, keep_dec = gateset.decay_struct(cfg, t_final)
            tail = [None] * (5 - len(ptrs)) + [decay_counts.data_ptr() if decay_counts is not None and int(n_shots) else None]
            self._call('dpemu_qsim_decay', (C.addressof(cfg), C.addressof(st), C.addressof(dec), *ptrs, *tail), stream)
        else:
            self._call('dpemu_qsim_meas' if measure else 'dpemu_qsim', (C.addressof(cfg), C.addressof(st), *ptrs), stream)
        return (pops, result, states) if measure else (pops, result)


class RunPipeline:
    """Successive device runs with ``depth`` batches in flight.

    One context runs its calls in call order (dpemu.h), so batch k + 1's
    launch cannot start before batch k's kernel has drained.  A launch whose
    waves run programs of different lengths (config 4: each wave holds ~7
    RB sequences) has a long tail in which most of the GPU idles; the
    pipeline holds ``depth`` contexts with the same programs loaded, one
    stream and one output set each, and sends batch k to context k % depth,
    so batch k + 1's waves fill the CUs batch k's tail leaves idle (config 4:
    3.65 -> 2.86 ms per batch at depth 2, ``profiles/r03_pipe_probe.json``).

    ``streams``: the caller's streams (default: new ones from torch's pool).
    Streams beyond the process's hardware queues (GPU_MAX_HW_QUEUES, 4 by
    default) share queues, and kernels on one queue run in turn: a pipeline
    whose streams were created after many others measured no overlap at all
    in bench.py (3.60 ms per batch), the same on the first streams of the
    process 2.79 -- so the bench makes its pipeline streams first.

    ``launch(cfg, n_shots, shot_begin, hist=None)`` makes the slot's stream
    wait for the caller's current stream, runs the batch there (into
    ``hist`` instead of the slot's own histogram when given) and returns
    (outputs, stream); the outputs are valid on that stream and are
    overwritten by the launch ``depth`` batches later.  ``drain()`` waits
    for every batch.  Memory: ``depth`` output sets and program images.
    """

    def __init__(self, programs, cfg: _abi.Config, n_shots: int, want=('summary', 'events', 'meas', 'hist'),
                 depth: int = 2, device: int = 0, first: Optional['Emulator'] = None, streams=None,
                 lib_path: Optional[str] = None):
        import torch
        if depth < 1:
            raise ValueError('depth must be >= 1')
        if streams is not None and len(streams) < depth:
            raise ValueError('need {} streams, got {}'.format(depth, len(streams)))
        self.emus, self._own = [], []
        # every context on ONE library: the caller's, else first's (an A/B
        # build passed as first=Emulator(0, lib_path=...) stays alone)
        if lib_path is None and first is not None:
            lib_path = first.lib_path
        try:
            for j in range(depth):
                if j == 0 and first is not None:
                    e = first                                  # the caller's context, programs loaded
                else:
                    e = Emulator(device, lib_path=lib_path)
                    self._own.append(e)
                    e.load(programs)
                self.emus.append(e)
        except Exception:
            self.close()
            raise
        self.device = torch.device('cuda', device)
        # streams: the caller's (e.g. created once at start-up, each on its own
        # hardware queue: streams that share a queue run their kernels in turn)
        self.streams = list(streams[:depth]) if streams is not None else \
            [torch.cuda.Stream(device=self.device) for _ in range(depth)]
        self.outputs = [alloc_device_outputs(cfg, n_shots, want=want, device=self.device) for _ in range(depth)]
        self.k = 0

    def launch(self, cfg: _abi.Config, n_shots: int, shot_begin: int, hist=None):
        import torch
        j = self.k % len(self.emus)
        s = self.streams[j]
        s.wait_stream(torch.cuda.current_stream(self.device))
        out = self.outputs[j]
        if hist is not None:
            out = dict(out, hist=hist)
        self.emus[j].run_device(cfg, n_shots, shot_begin, out, s)
        self.k += 1
        return out, s

    def drain(self):
        for s in self.streams:
            s.synchronize()

    def close(self):
        for e in self._own:
            e.close()
        self._own, self.emus = [], []


def device_output_specs(cfg: _abi.Config, n_shots: int):
    """{name: (shape, torch dtype)} of the dpemu_outputs arrays of a run"""
    import torch
    n_lanes = int(n_shots) * cfg.cores_per_shot
    return {'summary': ((n_lanes, 8), torch.int32), 'events': ((cfg.event_cap, n_lanes, 4), torch.int32),
            'trace': ((cfg.trace_cap, n_lanes, 4), torch.int32),
            'meas': ((cfg.meas_cap, n_lanes, 2), torch.int32), 'regs': ((16, n_lanes), torch.int32),
            'hist': ((cfg.n_groups, 1 << cfg.cores_per_shot), torch.int64),
            'hist_next': ((cfg.n_groups, 1 << cfg.cores_per_shot), torch.int64),   # zeroed by the run
            'acc': ((cfg.meas_cap, n_lanes, 2), torch.int32)}                    # DEMOD runs only


def alloc_device_outputs(cfg: _abi.Config, n_shots: int, want=('summary', 'events', 'meas', 'hist'),
                         device='cuda'):
    """torch device tensors laid out as dpemu_outputs."""
    import torch
    shapes = device_output_specs(cfg, n_shots)
    out = {}
    for k in want:
        shp, dt = shapes[k]
        if k in ('hist', 'hist_next'):
            if cfg.cores_per_shot > 12:
                continue
            out[k] = torch.zeros(shp, dtype=dt, device=device)
        elif 0 not in shp:
            out[k] = torch.empty(shp, dtype=dt, device=device)
    return out
