"""The Python half of the stage calls, without a GPU: what the stage check
functions refuse and in which words, what Emulator's methods hand to each C
entry point, the check-or-allocate helper, and the signature table of
_native against include/dpemu.h.

The tensors are tests/test_output_checks.py's fake-device tensors (CPU
storage that reports cuda:<index>), shaped after the hand-built case
``edge_four_samples`` (3 pairs on 3 lanes, 2 lines, 4 LO samples, meas_cap 4,
4 cores, event_cap 16) and, where whole shots are needed, a run of 3 shots of
the same configuration (12 lanes).  The library is a stub that records every
dpemu_* call, so every pointer and struct field can be compared with what
the method was given."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest
import torch

from distributed_processor_amd import _abi, _native
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.dds import DESC_FIELDS, ChannelPlan, DemodPairTable, FeedlineTable, ResonatorTable
from distributed_processor_amd.emulator import Emulator
from distributed_processor_amd.qsim import GateSet
from distributed_processor_amd.stage_tensors import (
    check_demod_tensors, check_feedline_tensors, check_iq_stats_tensors, check_qsim_tensors, check_states_tensor,
    check_tensor, check_trace_tensors)
from tests import handbuilt as hb
from tests.test_output_checks import _dev

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I32, I64 = torch.int32, torch.int64


def z(shape, dtype=I32, index=0):
    return _dev(torch.zeros(shape, dtype=dtype), index)


def with_cfg(cfg, **kw):
    c = type(cfg).from_buffer_copy(cfg)
    for k, v in kw.items():
        setattr(c, k, v)
    return c


def case():
    c = hb.case('edge_four_samples')
    assert (c.pt.n_pairs, c.pt.n_lanes, c.pt.event_cap, c.pt.n_rows, c.ft.n_lines, c.n_lo) == (3, 3, 16, (3, 3), 2, 4)
    assert (c.cfg.meas_cap, c.cfg.cores_per_shot) == (4, 4)
    return c


def run_outputs(n_lanes=3):
    return {'summary': z((n_lanes, 8)), 'events': z((16, n_lanes, 4))}


def refused(fn, args, faults):
    """``fn(**args)`` passes; with each (changes, message) of ``faults`` applied it raises exactly that message"""
    fn(**args)
    for changes, message in faults:
        with pytest.raises(DpemuError) as e:
            fn(**dict(args, **changes))
        assert str(e.value) == message, (changes, str(e.value))


def without(d, k):
    return {n: v for n, v in d.items() if n != k}


# ---- the messages ----------------------------------------------------------------------------------------------
def test_check_tensor_precedence():
    """device before dtype before contiguity before size"""
    spec = ((4, 6), I32)
    for t, message in ((_dev(torch.zeros((6, 4), dtype=torch.int16).t(), 1),
                        'x: tensor on cuda:1 but the emulator runs on cuda:0'),
                       (z((6, 4), torch.int16).t(), 'x: dtype torch.int16 (want torch.int32)'),
                       (z((6, 5)).t(), 'x: tensor must be contiguous'),
                       (z((4, 5)), 'x: 20 elements, the run writes 24 ((4, 6))')):
        with pytest.raises(DpemuError) as e:
            check_tensor('x', t, spec, 0)
        assert str(e.value) == message


def test_demod_messages():
    c = case()
    out = run_outputs()
    args = dict(pt=c.pt, cfg=c.cfg, iq_drv=z((3, 12)), iq_lo=z((3, 4)), outputs=out, acc=z((4, 3, 2)),
                result=z((3, 2)), device=0)
    iq = '{} must be an int32 tensor [3, n_samples]'
    refused(check_demod_tensors, args, [
        (dict(cfg=with_cfg(c.cfg, meas_cap=0)), 'demodulate needs cfg.meas_cap in [1, 32]'),
        (dict(cfg=with_cfg(c.cfg, meas_cap=33)), 'demodulate needs cfg.meas_cap in [1, 32]'),
        (dict(outputs=without(out, 'summary')), 'demodulate needs the run\'s summary output'),
        (dict(outputs=without(out, 'events')), 'demodulate needs the run\'s events output'),
        (dict(iq_drv=None), iq.format('iq_drv')),
        (dict(iq_drv=z((12,))), iq.format('iq_drv')),
        (dict(iq_drv=z((2, 12))), iq.format('iq_drv')),
        (dict(iq_drv=z((3, 0))), iq.format('iq_drv')),
        (dict(iq_lo=[0] * 4), iq.format('iq_lo')),
        (dict(iq_lo=z((4, 4))), iq.format('iq_lo')),
        (dict(iq_lo=z((3, 6))), 'iq_lo: n_samples 6 is not a multiple of 4'),
        (dict(outputs=dict(out, summary=z((2, 8)))), 'summary: 16 elements, the run writes 24 ((3, 8))'),
        (dict(outputs=dict(out, events=z((15, 3, 4)))), 'events: 180 elements, the run writes 192 ((16, 3, 4))'),
        (dict(outputs=dict(out, events=z((16, 3, 4), torch.float32))),
         'events: dtype torch.float32 (want torch.int32)'),
        (dict(iq_drv=z((3, 12), torch.int16)), 'iq_drv: dtype torch.int16 (want torch.int32)'),
        (dict(iq_lo=z((3, 4), index=1)), 'iq_lo: tensor on cuda:1 but the emulator runs on cuda:0'),
        (dict(iq_lo=z((4, 3)).t()), 'iq_lo: tensor must be contiguous'),
        (dict(acc=z((3, 3, 2))), 'acc: 18 elements, the run writes 24 ((4, 3, 2))'),
        (dict(acc=z((2, 3, 4)).permute(2, 1, 0)), 'acc: tensor must be contiguous'),
        (dict(result=z((3,))), 'result: 3 elements, the run writes 6 ((3, 2))'),
        (dict(result=torch.zeros((3, 2), dtype=I32)), 'result: tensor on cpu but the emulator runs on cuda:0'),
        # two faults
        (dict(cfg=with_cfg(c.cfg, meas_cap=0), outputs=without(out, 'events')),
         'demodulate needs cfg.meas_cap in [1, 32]'),
        (dict(outputs=without(out, 'events'), iq_drv=z((2, 12))), 'demodulate needs the run\'s events output'),
        (dict(iq_lo=z((2, 6))), iq.format('iq_lo')),
        (dict(outputs=dict(out, summary=z((2, 8))), acc=z((3, 3, 2))),
         'summary: 16 elements, the run writes 24 ((3, 8))'),
        (dict(acc=z((3, 3, 2)), result=z((3,))), 'acc: 18 elements, the run writes 24 ((4, 3, 2))'),
    ])
    check_demod_tensors(**dict(args, acc=None, result=None))


def test_feedline_messages():
    c = case()
    out = run_outputs()
    iq = '{} must be an int32 tensor [3, n_samples]'
    shared = [
        (dict(cfg=with_cfg(c.cfg, meas_cap=0)), 'the feedline stages need cfg.meas_cap in [1, 32]'),
        (dict(cfg=with_cfg(c.cfg, meas_cap=33)), 'the feedline stages need cfg.meas_cap in [1, 32]'),
        (dict(outputs=without(out, 'summary')), 'the feedline stages need the run\'s summary output'),
        (dict(outputs=without(out, 'events')), 'the feedline stages need the run\'s events output'),
        (dict(outputs=dict(out, summary=z((3, 8), I64))), 'summary: dtype torch.int64 (want torch.int32)'),
        (dict(outputs=dict(out, events=z((16, 2, 4)))), 'events: 128 elements, the run writes 192 ((16, 3, 4))'),
        (dict(adc=[0]), 'adc must be an int32 tensor [2, 4]'),
        (dict(adc=z((3, 4))), 'adc must be an int32 tensor [2, 4]'),
        (dict(adc=z((2, 8))), 'adc must be an int32 tensor [2, 4]'),
        (dict(adc=z((2, 4), torch.int16)), 'adc: dtype torch.int16 (want torch.int32)'),
        (dict(adc=z((2, 4), index=1)), 'adc: tensor on cuda:1 but the emulator runs on cuda:0'),
        (dict(cfg=with_cfg(c.cfg, meas_cap=0), outputs=without(out, 'events')),
         'the feedline stages need cfg.meas_cap in [1, 32]'),
    ]
    # the ADC stage: iq_drv, n_samples_lo, adc
    args = dict(lines=c.ft, cfg=c.cfg, outputs=out, device=0, iq_drv=z((3, 4)), adc=z((2, 4)), n_samples_lo=4)
    refused(check_feedline_tensors, args, shared + [
        (dict(iq_drv=z((4,))), iq.format('iq_drv')),
        (dict(iq_drv=z((4, 4))), iq.format('iq_drv')),
        (dict(iq_drv=z((3, 0))), iq.format('iq_drv')),
        (dict(iq_drv=z((3, 4), torch.float32)), 'iq_drv: dtype torch.float32 (want torch.int32)'),
        (dict(n_samples_lo=0, adc=None), 'n_samples_lo 0 is not a nonzero multiple of 4'),
        (dict(n_samples_lo=6, adc=None), 'n_samples_lo 6 is not a nonzero multiple of 4'),
        (dict(n_samples_lo=8), 'adc must be an int32 tensor [2, 8]'),
        (dict(iq_drv=z((2, 4)), n_samples_lo=6), iq.format('iq_drv')),
    ])
    check_feedline_tensors(**dict(args, adc=None))
    check_feedline_tensors(**dict(args, lines=FeedlineTable(c.pt, [[1], [2]])))     # pair 0 in no line: ignored here
    # the demodulator: iq_lo, adc, acc, result
    args = dict(lines=c.ft, cfg=c.cfg, outputs=out, device=0, iq_lo=z((3, 4)), adc=z((2, 4)), acc=z((4, 3, 2)),
                result=z((3, 2)))
    refused(check_feedline_tensors, args, shared + [
        (dict(iq_lo=z((2, 4))), iq.format('iq_lo')),
        (dict(iq_lo=z((3, 4), torch.int16)), 'iq_lo: dtype torch.int16 (want torch.int32)'),
        (dict(iq_lo=z((3, 6))), 'n_samples_lo 6 is not a nonzero multiple of 4'),
        (dict(lines=FeedlineTable(c.pt, [[1], [2]])), 'pair 0 is in no line'),
        (dict(acc=z((4, 3, 1))), 'acc: 12 elements, the run writes 24 ((4, 3, 2))'),
        (dict(result=z((3, 2), torch.int16)), 'result: dtype torch.int16 (want torch.int32)'),
        (dict(result=z((2, 2))), 'result: 4 elements, the run writes 6 ((3, 2))'),
        (dict(iq_lo=z((2, 6))), iq.format('iq_lo')),
        (dict(outputs=dict(out, summary=z((2, 8))), acc=z((4, 3, 1))),
         'summary: 16 elements, the run writes 24 ((3, 8))'),
        (dict(adc=z((2, 8)), acc=z((4, 3, 1))), 'adc must be an int32 tensor [2, 4]'),
    ])
    check_feedline_tensors(**dict(args, acc=None, result=None))


def test_trace_messages():
    c = case()
    out = run_outputs()
    args = dict(lines=c.ft, cfg=c.cfg, outputs=out, device=0, iq_lo=z((3, 4)), adc=z((2, 4)), n_bins=10, bin_clocks=3,
                by_slot=True, traces=z((4, 4, 2, 10, 4), I64))
    top = 2 ** 31 // (3 * 4 * 16)
    refused(check_trace_tensors, args, [
        (dict(iq_lo=None), 'feedline_traces needs the iq_lo and adc tensors'),
        (dict(adc=None), 'feedline_traces needs the iq_lo and adc tensors'),
        (dict(outputs=without(out, 'events')), 'the feedline stages need the run\'s events output'),
        (dict(adc=z((1, 4))), 'adc must be an int32 tensor [2, 4]'),
        (dict(n_bins=0), 'n_bins 0 not in [1, 4096]'),
        (dict(n_bins=4097), 'n_bins 4097 not in [1, 4096]'),
        (dict(bin_clocks=0), 'bin_clocks 0 must be >= 1'),
        (dict(bin_clocks=2 ** 32), 'bin_clocks 4294967296 must be >= 1'),
        (dict(bin_clocks=top + 1), 'n_pairs * meas_cap * bin_clocks * 16 = {} exceeds 2^31'.format(192 * (top + 1))),
        (dict(by_slot=False), 'traces: 1280 elements, the run writes 320 ((1, 4, 2, 10, 4))'),
        (dict(n_bins=11), 'traces: 1280 elements, the run writes 1408 ((4, 4, 2, 11, 4))'),
        (dict(traces=z((4, 4, 2, 10, 4))), 'traces: dtype torch.int32 (want torch.int64)'),
        # two faults
        (dict(n_bins=0, traces=z((4, 4, 2, 9, 4), I64)), 'n_bins 0 not in [1, 4096]'),
        (dict(n_bins=4097, bin_clocks=0), 'n_bins 4097 not in [1, 4096]'),
        (dict(iq_lo=z((3, 6)), n_bins=0), 'n_samples_lo 6 is not a nonzero multiple of 4'),
    ])
    check_trace_tensors(**dict(args, bin_clocks=top, by_slot=False, traces=z((1, 4, 2, 10, 4), I64)))


def test_iq_stats_messages():
    c = case()
    acc_msg = 'acc must be an int32 tensor [meas_cap in 1..32, n_cols, 2]'
    counts_msg = 'counts must be a run\'s summary [n_cols, 8] or a demodulate result [n_cols, 2]'
    args = dict(cfg=c.cfg, acc=z((4, 8, 2)), counts=z((8, 8)), n_cols=None, pairs=None, by_slot=False,
                stats=z((1, 4, 2, 16), I64), bits=z((8,)), device=0)
    wide = _dev(torch.zeros((1, 1, 1), dtype=I32).expand(32, 2 ** 26 + 4, 2))
    refused(check_iq_stats_tensors, args, [
        (dict(acc=[0]), acc_msg),
        (dict(acc=z((4, 16))), acc_msg),
        (dict(acc=z((4, 8, 3))), acc_msg),
        (dict(acc=z((33, 8, 2))), acc_msg),
        (dict(acc=z((0, 8, 2))), acc_msg),
        (dict(n_cols=7), 'acc has 8 columns, n_cols = 7'),
        (dict(acc=wide), 'n_cols * meas_cap = {} exceeds 2^31'.format(32 * (2 ** 26 + 4))),
        (dict(counts=None), counts_msg),
        (dict(counts=z((8,))), counts_msg),
        (dict(counts=z((8, 4))), counts_msg),
        (dict(pairs=c.pt), 'acc has 8 columns, the pair table 3 pairs'),
        (dict(acc=z((4, 3, 2))), 'acc has 3 columns: not a whole number of 4-core shots'),
        (dict(acc=z((4, 8, 2), torch.float32)), 'acc: dtype torch.float32 (want torch.int32)'),
        (dict(acc=z((4, 2, 8)).transpose(1, 2)), 'acc: tensor must be contiguous'),
        (dict(counts=z((7, 8))), 'counts: 56 elements, the run writes 64 ((8, 8))'),
        (dict(counts=z((7, 2))), 'counts: 14 elements, the run writes 16 ((8, 2))'),
        (dict(counts=z((8, 2), index=1)), 'counts: tensor on cuda:1 but the emulator runs on cuda:0'),
        (dict(acc=z((4, 0, 2)), counts=z((3, 2))), 'counts: 3 rows for 0 columns'),
        (dict(stats=z((4, 4, 2, 16), I64)), 'stats: 512 elements, the run writes 128 ((1, 4, 2, 16))'),
        (dict(by_slot=True), 'stats: 128 elements, the run writes 512 ((4, 4, 2, 16))'),
        (dict(stats=z((1, 4, 2, 16))), 'stats: dtype torch.int32 (want torch.int64)'),
        (dict(bits=z((7,))), 'bits: 7 elements, the run writes 8 ((8,))'),
        (dict(bits=z((8,), torch.int16)), 'bits: dtype torch.int16 (want torch.int32)'),
        # two faults
        (dict(acc=z((4, 8, 3)), counts=z((8, 4))), acc_msg),
        (dict(acc=z((4, 3, 2)), n_cols=4), 'acc has 3 columns, n_cols = 4'),
        (dict(counts=z((8, 4)), pairs=c.pt), counts_msg),
        (dict(counts=z((7, 8)), stats=z((1, 4, 2, 16))), 'counts: 56 elements, the run writes 64 ((8, 8))'),
    ])
    for ok in (dict(n_cols=8, counts=z((8, 2)), bits=None), dict(stats=None, bits=None),
               dict(acc=z((4, 3, 2)), counts=z((3, 2)), pairs=c.pt, bits=z((3,))),
               dict(acc=z((2, 8, 2)), by_slot=True, stats=z((2, 4, 2, 16), I64)),
               # no columns: no storage to check, on any device
               dict(acc=torch.zeros((4, 0, 2), dtype=I32), counts=torch.zeros((0, 8), dtype=I32), bits=z((5,)))):
        check_iq_stats_tensors(**dict(args, **ok))


def test_states_messages():
    shape_msg = 'states must be an int32 tensor [12]'
    refused(check_states_tensor, dict(states=z((12,)), n=12, device=0), [
        (dict(states=[0] * 12), shape_msg),
        (dict(states=z((12, 1))), shape_msg),
        (dict(states=z((11,))), shape_msg),
        (dict(states=z((12,), torch.float32)), 'states: dtype torch.float32 (want torch.int32)'),
        (dict(states=z((12,), torch.uint8)), 'states: dtype torch.uint8 (want torch.int32)'),
        (dict(states=torch.zeros(12, dtype=I32)), 'states: tensor on cpu but the emulator runs on cuda:0'),
        (dict(states=z((12,), index=1)), 'states: tensor on cuda:1 but the emulator runs on cuda:0'),
        (dict(states=z((24,))[::2]), 'states: tensor must be contiguous'),
        (dict(states=z((11,), torch.float32)), shape_msg),
    ])
    check_states_tensor(torch.zeros(0, dtype=I32), 0, 0)              # n = 0: any empty int32 tensor
    with pytest.raises(DpemuError) as e:
        check_states_tensor(torch.zeros(0, dtype=I64), 0, 0)
    assert str(e.value) == 'states: dtype torch.int64 (want torch.int32)'


def gates():
    return GateSet(drv_elem=0).registers([(0, 1), 2])


def test_qsim_messages():
    c = case()
    out = run_outputs(12)
    args = dict(cfg=c.cfg, gateset=gates(), outputs=out, n_shots=3, device=0, pops=z((2, 3, 4), I64),
                result=z((2, 3, 4)))
    refused(check_qsim_tensors, args, [
        (dict(n_shots=-1), 'n_regs * n_shots = 2 * -1 must be in [0, 2^31]'),
        (dict(n_shots=2 ** 30 + 1), 'n_regs * n_shots = 2 * 1073741825 must be in [0, 2^31]'),
        (dict(outputs=without(out, 'summary')), 'simulate_gates needs the run\'s summary output'),
        (dict(outputs=without(out, 'events')), 'simulate_gates needs the run\'s events output'),
        (dict(outputs=run_outputs(3)), 'summary: 24 elements, the run writes 96 ((12, 8))'),
        (dict(outputs=dict(out, events=z((8, 12, 4)))), 'events: 384 elements, the run writes 768 ((16, 12, 4))'),
        (dict(outputs=dict(out, events=z((16, 12, 4), index=2))),
         'events: tensor on cuda:2 but the emulator runs on cuda:0'),
        (dict(pops=z((2, 3, 4))), 'pops: dtype torch.int32 (want torch.int64)'),
        (dict(pops=z((2, 1, 4), I64)), 'pops: 8 elements, the run writes 24 ((2, 3, 4))'),
        (dict(result=z((2, 3, 4), I64)), 'result: dtype torch.int64 (want torch.int32)'),
        (dict(result=z((3, 3, 4))), 'result: 36 elements, the run writes 24 ((2, 3, 4))'),
        # two faults
        (dict(outputs=without(out, 'summary'), pops=z((2, 3, 4))), 'simulate_gates needs the run\'s summary output'),
        (dict(outputs=without(out, 'events'), n_shots=-1), 'n_regs * n_shots = 2 * -1 must be in [0, 2^31]'),
        (dict(pops=z((2, 3, 4)), result=z((3, 3, 4))), 'pops: dtype torch.int32 (want torch.int64)'),
    ])
    check_qsim_tensors(**dict(args, pops=None, result=None))
    check_qsim_tensors(**dict(args, n_shots=0, outputs={}, pops=z((7,)), result=None))   # no shots: nothing is checked


# ---- the calls -------------------------------------------------------------------------------------------------
STRUCT_ARGS = {      # entry point -> {argument index: the struct it points to}
    'dpemu_run': {1: _abi.Config, 4: _abi.Outputs},
    'dpemu_dds': {1: _abi.DDSChannels},
    'dpemu_demod_iq': {2: _abi.DemodPairs},
    'dpemu_feedline_adc': {2: _abi.DemodPairs, 3: _abi.Feedlines},
    'dpemu_feedline_adc_res': {2: _abi.DemodPairs, 3: _abi.Feedlines, 4: _abi.Resonators},
    'dpemu_demod_feedline': {2: _abi.DemodPairs, 3: _abi.Feedlines},
    'dpemu_feedline_traces': {2: _abi.DemodPairs, 3: _abi.Feedlines, 4: _abi.TraceBins},
    'dpemu_iq_stats': {2: _abi.IQColumns},
    'dpemu_qsim': {2: _abi.Qsim},
    'dpemu_qsim_meas': {2: _abi.Qsim},
}


class StubLibrary:
    """stands in for the ctypes handle of libdpemu.so: every dpemu_* call returns 0 and is recorded as (name,
    arguments, {index: the fields of the struct that argument pointed to}); a stream handle is recorded as
    its integer"""

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith('dpemu_'):
            raise AttributeError(name)

        def call(*args):
            base = name[:-3] if name.endswith('_st') else name
            structs = {}
            for i, tp in STRUCT_ARGS.get(base, {}).items():
                s = tp.from_address(args[i])
                structs[i] = {f: getattr(s, f) for f, _ in tp._fields_ if not isinstance(getattr(s, f), C.Array)}
            stream = args[-1].value if isinstance(args[-1], C.c_void_p) else args[-1]
            self.calls.append((name, list(args[:-1]) + [stream], structs))
            return 0
        return call


STREAMS = ((None, None), (0x5A5A00, 0x5A5A00), (types.SimpleNamespace(cuda_stream=0x77AA00), 0x77AA00))


@pytest.fixture
def emu():
    e = Emulator.__new__(Emulator)
    e._L, e._h, e.device, e.lib_path, e.programs = StubLibrary(), C.c_void_p(0xD0), 0, None, None
    e._ro_key = ('caller', 0)                   # (readout tables "loaded by the caller": run_device loads none)
    yield e
    e._h = None


def one_call(emu):
    assert len(emu._L.calls) == 1
    return emu._L.calls.pop()


def expect(emu, call, name, cfg, ptrs, handle):
    """``call`` = ``name``(ctx, cfg, *ptrs, stream); in ``ptrs`` None stands for a struct's address"""
    got_name, args, structs = call
    assert got_name == name
    assert len(args) == len(ptrs) + 3 and args[0] is emu._h and args[-1] == handle
    if cfg is not None:
        assert args[1] == C.addressof(cfg)
    for i, p in enumerate(ptrs):
        if p is None:
            assert i + 2 in structs and isinstance(args[i + 2], int) and args[i + 2], i
        else:
            assert args[i + 2] == p, i
    return structs


def pair_fields(pt, meas_cap, n_drv, n_lo):
    want = dict(n_pairs=pt.n_pairs, n_lanes=pt.n_lanes, event_cap=pt.event_cap, meas_cap=meas_cap, n_samples_drv=n_drv,
                n_samples_lo=n_lo)
    want.update({f: pt.cols[f].ctypes.data for f in DemodPairTable.FIELDS})
    return want


def line_fields(ft):
    return dict(n_lines=ft.n_lines, line_first=ft.line_first.ctypes.data, member=ft.member.ctypes.data)


@pytest.mark.parametrize('stream,handle', STREAMS)
def test_demodulate_calls(emu, stream, handle):
    c = case()
    out = run_outputs()
    iq_d, iq_l, acc, res = z((3, 12)), z((3, 4)), z((4, 3, 2)), z((3, 2))
    got = emu.demodulate(c.cfg, None, iq_d, None, iq_l, out, acc, res, stream, pairs=c.pt)
    assert got[0] is acc and got[1] is res
    ptrs = [None, out['summary'].data_ptr(), out['events'].data_ptr(), iq_d.data_ptr(), iq_l.data_ptr(),
            acc.data_ptr(), res.data_ptr()]
    st = expect(emu, one_call(emu), 'dpemu_demod_iq', c.cfg, ptrs, handle)
    assert st[2] == pair_fields(c.pt, 4, 12, 4)
    # one plan that holds both channels of (shot 5, core 1) and (shot 5, core 2)
    plan = ChannelPlan.__new__(ChannelPlan)
    drv, lo = c.cfg.ro_drv_elem, c.cfg.meas_elem
    plan.channels = [(5, 1, drv), (5, 1, lo), (5, 2, drv), (5, 2, lo)]
    plan.desc = np.array([(0, drv, 16, 1, 0, 0, 0, 0), (0, lo, 4, 1, 0, 0, 0, 0), (2, drv, 16, 1, 0, 0, 0, 0),
                          (2, lo, 4, 1, 0, 0, 0, 0)], np.uint32)
    plan.n_lanes, plan.event_cap = 3, 16
    iq, acc, res = z((4, 8)), z((4, 2, 2)), z((2, 2))
    got = emu.demodulate_plan(c.cfg, plan, iq, out, acc, res, stream)
    assert got[0] is acc and got[1] is res
    ptrs = [None, out['summary'].data_ptr(), out['events'].data_ptr(), iq.data_ptr(), iq.data_ptr(), acc.data_ptr(),
            res.data_ptr()]
    st = expect(emu, one_call(emu), 'dpemu_demod_iq', c.cfg, ptrs, handle)[2]
    assert [st[f] for f in ('n_pairs', 'n_lanes', 'event_cap', 'meas_cap', 'n_samples_drv', 'n_samples_lo')] == \
        [2, 3, 16, 4, 8, 8]


@pytest.mark.parametrize('stream,handle', STREAMS)
def test_feedline_calls(emu, stream, handle):
    c = case()
    out = run_outputs()
    s_ptr, e_ptr = out['summary'].data_ptr(), out['events'].data_ptr()
    iq_d, iq_l, adc, acc, res, states = z((3, 8)), z((3, 4)), z((2, 4)), z((4, 3, 2)), z((3, 2)), z((3,))
    tab = ResonatorTable.from_coefficients(c.pt, np.zeros((3, 2, 4), np.int64), 7)
    for resonators in (None, tab):
        for st_t in (None, states):
            assert emu.feedline_adc(c.cfg, c.ft, iq_d, out, 4, adc, stream, resonators, st_t) is adc
            name = 'dpemu_feedline_adc' + ('' if resonators is None else '_res') + ('' if st_t is None else '_st')
            ptrs = [None, None] + ([] if resonators is None else [None])
            ptrs += [s_ptr, e_ptr, iq_d.data_ptr(), adc.data_ptr()]
            ptrs += [] if st_t is None else [states.data_ptr()]
            st = expect(emu, one_call(emu), name, c.cfg, ptrs, handle)
            assert st[2] == pair_fields(c.pt, 4, 8, 4) and st[3] == line_fields(c.ft)
            if resonators is not None:
                assert st[4] == dict(coef=tab.coef.ctypes.data, adc_sigma=7)
    got = emu.demodulate_feedline(c.cfg, c.ft, iq_l, out, adc=adc, acc=acc, result=res, stream=stream)
    assert got[0] is acc and got[1] is res
    ptrs = [None, None, s_ptr, e_ptr, adc.data_ptr(), iq_l.data_ptr(), acc.data_ptr(), res.data_ptr()]
    st = expect(emu, one_call(emu), 'dpemu_demod_feedline', c.cfg, ptrs, handle)
    assert st[2] == pair_fields(c.pt, 4, 0, 4) and st[3] == line_fields(c.ft)
    with pytest.raises(DpemuError) as e:
        emu.demodulate_feedline(c.cfg, c.ft, iq_l, out, adc=adc, acc=acc, result=res, states=states)
    assert str(e.value) == 'resonators and states shape the adc trace this call makes: pass iq_drv, not adc'
    with pytest.raises(DpemuError) as e:
        emu.demodulate_feedline(c.cfg, c.ft, iq_l, out, acc=acc, result=res)
    assert str(e.value) == 'demodulate_feedline needs the adc tensor or iq_drv to make it from'
    with pytest.raises(DpemuError) as e:
        emu.feedline_adc(c.cfg, c.ft, iq_d, out, 4, adc, stream, ResonatorTable.from_coefficients(
            hb.case('edge_short_drive').pt, np.zeros((3, 2, 4), np.int64)))
    assert str(e.value) == 'the resonator table is of another pair table than the feedlines'
    assert not emu._L.calls
    # traces
    tr = z((4, 4, 2, 10, 4), I64)
    for st_t in (None, states):
        assert emu.feedline_traces(c.cfg, c.ft, iq_l, out, adc, 10, 3, True, tr, stream, st_t) is tr
        ptrs = [None, None, None, s_ptr, e_ptr, adc.data_ptr(), iq_l.data_ptr(), tr.data_ptr()]
        ptrs += [] if st_t is None else [states.data_ptr()]
        st = expect(emu, one_call(emu), 'dpemu_feedline_traces' + ('' if st_t is None else '_st'), c.cfg, ptrs, handle)
        assert st[2] == pair_fields(c.pt, 4, 0, 4) and st[3] == line_fields(c.ft)
        assert st[4] == dict(n_bins=10, bin_clocks=3, by_slot=1)
    tr7 = z((1, 4, 2, 7, 4), I64)
    emu.feedline_traces(c.cfg, c.ft, iq_l, out, adc, 7, traces=tr7, stream=stream)
    assert one_call(emu)[2][4] == dict(n_bins=7, bin_clocks=1, by_slot=0)
    with pytest.raises(DpemuError) as e:
        emu.feedline_traces(c.cfg, c.ft, iq_l, out, adc, 10, 3, True, tr, stream, z((4,)))
    assert str(e.value) == 'states must be an int32 tensor [3]' and not emu._L.calls


@pytest.mark.parametrize('stream,handle', STREAMS)
def test_iq_stats_calls(emu, stream, handle):
    c = case()
    acc, summ, res, stats = z((4, 12, 2)), z((12, 8)), z((12, 2)), z((1, 4, 2, 16), I64)
    bits, states = z((12,)), z((12,))
    cols = dict(n_cols=12, meas_cap=4, by_slot=0, count_stride=8, core=None, shot=None, shot_begin=40, axis=None,
                thr=None)
    for counts, off in ((summ, 20), (res, 0)):
        for st_t in (None, states):
            got = emu.iq_stats(c.cfg, acc, counts, 12, 40, stats=stats, bits=bits, stream=stream, states=st_t)
            assert got[0] is stats and got[1] is bits
            ptrs = [None, acc.data_ptr(), counts.data_ptr() + off, stats.data_ptr(), bits.data_ptr()]
            ptrs += [] if st_t is None else [states.data_ptr()]
            st = expect(emu, one_call(emu), 'dpemu_iq_stats' + ('' if st_t is None else '_st'), c.cfg, ptrs, handle)
            assert st[2] == dict(cols, count_stride=int(counts.shape[1]))
    # no bits; by_slot; per-core axis and thr
    stats4 = z((4, 4, 2, 16), I64)
    got = emu.iq_stats(c.cfg, acc, summ, by_slot=True, axis=[1, 2, 3, 4], thr=[-1, 0, 1, 2], stats=stats4,
                       stream=stream)
    assert got[0] is stats4 and got[1] is None
    name, args, st = one_call(emu)
    assert name == 'dpemu_iq_stats'
    assert args[3:] == [acc.data_ptr(), summ.data_ptr() + 20, stats4.data_ptr(), None, handle]
    assert st[2]['axis'] and st[2]['thr'] and dict(st[2], axis=None, thr=None) == dict(cols, by_slot=1, shot_begin=0)
    with pytest.raises(DpemuError) as e:
        emu.iq_stats(c.cfg, acc, summ, axis=[1, 2, 3], stats=stats, stream=stream)
    assert str(e.value) == 'axis must hold cores_per_shot = 4 uint32 values'
    with pytest.raises(DpemuError) as e:
        emu.iq_stats(c.cfg, acc, summ, thr=[0, 0, 0, 2 ** 31], stats=stats, stream=stream)
    assert str(e.value) == 'thr must hold cores_per_shot = 4 int32 values'
    # the pairs of a table: demodulate's acc / result
    acc3, res3, bits3 = z((4, 3, 2)), z((3, 2)), z((3,))
    got = emu.iq_stats(c.cfg, acc3, res3, pairs=c.pt, stats=stats, bits=bits3, stream=stream)
    assert got[0] is stats and got[1] is bits3
    ptrs = [None, acc3.data_ptr(), res3.data_ptr(), stats.data_ptr(), bits3.data_ptr()]
    st = expect(emu, one_call(emu), 'dpemu_iq_stats', c.cfg, ptrs, handle)
    assert st[2] == dict(cols, n_cols=3, count_stride=2, shot_begin=0, core=c.pt.cols['core'].ctypes.data,
                         shot=c.pt.cols['shot'].ctypes.data)
    # no columns: null pointers
    empty = torch.zeros((4, 0, 2), dtype=I32), torch.zeros((0, 8), dtype=I32)
    for st_t in (None, torch.zeros(0, dtype=I32)):
        emu.iq_stats(c.cfg, *empty, stats=stats, bits=z((5,)), stream=stream, states=st_t)
        name, args, _ = one_call(emu)
        assert name == 'dpemu_iq_stats' + ('' if st_t is None else '_st')
        assert args[3:] == [None, None, stats.data_ptr(), None] + ([] if st_t is None else [None]) + [handle]


@pytest.mark.parametrize('stream,handle', STREAMS)
def test_simulate_gates_calls(emu, stream, handle):
    c = case()
    out = run_outputs(12)
    gs, pops, res, states = gates(), z((2, 3, 4), I64), z((2, 3, 4)), z((12,))
    qs = dict(n_regs=2, n_gates=0, drv_elem=0, detune=None, n_lanes=12, event_cap=16, shot_begin=9, n_shots=3)
    ptrs = [None, out['summary'].data_ptr(), out['events'].data_ptr(), pops.data_ptr(), res.data_ptr()]
    got = emu.simulate_gates(c.cfg, gs, out, 3, 9, pops, res, stream)
    assert len(got) == 2 and got[0] is pops and got[1] is res
    st = expect(emu, one_call(emu), 'dpemu_qsim', c.cfg, ptrs, handle)[2]
    assert {k: st[k] for k in qs} == qs and st['reg_core'] and st['gates']
    got = emu.simulate_gates(c.cfg, gs, out, 3, 9, pops, res, stream, measure=True, states=states)
    assert len(got) == 3 and got[0] is pops and got[1] is res and got[2] is states
    st = expect(emu, one_call(emu), 'dpemu_qsim_meas', c.cfg, ptrs + [states.data_ptr()], handle)[2]
    assert {k: st[k] for k in qs} == qs
    for kw, message in ((dict(states=states), 'states is the output of measure=True'),
                        (dict(measure=True, states=z((11,))), 'states must be an int32 tensor [12]')):
        with pytest.raises(DpemuError) as e:
            emu.simulate_gates(c.cfg, gs, out, 3, 9, pops, res, stream, **kw)
        assert str(e.value) == message and not emu._L.calls


@pytest.mark.parametrize('stream,handle', STREAMS)
def test_run_device_call(emu, stream, handle):
    c = case()
    cfg = with_cfg(c.cfg, n_groups=2)
    out = dict(run_outputs(12), meas=z((4, 12, 2)), hist=z((2, 16), I64), hist_next=z((2, 16), I64), acc=z((4, 12, 2)))
    assert emu.run_device(cfg, 3, 21, out, stream) is None
    name, args, st = one_call(emu)
    assert name == 'dpemu_run' and len(args) == 6 and args[0] is emu._h
    assert args[1] == C.addressof(cfg) and args[2:4] == [21, 3] and args[5] == handle
    assert st[4] == {k: (out[k].data_ptr() if k in out else None) for k in _abi.OUTPUT_NAMES}
    for bad, message in ((dict(out, wave=z((1,))), "unknown outputs ['wave']"),
                         (dict(out, meas=z((4, 12, 1))), 'meas: 48 elements, the run writes 96 ((4, 12, 2))'),
                         (dict(out, hist=z((2, 16))), 'hist: dtype torch.int32 (want torch.int64)')):
        with pytest.raises(DpemuError) as e:
            emu.run_device(cfg, 3, 21, bad, stream)
        assert str(e.value) == message and not emu._L.calls


def dds_plan():
    plan = ChannelPlan.__new__(ChannelPlan)
    plan.desc = np.array([(0, 0, 16, 1, 0, 5, 0, 16), (2, 1, 4, 4, 0, 5, 0, 16)], np.uint32)
    plan.env, plan.freq = np.zeros(5, np.uint32), np.zeros(16, np.uint32)
    plan.n_lanes, plan.event_cap = 3, 16
    plan._cols = {f: np.ascontiguousarray(plan.desc[:, i]) for i, f in enumerate(DESC_FIELDS)}
    plan._dev = (z((5,)), z((16,)))             # the tables "already uploaded"
    return plan


@pytest.mark.parametrize('stream,handle', STREAMS)
def test_synthesize_call(emu, stream, handle):
    plan, out, iq = dds_plan(), run_outputs(), z((2, 64))
    assert emu.synthesize(plan, out, 64, iq, stream) is iq
    ptrs = [out['summary'].data_ptr(), out['events'].data_ptr(), plan._dev[0].data_ptr(), plan._dev[1].data_ptr(),
            iq.data_ptr()]
    name, args, st = one_call(emu)
    assert name == 'dpemu_dds' and args[0] is emu._h and args[2:] == ptrs + [handle] and st[1] == dict(
        {f: plan._cols[f].ctypes.data for f in DESC_FIELDS}, n_channels=2, n_lanes=3, n_samples=64, event_cap=16)
    for k in ('summary', 'events'):
        with pytest.raises(DpemuError) as e:
            emu.synthesize(plan, without(out, k), 64, iq, stream)
        assert str(e.value) == 'synthesize needs the run\'s {} output'.format(k)
    for bad in (dict(outputs=run_outputs(4)), dict(outputs=dict(out, events=z((8, 3, 4)))), dict(iq=z((2, 60))),
                dict(iq=z((3, 64))), dict(iq=z((2, 64), torch.int16)),
                dict(outputs=dict(out, summary=z((8, 3)).t())),
                dict(outputs=dict(out, events=torch.zeros((16, 3, 4), dtype=I32)))):
        with pytest.raises(DpemuError):
            emu.synthesize(**dict(dict(plan=plan, outputs=out, n_samples=64, iq=iq, stream=stream), **bad))
    assert not emu._L.calls


# ---- what this module's introduction added (not in the code the tests above were first run against) -------------
def test_synthesize_refuses_what_the_later_stages_refuse(emu):
    """synthesize's tensors go through check_tensor: dtype width, device index, contiguity and device of iq"""
    plan, out, iq = dds_plan(), run_outputs(), z((2, 64))
    for bad, message in (
            (dict(outputs=dict(out, summary=z((3, 8), torch.int16))), 'summary: dtype torch.int16 (want torch.int32)'),
            (dict(outputs=dict(out, events=z((16, 3, 4), torch.float32))),
             'events: dtype torch.float32 (want torch.int32)'),
            (dict(outputs=dict(out, events=z((16, 3, 4), index=1))),
             'events: tensor on cuda:1 but the emulator runs on cuda:0'),
            (dict(outputs=run_outputs(4)), 'summary: 32 elements, the run writes 24 ((3, 8))'),
            (dict(iq=z((2, 64), index=1)), 'iq: tensor on cuda:1 but the emulator runs on cuda:0'),
            (dict(iq=torch.zeros((2, 64), dtype=I32)), 'iq: tensor on cpu but the emulator runs on cuda:0'),
            (dict(iq=z((64, 2)).t()), 'iq: tensor must be contiguous'),
            (dict(iq=z((2, 64), I64)), 'iq: dtype torch.int64 (want torch.int32)'),
            (dict(iq=z((2, 60))), 'iq: 120 elements, the run writes 128 ((2, 64))')):
        with pytest.raises(DpemuError) as e:
            emu.synthesize(**dict(dict(plan=plan, outputs=out, n_samples=64, iq=iq), **bad))
        assert str(e.value) == message and not emu._L.calls


def test_tensor_or_new():
    from distributed_processor_amd import stage_tensors as stg
    c = case()
    cpu = torch.device('cpu')
    specs = {}
    for s in (stg.run_input_specs(3, 16), stg.dds_specs(dds_plan(), 64), stg.demod_specs(c.cfg, 3),
              stg.adc_specs(c.ft, 4), stg.trace_specs(c.cfg, 10, True), stg.iq_stats_specs(c.cfg, 4, 12, False),
              stg.qsim_specs(2, 3), stg.states_specs(12)):
        specs.update({'{} of {}'.format(k, '/'.join(s)): v for k, v in s.items()})
    assert specs['traces of traces'][0] == (4, 4, 2, 10, 4) and specs['stats of stats/bits'][0] == (1, 4, 2, 16)
    assert len(specs) == 12
    for name, (shape, dtype) in specs.items():
        new = stg.tensor_or_new(name, None, (shape, dtype), cpu)
        assert isinstance(new, torch.Tensor) and tuple(new.shape) == tuple(shape) and new.dtype == dtype
        assert new.device == cpu and new.is_contiguous()
        assert stg.tensor_or_new(name, None, (shape, dtype), cpu, alloc=False) is None
        given = z(shape, dtype)
        assert stg.tensor_or_new(name, given, (shape, dtype), 0) is given
        assert stg.tensor_or_new(name, given, (shape, dtype), 0, alloc=False) is given
        with pytest.raises(DpemuError):
            stg.tensor_or_new(name, z(tuple(shape) + (2,), dtype), (shape, dtype), 0)
    # the check functions return a caller's tensors as they are and leave None alone unless told to allocate
    out = run_outputs()
    acc, res = z((4, 3, 2)), z((3, 2))
    got = stg.check_demod_tensors(c.pt, c.cfg, z((3, 4)), z((3, 4)), out, acc, res, 0)
    assert got[0] is acc and got[1] is res
    assert stg.check_demod_tensors(c.pt, c.cfg, z((3, 4)), z((3, 4)), out, None, res, 0) == (None, res)
    assert stg.check_feedline_tensors(c.ft, c.cfg, out, 0, iq_drv=z((3, 4)), n_samples_lo=4) == (None, None, None)
    got = stg.check_iq_stats_tensors(c.cfg, z((4, 8, 2)), z((8, 2)), None, None, False, None, None, 0)
    assert got == (8, None, None)
    assert stg.check_qsim_tensors(c.cfg, gates(), run_outputs(12), 3, 0) == (None, None)


def header_prototypes():
    """{entry point: its parameter list} of include/dpemu.h, comments removed"""
    with open(os.path.join(REPO, 'include', 'dpemu.h')) as f:
        txt = re.sub(r'/\*.*?\*/', '', f.read(), flags=re.S)
    protos = dict(re.findall(r'\b(dpemu_[a-z_0-9]+)\s*\(([^()]*)\)\s*;', txt))
    return {n: [] if a.strip() == 'void' else [p.strip() for p in a.split(',')] for n, a in protos.items()}


def test_signature_table_matches_header():
    protos = header_prototypes()
    assert set(protos) == set(_native.SIGNATURES) == set(_native.EXPORTS)
    for name, (argtypes, restype) in _native.SIGNATURES.items():
        assert len(argtypes) == len(protos[name]), name
        for tp, param in zip(argtypes, protos[name]):
            assert (tp is C.c_void_p or tp._type_ is C.c_void_p) == ('*' in param), (name, param)
        assert restype in (C.c_int, C.c_char_p)
    st = sorted(n for n in protos if n.endswith('_st'))
    assert st == sorted(b + '_st' for b in _native.ST_BASES) and len(st) == 4
    for b in _native.ST_BASES:
        base, var = _native.SIGNATURES[b], _native.SIGNATURES[b + '_st']
        assert len(var[0]) == len(base[0]) + 1 and var[1] is base[1]
        assert [p.split()[-1] for p in protos[b + '_st']] == \
            [p.split()[-1] for p in protos[b][:-1]] + ['*states', '*stream']
