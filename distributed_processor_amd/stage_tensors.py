"""The device tensors of the stages behind Emulator's methods: the C ABI takes
bare pointers, so they are checked here first.  Every stage tensor's shape and
dtype is written once, in a ``*_specs`` function ({name: (shape, torch dtype)},
as emulator.device_output_specs); checks and allocations read it from there.
The ``check_*`` functions hold a stage's argument rules and return its outputs:
a caller's tensor checked, None left as it is or, with ``alloc`` (Emulator's
methods), replaced by a new tensor on the emulator's device."""

import math

import numpy as np

from . import _abi
from ._native import DpemuError


def check_tensor(name, t, spec, device):
    """a caller tensor must match what the kernel writes: size, dtype,
    contiguity and device (the C ABI has no size arguments)"""
    import torch
    shape, dtype = spec
    if not isinstance(t, torch.Tensor):
        raise DpemuError('{}: expected a torch tensor'.format(name))
    if name in ('hist', 'hist_next') and len(shape) == 2 and shape[1] > 4096:
        raise DpemuError('{} needs cores_per_shot <= 12'.format(name))
    # (cheap attribute calls only: this runs for every output of every launch,
    # and a bench step of config 1 is 27 us of GPU time)
    if not t.is_cuda or t.get_device() != device:
        raise DpemuError('{}: tensor on {} but the emulator runs on cuda:{}'.format(name, t.device, device))
    if t.element_size() != dtype.itemsize or t.is_floating_point():
        raise DpemuError('{}: dtype {} (want {})'.format(name, t.dtype, dtype))
    if not t.is_contiguous():
        raise DpemuError('{}: tensor must be contiguous'.format(name))
    if t.numel() != math.prod(shape):
        raise DpemuError('{}: {} elements, the run writes {} ({})'.format(name, t.numel(), int(np.prod(shape)),
                                                                        tuple(shape)))


def tensor_or_new(name, t, spec, device, alloc=True):
    """``t`` after check_tensor; for ``t`` None a new, uninitialised tensor of ``spec`` on ``device`` (the
    emulator's device index, or a torch.device), or None when ``alloc`` is false"""
    if t is None:
        import torch
        return torch.empty(spec[0], dtype=spec[1], device=device) if alloc else None
    check_tensor(name, t, spec, device)
    return t


# ---- one spec per stage tensor ----
def run_input_specs(n_lanes, event_cap):
    """the two outputs of a run that every later stage reads (as emulator.device_output_specs has them)"""
    import torch
    return {'summary': ((n_lanes, 8), torch.int32), 'events': ((event_cap, n_lanes, 4), torch.int32)}


def dds_specs(plan, n_samples):
    import torch
    return {'iq': ((plan.n_channels, int(n_samples)), torch.int32)}


def demod_specs(cfg, n_pairs):
    """the outputs of demodulate, demodulate_plan and demodulate_feedline"""
    import torch
    return {'acc': ((cfg.meas_cap, n_pairs, 2), torch.int32), 'result': ((n_pairs, 2), torch.int32)}


def adc_specs(lines, n_samples_lo):
    import torch
    return {'adc': ((lines.n_lines, n_samples_lo), torch.int32)}


def trace_specs(cfg, n_bins, by_slot):
    import torch
    return {'traces': ((cfg.meas_cap if by_slot else 1, cfg.cores_per_shot, 2, n_bins, _abi.TRACE_WORDS), torch.int64)}


def iq_stats_specs(cfg, meas_cap, n_cols, by_slot):
    import torch
    return {'stats': ((meas_cap if by_slot else 1, cfg.cores_per_shot, 2, _abi.IQ_STAT_WORDS), torch.int64),
            'bits': ((n_cols,), torch.int32)}


def qsim_specs(n_regs, n_shots):
    import torch
    return {'pops': ((n_regs, n_shots, 4), torch.int64), 'result': ((n_regs, n_shots, 4), torch.int32)}


def qsim_decay_specs(n_regs, n_shots):     # simulate_gates(decay_counts=): per row {jumps, flips} of the two qubits
    import torch
    return {'counts': ((n_regs, n_shots, 4), torch.int32)}


def states_specs(n):          # simulate_gates(measure=True)'s output, the readout stages' input: a word per lane
    import torch
    return {'states': ((int(n),), torch.int32)}


# ---- the shared checks ----
def need_run_inputs(needs, outputs):
    """``outputs`` holds a run's summary and events; ``needs`` names the caller in the message"""
    for k in ('summary', 'events'):
        if k not in outputs:
            raise DpemuError('{} the run\'s {} output'.format(needs, k))


def check_run_inputs(needs, outputs, n_lanes, event_cap, device):
    """need_run_inputs, and the two are the device tensors of a run of n_lanes lanes"""
    need_run_inputs(needs, outputs)
    for k, spec in run_input_specs(n_lanes, event_cap).items():
        check_tensor(k, outputs[k], spec, device)


def check_iq_buffer(name, t, rows, device):
    """an iq buffer is an int32 device tensor [rows, n_samples > 0], one row per channel of its plan"""
    import torch
    if not isinstance(t, torch.Tensor) or t.dim() != 2 or t.shape[0] != rows or t.shape[1] == 0:
        raise DpemuError('{} must be an int32 tensor [{}, n_samples]'.format(name, rows))
    check_tensor(name, t, (tuple(t.shape), torch.int32), device)


# ---- the stages ----
def _check_readout_tensors(needs, lo_rule, pt, cfg, outputs, device, iq_drv, iq_lo, n_samples_lo=None, lines=None,
                           adc=None, acc=None, result=None, alloc=False):
    """the body of check_demod_tensors and check_feedline_tensors, which word two refusals differently
    (``needs``, ``lo_rule``).  With ``lines`` an iq buffer that is None is not part of the call; without,
    both are.  The ADC stage (no iq_lo) makes adc, a demodulator acc and result.  Returns (adc, acc, result)."""
    import torch
    if not 1 <= cfg.meas_cap <= 32:
        raise DpemuError('{} cfg.meas_cap in [1, 32]'.format(needs))
    need_run_inputs(needs, outputs)
    if iq_drv is not None or lines is None:
        check_iq_buffer('iq_drv', iq_drv, pt.n_rows[0], device)
    if iq_lo is not None or lines is None:
        check_iq_buffer('iq_lo', iq_lo, pt.n_rows[1], device)
        n_samples_lo = iq_lo.shape[1]
        if lines is not None and (lines.line_of < 0).any():
            raise DpemuError('pair {} is in no line'.format(int(np.argmax(lines.line_of < 0))))
    n_samples_lo = int(n_samples_lo)
    if n_samples_lo <= 0 or n_samples_lo % 4:
        raise DpemuError(lo_rule.format(n_samples_lo))
    check_run_inputs(needs, outputs, pt.n_lanes, pt.event_cap, device)
    if lines is not None:
        spec = adc_specs(lines, n_samples_lo)['adc']
        if adc is not None and (not isinstance(adc, torch.Tensor) or tuple(adc.shape) != spec[0]):
            raise DpemuError('adc must be an int32 tensor [{}, {}]'.format(*spec[0]))
        adc = tensor_or_new('adc', adc, spec, device, alloc and iq_lo is None)
    specs = demod_specs(cfg, pt.n_pairs)
    acc = tensor_or_new('acc', acc, specs['acc'], device, alloc and iq_lo is not None)
    result = tensor_or_new('result', result, specs['result'], device, alloc and iq_lo is not None)
    return adc, acc, result


def check_demod_tensors(pt, cfg, iq_drv, iq_lo, outputs, acc, result, device, alloc=False):
    """the tensors of Emulator.demodulate against the pair table ``pt`` (dds.DemodPairTable): the run's summary /
    events, the two iq buffers (one row per channel of their plans, int32, LO rows a nonzero multiple of 4
    samples) and acc [meas_cap, n_pairs, 2] / result [n_pairs, 2].  Returns (acc, result)."""
    return _check_readout_tensors('demodulate needs', 'iq_lo: n_samples {} is not a multiple of 4', pt, cfg, outputs,
                                  device, iq_drv, iq_lo, acc=acc, result=result, alloc=alloc)[1:]


def check_feedline_tensors(lines, cfg, outputs, device, iq_drv=None, iq_lo=None, adc=None, acc=None, result=None,
                           n_samples_lo=None, alloc=False):
    """the tensors of Emulator.feedline_adc (iq_drv, n_samples_lo, adc or None) and
    Emulator.demodulate_feedline (iq_lo, adc, acc / result or None) against the feedline table ``lines``
    (dds.FeedlineTable): the run's summary / events, one iq row per channel of the plan, adc int32
    [n_lines, n_samples_lo] with n_samples_lo a nonzero multiple of 4, and for the demodulator every pair
    in a line.  Returns (adc, acc, result)."""
    return _check_readout_tensors('the feedline stages need', 'n_samples_lo {} is not a nonzero multiple of 4',
                                  lines.pairs, cfg, outputs, device, iq_drv, iq_lo, n_samples_lo, lines, adc, acc,
                                  result, alloc)


def check_trace_tensors(lines, cfg, outputs, device, iq_lo, adc, n_bins, bin_clocks, by_slot, traces=None,
                        alloc=False):
    """the tensors and bins of Emulator.feedline_traces: what
    check_feedline_tensors asks of the demodulator's iq_lo and adc (both
    required here), n_bins in 1..TRACE_BINS_MAX, bin_clocks >= 1 within the
    int64 sums' bound n_pairs meas_cap bin_clocks 16 <= 2^31, and traces int64
    [S, C, 2, n_bins, TRACE_WORDS].  Returns traces."""
    if iq_lo is None or adc is None:
        raise DpemuError('feedline_traces needs the iq_lo and adc tensors')
    check_feedline_tensors(lines, cfg, outputs, device, iq_lo=iq_lo, adc=adc)
    n_bins, bin_clocks = int(n_bins), int(bin_clocks)
    if not 1 <= n_bins <= _abi.TRACE_BINS_MAX:
        raise DpemuError('n_bins {} not in [1, {}]'.format(n_bins, _abi.TRACE_BINS_MAX))
    if not 1 <= bin_clocks < 2 ** 32:
        raise DpemuError('bin_clocks {} must be >= 1'.format(bin_clocks))
    if lines.pairs.n_pairs * cfg.meas_cap * bin_clocks * 16 > 2 ** 31:
        raise DpemuError('n_pairs * meas_cap * bin_clocks * 16 = {} exceeds 2^31'.format(
            lines.pairs.n_pairs * cfg.meas_cap * bin_clocks * 16))
    return tensor_or_new('traces', traces, trace_specs(cfg, n_bins, by_slot)['traces'], device, alloc)


def check_iq_stats_tensors(cfg, acc, counts, n_cols, pairs, by_slot, stats, bits, device, alloc=False):
    """the tensors of Emulator.iq_stats: acc int32 [meas_cap 1..32, n_cols, 2], counts a summary [n_cols, 8]
    or a demodulate result [n_cols, 2], stats int64 [S, C, 2, IQ_STAT_WORDS] and bits int32 [n_cols] (None:
    none, True: a new tensor); n_cols agrees with ``pairs`` or is a whole number of shots.  Returns (n_cols,
    stats, bits)."""
    import torch
    if not isinstance(acc, torch.Tensor) or acc.dim() != 3 or acc.shape[2] != 2 or not 1 <= acc.shape[0] <= 32:
        raise DpemuError('acc must be an int32 tensor [meas_cap in 1..32, n_cols, 2]')
    meas_cap, n = int(acc.shape[0]), int(acc.shape[1])
    if n_cols is not None and int(n_cols) != n:
        raise DpemuError('acc has {} columns, n_cols = {}'.format(n, n_cols))
    if n * meas_cap > 2 ** 31:
        raise DpemuError('n_cols * meas_cap = {} exceeds 2^31'.format(n * meas_cap))
    if not isinstance(counts, torch.Tensor) or counts.dim() != 2 or counts.shape[1] not in (2, 8):
        raise DpemuError('counts must be a run\'s summary [n_cols, 8] or a demodulate result [n_cols, 2]')
    if pairs is not None and pairs.n_pairs != n:
        raise DpemuError('acc has {} columns, the pair table {} pairs'.format(n, pairs.n_pairs))
    if pairs is None and n % cfg.cores_per_shot:
        raise DpemuError('acc has {} columns: not a whole number of {}-core shots'.format(n, cfg.cores_per_shot))
    if n:                                   # (an empty tensor has no storage to check)
        check_tensor('acc', acc, (tuple(acc.shape), torch.int32), device)
        check_tensor('counts', counts, ((n, int(counts.shape[1])), torch.int32), device)
    elif counts.shape[0] != 0:
        raise DpemuError('counts: {} rows for 0 columns'.format(counts.shape[0]))
    specs = iq_stats_specs(cfg, meas_cap, n, by_slot)
    stats = tensor_or_new('stats', stats, specs['stats'], device, alloc)
    if bits is True:
        bits = tensor_or_new('bits', None, specs['bits'], device, alloc)
    elif bits is not None and n:
        check_tensor('bits', bits, specs['bits'], device)
    return n, stats, bits


def check_states_tensor(states, n, device, alloc=False):
    """a ``states`` tensor of the readout stages, of simulate_gates(measure=True) and of
    run_device(states=) / cosimulate: int32 [n] on the emulator's device (n = 0: any empty tensor).
    Returns states."""
    import torch
    spec = states_specs(n)['states']
    if states is None and alloc:
        return tensor_or_new('states', None, spec, device)
    if not isinstance(states, torch.Tensor) or states.dim() != 1 or states.shape[0] != int(n):
        raise DpemuError('states must be an int32 tensor [{}]'.format(int(n)))
    if states.dtype != torch.int32:
        raise DpemuError('states: dtype {} (want torch.int32)'.format(states.dtype))
    if n:
        check_tensor('states', states, spec, device)
    return states


def check_qsim_tensors(cfg, gateset, outputs, n_shots, device, pops=None, result=None, alloc=False):
    """the tensors of Emulator.simulate_gates: the summary / events of a run of
    n_shots shots under cfg (event_cap > 0), at least one register, and pops
    int64 / result int32 [n_regs, n_shots, 4].  Returns (pops, result)."""
    n_shots = int(n_shots)
    if n_shots < 0 or gateset.n_regs * n_shots > 2 ** 31:
        raise DpemuError('n_regs * n_shots = {} * {} must be in [0, 2^31]'.format(gateset.n_regs, n_shots))
    if n_shots:                                 # (an empty tensor has no storage to check)
        check_run_inputs('simulate_gates needs', outputs, n_shots * cfg.cores_per_shot, cfg.event_cap, device)
    specs = qsim_specs(gateset.n_regs, n_shots)
    return tuple(tensor_or_new(k, t, specs[k], device, alloc) if n_shots or t is None else t
                 for k, t in (('pops', pops), ('result', result)))
