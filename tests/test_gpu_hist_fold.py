"""The histogram reduce folded into straight_kernel (csrc/lane.h
fold_replicas) and the ordering event recorded only when a second stream needs
it (csrc/capi.cpp order_begin), on the GPU against oracle_fast.

Pulse-only programs with a measurement: config 1's (C = 1, one group) and
Ramsey points with C = 2 and C = 4 in 1-3 groups.  The plan folds where a
workgroup's 256 / C shots are at least 4 per bin -- every C = 1 and C = 2
shape here and C = 4 with one group; C = 4 with 2 or 3 groups (32 / 48 bins
on 64 shots) counts straight into the replicas and keeps the reduce launch
(tests/test_hist_fold_plan.py pins which).  Shot counts: one partial
workgroup, the workgroups around a full one at C = 1 (255, 256, 257), and
64 * 256 + 3 -- more workgroups than the 64 replica rows, so rows wrap and
the last workgroup is mostly invalid lanes."""

import functools

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, workloads
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (2, 1), (2, 2), (2, 3), (4, 1), (4, 2), (4, 3)]
SHOTS = (1, 255, 256, 257, 64 * 256 + 3)
KW = dict(max_cycles=10000, event_cap=8, meas_cap=4, seed=0x5EED, p1=0.5)


@functools.lru_cache(maxsize=None)
def programs(C, ng):
    return ProgramSet(workloads.config1_linear()) if C == 1 else ProgramSet(workloads.config2_ramsey(C, ng))


@functools.lru_cache(maxsize=None)
def ref(C, ng, n, shot0=0, want=('hist',)):
    """oracle_fast's outputs of shots [shot0, shot0 + n): computed once per shape, shared, never written"""
    ps = programs(C, ng)
    cfg = _abi.make_config(C, n_groups=ng, **KW)
    r = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, shot0, n, want=want)
    for a in r.values():
        a.setflags(write=False)
    return r


def ref_hist(C, ng, n, shot0=0):
    return ref(C, ng, n, shot0)['hist'].astype(np.int64)


@pytest.mark.parametrize('C,ng', SHAPES)
def test_folded_histogram_matches_oracle(C, ng):
    """every shot count, both lane orders, stored (hist_assign, over stale
    counts) and added (to a pre-filled histogram); hist_next comes back zero"""
    import torch
    ps = programs(C, ng)
    with Emulator(0) as emu:
        emu.load(ps)
        for n in SHOTS:
            want = ref_hist(C, ng, n)
            assert want.sum() == n
            for order in (_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR):
                for assign in (False, True):
                    cfg = _abi.make_config(C, n_groups=ng, lane_order=order, hist_assign=assign, **KW)
                    out = alloc_device_outputs(cfg, n, want=('summary', 'events', 'meas', 'hist', 'hist_next'))
                    pre = torch.arange(1, out['hist'].numel() + 1, dtype=torch.int64, device='cuda') * 1000003
                    out['hist'].copy_(pre.view(out['hist'].shape))
                    out['hist_next'].fill_(0x5A5A5A5A)
                    emu.run_device(cfg, n, 0, out)
                    torch.cuda.synchronize()
                    assert emu.last_kernel().startswith('straight_kernel<')
                    got = out['hist'].cpu().numpy()
                    base = 0 if assign else pre.view(out['hist'].shape).cpu().numpy()
                    np.testing.assert_array_equal(got, want + base, err_msg=str((C, ng, n, order, assign)))
                    assert not out['hist_next'].any(), (C, ng, n, order, assign)


@pytest.mark.parametrize('C,ng', [(1, 1), (2, 3)])
def test_back_to_back_then_direct(C, ng):
    """two folded runs on one context with nothing between them, then a run
    with DPEMU_X_HIST_DIRECT, then a folded one again: all four histograms
    right, so the replicas and the tickets are back at zero after every run"""
    import torch
    n = 64 * 256 + 3
    ps = programs(C, ng)
    cfg = _abi.make_config(C, n_groups=ng, **KW)
    direct = _abi.make_config(C, n_groups=ng, exec_flags=_abi.X_HIST_DIRECT, **KW)
    with Emulator(0) as emu:
        emu.load(ps)
        outs = [alloc_device_outputs(cfg, n, want=('summary', 'hist')) for _ in range(4)]
        emu.run_device(cfg, n, 0, outs[0])
        emu.run_device(cfg, n, n, outs[1])
        emu.run_device(direct, n, 2 * n, outs[2])
        emu.run_device(cfg, n, 3 * n, outs[3])
        torch.cuda.synchronize()
        for k, o in enumerate(outs):
            np.testing.assert_array_equal(o['hist'].cpu().numpy(), ref_hist(C, ng, n, k * n), err_msg=str(k))


def test_folded_outputs_unchanged():
    """the records around the histogram are the oracle's as before (the fold's
    first wave waits for its own stores; the other waves leave early)"""
    import torch
    C, ng, n = 2, 3, 257
    want = ('summary', 'events', 'meas', 'hist')
    r = ref(C, ng, n, 5, want)
    cfg = _abi.make_config(C, n_groups=ng, **KW)
    with Emulator(0) as emu:
        emu.load(programs(C, ng))
        out = alloc_device_outputs(cfg, n, want=want)
        emu.run_device(cfg, n, 5, out)
        torch.cuda.synchronize()
        s = _abi.unpack_summary(r['summary'])
        valid = {'events': np.minimum(s['n_events'], cfg.event_cap), 'meas': np.minimum(s['n_meas'], cfg.meas_cap)}
        for k in want:
            a, b = out[k].cpu().numpy().view(r[k].dtype).reshape(r[k].shape), r[k]
            if k in valid:
                m = np.arange(b.shape[0])[:, None] < valid[k][None, :]
                a, b = a[m], b[m]
            assert np.array_equal(a, b), k


def test_alternating_streams_in_call_order():
    """eight calls of one context alternating between the default stream and a
    created one, each with its own outputs: every histogram and summary equals
    the single-stream result (the replicas, tickets and run constants are the
    context's, so each call must wait for the one before it on the other
    stream -- from the default stream through an event recorded only then)"""
    import torch
    C, ng, n = 2, 3, 64 * 256 + 3
    cfg = _abi.make_config(C, n_groups=ng, **KW)
    side = torch.cuda.Stream()
    with Emulator(0) as emu:
        emu.load(programs(C, ng))
        outs = [alloc_device_outputs(cfg, n, want=('summary', 'hist')) for _ in range(8)]
        for k, o in enumerate(outs):
            emu.run_device(cfg, n, k * n, o, side if k % 2 else None)
        torch.cuda.synchronize()
        single = [alloc_device_outputs(cfg, n, want=('summary', 'hist')) for _ in range(8)]
        for k, o in enumerate(single):
            emu.run_device(cfg, n, k * n, o)
        torch.cuda.synchronize()
        for k, (o, s) in enumerate(zip(outs, single)):
            assert torch.equal(o['hist'], s['hist']) and torch.equal(o['summary'], s['summary']), k
            np.testing.assert_array_equal(o['hist'].cpu().numpy(), ref_hist(C, ng, n, k * n), err_msg=str(k))
