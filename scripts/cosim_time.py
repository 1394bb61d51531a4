"""Kernel time of the co-simulation interpreter by the library's
own event pairs (dpemu_set_kernel_timing / dpemu_kernel_times), on config 3's
shard as the benchmark runs it -- --shots shots x 8 cores, shot-major lanes,
event_cap 16 -- in one process:

* dpemu_run (branch_kernel<0xb,c8>, the Philox state draw) on
  workloads.cosim_active_reset's programs, measured TWICE (before and after the
  variant), so the box's own run-to-run spread is known;
* dpemu_run_states (branch_kernel<0x8b,c8>: one loaded word in place of the
  draw) on the same programs, with the converged states buffer;
* the whole converged loop, Emulator.cosimulate from zeros: passes, wall time,
  and the kernel times of its dpemu_run_states and dpemu_qsim_meas launches.

Prints one JSON line; --out appends it to a file."""

import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_processor_amd import _abi, workloads                              # noqa: E402
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs   # noqa: E402
from scripts.feedline_time import spread                                            # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shots', type=int, default=1250000)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--launches', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--lib', default=None, help='another build of libdpemu.so (A/B runs)')
    a = ap.parse_args()
    import torch
    prog, gs = workloads.cosim_active_reset(8, prep=1)
    ps = ProgramSet(prog)
    n = a.shots
    cfg = _abi.make_config(8, n_groups=ps.n_groups, max_cycles=50000, event_cap=16, trace_cap=0, meas_cap=4,
                           meas_latency=workloads.CONFIG3_MEAS_LATENCY, seed=0x5EED, p1=0.5, hist_assign=True,
                           lane_order=_abi.LANES_SHOT_MAJOR)
    with Emulator(0, lib_path=a.lib) as emu:
        emu.load(ps)
        out = alloc_device_outputs(cfg, n, want=('summary', 'events', 'meas', 'hist'))
        # the converged loop, timed as a whole (the first call also warms the kernels up)
        emu.cosimulate(cfg, gs, out, n)
        torch.cuda.synchronize()
        emu.kernel_timing(True)
        t0 = time.perf_counter()
        pops, res, states, passes = emu.cosimulate(cfg, gs, out, n)
        torch.cuda.synchronize()
        wall_ms = (time.perf_counter() - t0) * 1e3
        loop_ms = emu.kernel_times()
        assert len(loop_ms) == 2 * passes and emu.last_kernel() == 'qsim_kernel<meas>'
        st = states.cpu().numpy().view(np.uint32)
        assert not ((st >> 1) & 1).any()                                      # every qubit is reset

        def timed(states_arg):
            for _ in range(a.warmup):
                emu.run_device(cfg, n, 0, out, states=states_arg)
            torch.cuda.synchronize()
            emu.kernel_times()
            for _ in range(a.launches):
                emu.run_device(cfg, n, 0, out, states=states_arg)
            ms = emu.kernel_times()
            assert len(ms) == a.launches
            return spread(ms), emu.last_kernel()
        base1, base_name = timed(None)
        var, var_name = timed(states)
        base2, _ = timed(None)
        emu.kernel_timing(False)
        assert base_name == 'branch_kernel<feat=0xb,c8>' and var_name == 'branch_kernel<feat=0x8b,c8>', (base_name, var_name)
        base_med = 0.5 * (base1['ms_median'] + base2['ms_median'])
        rec = {'shots': n, 'cores': 8, 'lanes': 8 * n, 'launches': a.launches, 'lib': a.lib,
               'run': {'kernel': base_name, 'first': base1, 'second': base2,
                       'spread_ms': abs(base1['ms_median'] - base2['ms_median'])},
               'run_states': dict(var, kernel=var_name), 'states_to_run_ratio': var['ms_median'] / base_med,
               'loop': {'passes': passes, 'wall_ms': wall_ms, 'run_states_ms': loop_ms[0::2], 'qsim_meas_ms': loop_ms[1::2],
                        'kernel_ms_total': float(sum(loop_ms))},
               'first_readout_ones': float((st & 1).mean())}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
