"""Kernel time of demod_iq_kernel by the library's own event
pairs (dpemu_set_kernel_timing / dpemu_kernel_times): config 3's readout
channels, one readout per lane (rdrv at 10, rdlo 300 clocks later, a
1000-clock window, rdrv 16 and rdlo 4 samples per clock), --shots x --cores
pairs.  Prints one JSON line: the median of --launches launches after
--warmup, the algorithmic bytes (per readout the LO window, 4 B per sample,
plus every 64-B line of the drive window) and their rate against 8 TB/s."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_processor_amd import _abi, isa, workloads                      # noqa: E402
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable           # noqa: E402
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs   # noqa: E402

HBM_PEAK = 8e12


def one_readout(n_cores):
    prog = {}
    for c in range(n_cores):
        b = workloads.CoreBuilder()
        b.emit(isa.pulse_reset())
        workloads.readout(b, workloads.qubit_params(c), 10)
        b.emit(isa.done_cmd())
        prog[str(c)] = b.assembled()
    return prog


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shots', type=int, default=1024)
    ap.add_argument('--cores', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--lib', default=None, help='another build of libdpemu.so (A/B)')
    a = ap.parse_args()
    import torch
    ps = ProgramSet(one_readout(a.cores))
    cfg = _abi.make_config(a.cores, n_groups=ps.n_groups, max_cycles=50000, event_cap=8, meas_cap=1,
                           meas_latency=workloads.CONFIG3_DEMOD_LATENCY, lane_order=_abi.LANES_SHOT_MAJOR,
                           demod=workloads.config3_demod(ps))
    n_clks = 10 + workloads.RDLO_DELAY + workloads.READ_CLKS + 2
    who = [(s, c) for s in range(a.shots) for c in range(a.cores)]
    params = {e: (d['samples_per_clk'], d['interp_ratio']) for e, d in enumerate(workloads.ELEMS)}
    with Emulator(0, lib_path=a.lib) as emu:
        emu.load(ps)
        out = alloc_device_outputs(cfg, a.shots, want=('summary', 'events'))
        emu.run_device(cfg, a.shots, 0, out)
        drv = ChannelPlan(ps, cfg, 0, a.shots, [(s, c, workloads.RDRV) for s, c in who], params)
        lo = ChannelPlan(ps, cfg, 0, a.shots, [(s, c, workloads.RDLO) for s, c in who], params)
        iq_d = emu.synthesize(drv, out, n_clks * params[workloads.RDRV][0])
        iq_l = emu.synthesize(lo, out, n_clks * params[workloads.RDLO][0])
        pt = DemodPairTable(cfg, drv, lo)
        acc = torch.empty((cfg.meas_cap, pt.n_pairs, 2), dtype=torch.int32, device=iq_d.device)
        res = torch.empty((pt.n_pairs, 2), dtype=torch.int32, device=iq_d.device)
        for _ in range(a.warmup):
            emu.demodulate(cfg, drv, iq_d, lo, iq_l, out, acc, res, pairs=pt)
        torch.cuda.synchronize()
        emu.kernel_timing(True)
        for _ in range(a.launches):
            emu.demodulate(cfg, drv, iq_d, lo, iq_l, out, acc, res, pairs=pt)
        ms = emu.kernel_times()
        emu.kernel_timing(False)
        counts = res[:, 0].cpu().numpy()
    assert len(ms) == a.launches and (counts == 1).all()
    spc_d, spc_l = params[workloads.RDRV][0], params[workloads.RDLO][0]
    per_read = workloads.READ_CLKS * (spc_l * 4 + max(64, spc_d * 4))     # LO window + drive-window lines
    total = per_read * pt.n_pairs
    med = float(np.median(ms))
    print(json.dumps({'lib': a.lib, 'kernel': 'demod_iq_kernel', 'pairs': pt.n_pairs, 'window_clks': workloads.READ_CLKS,
                      'launches': a.launches, 'ms_median': med, 'ms_min': float(min(ms)), 'ms_max': float(max(ms)),
                      'bytes_per_readout': per_read, 'bytes': total, 'bytes_per_s': total / (med * 1e-3),
                      'fraction_of_8TBps': total / (med * 1e-3) / HBM_PEAK}))


if __name__ == '__main__':
    main()
