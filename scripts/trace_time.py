"""Kernel time of the averaged-trace stage by the library's
own event pairs (dpemu_set_kernel_timing / dpemu_kernel_times):
scripts/feedline_time.py's inputs -- config 3's readout channels, one readout
per lane (a 1000-clock window, rdrv 16 and rdlo 4 samples per clock), --shots
x --cores pairs with the --cores pairs of every shot on one feedline -- with
n_bins = the window's clocks at bin_clocks 1.  feedline_trace_kernel and
feedline_demod_kernel are launched in turn on the same inputs in one process
(--launches rounds after --warmup), and a torch.clone of as many bytes as the
cost model counts is timed by device events beside them (a clone reads and
writes its bytes: it moves twice what the model counts).  Prints one JSON
line; --out appends it to a file.

Cost model (bytes the algorithm must move): the
demodulator's -- per readout and window clock spc_lo * 4 B of the LO row and
spc_lo * 4 B of the ADC row.  The table (S C 2 n_bins 32 B) and the atomics
that fill it are not counted."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_processor_amd import _abi, workloads                            # noqa: E402
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable, FeedlineTable          # noqa: E402
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs   # noqa: E402
from scripts.demod_iq_time import one_readout                                   # noqa: E402
from scripts.feedline_time import HBM_PEAK, clone_ms, spread                     # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shots', type=int, default=1024)
    ap.add_argument('--cores', type=int, default=8)
    ap.add_argument('--by-slot', action='store_true')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--lib', default=None, help="another build of libdpemu.so (A/B runs)")
    a = ap.parse_args()
    import torch
    ps = ProgramSet(one_readout(a.cores))
    cfg = _abi.make_config(a.cores, n_groups=ps.n_groups, max_cycles=50000, event_cap=8, meas_cap=1,
                           meas_latency=workloads.CONFIG3_DEMOD_LATENCY, lane_order=_abi.LANES_SHOT_MAJOR,
                           demod=workloads.config3_demod(ps))
    n_clks = 10 + workloads.RDLO_DELAY + workloads.READ_CLKS + 2
    who = [(s, c) for s in range(a.shots) for c in range(a.cores)]
    params = {e: (d['samples_per_clk'], d['interp_ratio']) for e, d in enumerate(workloads.ELEMS)}
    spc_d, spc_l = params[workloads.RDRV][0], params[workloads.RDLO][0]
    n_bins = workloads.READ_CLKS
    with Emulator(0, lib_path=a.lib) as emu:
        emu.load(ps)
        out = alloc_device_outputs(cfg, a.shots, want=('summary', 'events'))
        emu.run_device(cfg, a.shots, 0, out)
        drv = ChannelPlan(ps, cfg, 0, a.shots, [(s, c, workloads.RDRV) for s, c in who], params)
        lo = ChannelPlan(ps, cfg, 0, a.shots, [(s, c, workloads.RDLO) for s, c in who], params)
        iq_d = emu.synthesize(drv, out, n_clks * spc_d)
        iq_l = emu.synthesize(lo, out, n_clks * spc_l)
        pt = DemodPairTable(cfg, drv, lo)
        ft = FeedlineTable(pt)
        assert ft.n_lines == a.shots and all(len(ln) == a.cores for ln in ft.lines)
        dev = iq_d.device
        adc = emu.feedline_adc(cfg, ft, iq_d, out, n_clks * spc_l)
        acc = torch.empty((cfg.meas_cap, pt.n_pairs, 2), dtype=torch.int32, device=dev)
        res = torch.empty((pt.n_pairs, 2), dtype=torch.int32, device=dev)
        S = cfg.meas_cap if a.by_slot else 1
        traces = torch.empty((S, a.cores, 2, n_bins, _abi.TRACE_WORDS), dtype=torch.int64, device=dev)

        def one_round():
            emu.feedline_traces(cfg, ft, iq_l, out, adc, n_bins, by_slot=a.by_slot, traces=traces)
            emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc, acc=acc, result=res)
        for _ in range(a.warmup):
            one_round()
        torch.cuda.synchronize()
        emu.kernel_timing(True)
        for _ in range(a.launches):
            one_round()
        ms = emu.kernel_times()
        emu.kernel_timing(False)
        assert len(ms) == 2 * a.launches and (res[:, 0] == 1).all().item()
        t = traces.cpu().numpy()
        # every pair has one readout whose window (clipped by the rows' end) fills its bins with spc_l samples each
        n_samples = int(t[..., 1].sum())
        assert int(t[..., 0].sum()) * spc_l == n_samples and pt.n_pairs * (n_bins - 8) * spc_l <= n_samples
        nb = n_samples * 2 * 4                      # the samples summed, one 4-B word of each row
        c = spread(clone_ms(torch, nb, a.warmup, a.launches))
        rec = {'shots': a.shots, 'members_per_line': a.cores, 'lines': ft.n_lines, 'readouts': pt.n_pairs,
               'window_clks': n_samples / (spc_l * pt.n_pairs), 'n_bins': n_bins, 'bin_clocks': 1,
               'by_slot': bool(a.by_slot), 'spc': [spc_d, spc_l], 'launches': a.launches, 'lib': a.lib,
               'model_bytes': nb, 'clone_ms_median': c['ms_median'],
               'clone_ms_min': c['ms_min'], 'clone_ms_max': c['ms_max']}
        for name, tm in (('feedline_trace_kernel', ms[0::2]), ('feedline_demod_kernel', ms[1::2])):
            r = spread(tm)
            r.update(model_bytes_per_s=nb / (r['ms_median'] * 1e-3),
                     fraction_of_8TBps=nb / (r['ms_median'] * 1e-3) / HBM_PEAK,
                     ratio_to_clone=r['ms_median'] / c['ms_median'])
            rec[name] = r
        rec['trace_to_demod_ratio'] = rec['feedline_trace_kernel']['ms_median'] / rec['feedline_demod_kernel']['ms_median']
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
