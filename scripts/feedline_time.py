"""Kernel times of the multiplexed readout stages by the
library's own event pairs (dpemu_set_kernel_timing / dpemu_kernel_times):
scripts/demod_iq_time.py's inputs -- config 3's readout channels, one readout
per lane (rdrv at 10, rdlo 300 clocks later, a 1000-clock window, rdrv 16 and
rdlo 4 samples per clock), --shots x --cores pairs -- with the --cores pairs
of every shot on one feedline.  feedline_adc_kernel, feedline_demod_kernel and
demod_iq_kernel are launched in turn on the same inputs in one process
(--launches rounds after --warmup), and a torch.clone of as many bytes as each
stage's cost model counts is timed by device events beside them (a clone reads
and writes its bytes: it moves twice what the model counts).  Prints one JSON
line; --out appends it to a file.

Cost model (bytes the algorithm must move):
  ADC stage    per line and clock: every member's drive samples -- at 16:4 the
               gather takes one 4-B word in four, but each 64-B segment it
               touches is fetched whole, so all spc_drv * 4 B per clock -- plus
               the spc_lo * 4 B of the ADC row written
  demodulator  per readout and window clock: spc_lo * 4 B of the LO row and
               spc_lo * 4 B of the ADC row"""

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

HBM_PEAK = 8e12


def clone_ms(torch, n_bytes, warmup, launches):
    src = torch.empty(n_bytes // 4, dtype=torch.int32, device='cuda').zero_()
    ms = []
    for i in range(warmup + launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst = src.clone()
        b.record()
        b.synchronize()
        del dst
        if i >= warmup:
            ms.append(a.elapsed_time(b))
    return ms


def spread(ms):
    return {'ms_median': float(np.median(ms)), 'ms_min': float(min(ms)), 'ms_max': float(max(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shots', type=int, default=1024)
    ap.add_argument('--cores', type=int, default=8)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--lib', default=None, help='another build of libdpemu.so (A/B)')
    ap.add_argument('--out', default=None)
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
        adc = torch.empty((ft.n_lines, n_clks * spc_l), dtype=torch.int32, device=dev)
        acc = torch.empty((cfg.meas_cap, pt.n_pairs, 2), dtype=torch.int32, device=dev)
        res = torch.empty((pt.n_pairs, 2), dtype=torch.int32, device=dev)
        acc1, res1 = torch.empty_like(acc), torch.empty_like(res)

        def one_round():
            emu.feedline_adc(cfg, ft, iq_d, out, n_clks * spc_l, adc=adc)
            emu.demodulate_feedline(cfg, ft, iq_l, out, adc=adc, acc=acc, result=res)
            emu.demodulate(cfg, drv, iq_d, lo, iq_l, out, acc1, res1, pairs=pt)
        for _ in range(a.warmup):
            one_round()
        torch.cuda.synchronize()
        emu.kernel_timing(True)
        for _ in range(a.launches):
            one_round()
        ms = emu.kernel_times()
        emu.kernel_timing(False)
        counts = res[:, 0].cpu().numpy()
        assert len(ms) == 3 * a.launches and (counts == 1).all() and (res1[:, 0] == 1).all().item()
        adc_bytes = ft.n_lines * n_clks * (a.cores * spc_d * 4 + spc_l * 4)
        demod_bytes = pt.n_pairs * workloads.READ_CLKS * 2 * spc_l * 4
        rec = {'lib': a.lib, 'shots': a.shots, 'members_per_line': a.cores, 'lines': ft.n_lines, 'readouts': pt.n_pairs,
               'window_clks': workloads.READ_CLKS, 'trace_clks': n_clks, 'spc': [spc_d, spc_l], 'launches': a.launches}
        for name, t, nb in (('feedline_adc_kernel', ms[0::3], adc_bytes), ('feedline_demod_kernel', ms[1::3], demod_bytes),
                            ('demod_iq_kernel', ms[2::3], None)):
            r = spread(t)
            if nb is not None:
                c = spread(clone_ms(torch, nb, a.warmup, a.launches))
                r.update(model_bytes=nb, model_bytes_per_s=nb / (r['ms_median'] * 1e-3),
                         fraction_of_8TBps=nb / (r['ms_median'] * 1e-3) / HBM_PEAK,
                         clone_ms_median=c['ms_median'], clone_ms_min=c['ms_min'], clone_ms_max=c['ms_max'],
                         ratio_to_clone=r['ms_median'] / c['ms_median'])
            rec[name] = r
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
