"""Kernel time of the resonator stage by the library's own
event pairs (dpemu_set_kernel_timing / dpemu_kernel_times): scripts/feedline_time.py's
inputs -- config 3's readout channels, one readout per lane, a 1312-clock
trace at 16 drive and 4 LO samples per clock, --shots x --cores pairs with the
--cores pairs of every shot on one feedline.  feedline_res_kernel (a
resonator of linewidth --kappa per member, converter noise on) and
feedline_adc_kernel are launched in turn on the same inputs in one process
(--launches rounds after --warmup).  Prints one JSON line; --out appends it to
a file.

Cost model:
  per member and LO sample   the drive bytes fetched -- at 16:4 the gather takes
                             one 4-B word in four, but each 64-B segment it
                             touches is fetched whole: spc_drv / spc_lo * 4 B --
                             and eight 64-bit multiply-adds (v_mad_i64_i32)
  per line and LO sample     one Philox4x32-10 draw and 4 B of the ADC row written"""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_processor_amd import _abi, workloads                            # noqa: E402
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable, FeedlineTable, ResonatorTable   # noqa: E402
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs   # noqa: E402
from scripts.demod_iq_time import one_readout                                   # noqa: E402
from scripts.feedline_time import spread                                        # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shots', type=int, default=1024)
    ap.add_argument('--cores', type=int, default=8)
    ap.add_argument('--kappa', type=float, default=0.005, help='full linewidth, turns per clock')
    ap.add_argument('--adc-sigma', type=float, default=0.01)
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
        pt = DemodPairTable(cfg, drv, lo)
        ft = FeedlineTable(pt)
        assert ft.n_lines == a.shots and all(len(ln) == a.cores for ln in ft.lines)
        rng = np.random.RandomState(1)
        f_res = rng.randint(0, 2 ** 32, size=(pt.n_pairs, 1), dtype=np.int64) + np.array([0, int(a.kappa * 2 ** 32)])
        tab = ResonatorTable(pt, f_res % 2 ** 32, a.kappa * 2 ** 32, adc_sigma=a.adc_sigma)
        n_lo = n_clks * spc_l
        adc = torch.empty((ft.n_lines, n_lo), dtype=torch.int32, device=iq_d.device)
        adc1 = torch.empty_like(adc)

        def one_round():
            emu.feedline_adc(cfg, ft, iq_d, out, n_lo, adc=adc, resonators=tab)
            emu.feedline_adc(cfg, ft, iq_d, out, n_lo, adc=adc1)
        for _ in range(a.warmup):
            one_round()
        torch.cuda.synchronize()
        emu.kernel_timing(True)
        for _ in range(a.launches):
            one_round()
        ms = emu.kernel_times()
        emu.kernel_timing(False)
        assert len(ms) == 2 * a.launches and adc.any().item()
        members = pt.n_pairs
        rec = {'lib': a.lib, 'shots': a.shots, 'members_per_line': a.cores, 'lines': ft.n_lines, 'members': members,
               'trace_clks': n_clks, 'spc': [spc_d, spc_l],
               'kappa': a.kappa, 'adc_sigma_word': tab.adc_sigma, 'launches': a.launches,
               'model': {'drive_bytes_fetched': members * n_lo * (spc_d // spc_l) * 4,
                         'mad_i64': 8 * members * n_lo, 'philox_draws': ft.n_lines * n_lo,
                         'adc_bytes_written': ft.n_lines * n_lo * 4},
               'feedline_res_kernel': spread(ms[0::2]), 'feedline_adc_kernel': spread(ms[1::2])}
        rec['ratio_res_to_adc'] = rec['feedline_res_kernel']['ms_median'] / rec['feedline_adc_kernel']['ms_median']
        rec['mad_i64_per_s'] = rec['model']['mad_i64'] / (rec['feedline_res_kernel']['ms_median'] * 1e-3)
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
