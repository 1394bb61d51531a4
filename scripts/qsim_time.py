"""Kernel time of the qubit-state stage by the library's own
event pairs (dpemu_set_kernel_timing / dpemu_kernel_times): config 4 as the
benchmark runs it -- workloads.config4_rb2q_set, 2 cores, depth 200, --seqs
sequences x --spg shots in one launch -- with dpemu_run and dpemu_qsim (with
--measure: dpemu_qsim_meas, one readout per lane) launched in turn in one
process (--launches rounds after --warmup) on the gate set
workloads.rb2q_gateset(2, --over-rotation, --err, --err).  Prints one JSON
line: qsim_kernel's ms beside the run's kernel ms, gates per second and event
bytes per second; --out appends it to a file.

Cost model: a row reads the 16-byte records of its two lanes
once (event bytes = 16 B x the records below event_cap) and applies n_gates
gates of 13 rounded complex products each; the 32 + 16 B it writes per row
are not counted.

--decay T1,T2 (clocks; implies --measure) times dpemu_qsim_decay's
qsim_kernel<meas,decay> beside qsim_kernel<meas> on the same records in the
same process: every round launches the run, the base kernel and the decaying
one, and the line carries both medians and their ratio ('decay')."""

import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from distributed_processor_amd import _abi, isa, qsim, workloads                  # noqa: E402
from distributed_processor_amd.emulator import Emulator, alloc_device_outputs     # noqa: E402
from scripts.feedline_time import spread                                          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--seqs', type=int, default=10000)
    ap.add_argument('--spg', type=int, default=10, help='shots per sequence')
    ap.add_argument('--depth', type=int, default=200)
    ap.add_argument('--over-rotation', type=float, default=0.0)
    ap.add_argument('--err', type=float, default=0.0, help='Pauli error probability per pulse')
    ap.add_argument('--shot-major', action='store_true')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--launches', type=int, default=5)
    ap.add_argument('--out', default=None)
    ap.add_argument('--lib', default=None, help="another build of libdpemu.so (A/B runs)")
    ap.add_argument('--measure', action='store_true',
                    help='dpemu_qsim_meas (qsim_kernel<meas>): the rdlo strobe of every lane measures')
    ap.add_argument('--decay', default=None, metavar='T1,T2',
                    help='also time dpemu_qsim_decay (qsim_kernel<meas,decay>) with these times on every core, in the '
                         'same rounds as qsim_kernel<meas> (implies --measure)')
    a = ap.parse_args()
    a.measure = a.measure or bool(a.decay)
    import torch
    ps = workloads.config4_rb2q_set(a.seqs, a.depth)
    ops = ps.words[:, 3] >> 28
    strobes = np.add.reduceat(((ops == isa.OP_PULSE_TRIG) | (ops == isa.OP_PULSE_RESET)).astype(np.int64),
                              ps.offsets.astype(np.int64))
    n = a.seqs * a.spg
    cfg = _abi.make_config(2, n_groups=ps.n_groups, shots_per_group=a.spg, max_cycles=1 << 20,
                           event_cap=int(strobes.max()) + 1, meas_cap=2, seed=0x5EED, exec_flags=_abi.X_STREAM_EVENTS,
                           lane_order=_abi.LANES_SHOT_MAJOR if a.shot_major else _abi.LANES_CORE_MAJOR)
    gs = workloads.rb2q_gateset(2, over_rotation=a.over_rotation, err_1q=a.err, err_2q=a.err)
    gs_decay = None
    if a.decay:
        t1, t2 = (float(v) for v in a.decay.split(','))
        gs_decay = workloads.rb2q_gateset(2, over_rotation=a.over_rotation, err_1q=a.err, err_2q=a.err)
        gs_decay.set_decay(0, t1, t2).set_decay(1, t1, t2)
    with Emulator(0, lib_path=a.lib) as emu:
        emu.load(ps)
        out = alloc_device_outputs(cfg, n, want=('summary', 'events'))
        pops = torch.empty((1, n, 4), dtype=torch.int64, device='cuda')
        res = torch.empty((1, n, 4), dtype=torch.int32, device='cuda')

        states = torch.empty((2 * n,), dtype=torch.int32, device='cuda') if a.measure else None

        def one_round():
            emu.run_device(cfg, n, 0, out)
            if a.measure:
                emu.simulate_gates(cfg, gs, out, n, pops=pops, result=res, measure=True, states=states)
            else:
                emu.simulate_gates(cfg, gs, out, n, pops=pops, result=res)
            if gs_decay is not None:
                emu.simulate_gates(cfg, gs_decay, out, n, pops=pops_d, result=res_d, measure=True, states=states_d,
                                   decay_counts=counts_d)
        per = 3 if gs_decay is not None else 2          # timed kernels per round
        if gs_decay is not None:
            pops_d, res_d, states_d = torch.empty_like(pops), torch.empty_like(res), torch.empty_like(states)
            counts_d = torch.empty((1, n, 4), dtype=torch.int32, device='cuda')
        for _ in range(a.warmup):
            one_round()
        torch.cuda.synchronize()
        emu.kernel_timing(True)
        for _ in range(a.launches):
            one_round()
        ms = emu.kernel_times()
        emu.kernel_timing(False)
        assert len(ms) == per * a.launches and emu.last_kernel() == (
            'qsim_kernel<meas,decay>' if gs_decay is not None else 'qsim_kernel<meas>' if a.measure else 'qsim_kernel')
        emu.run_device(cfg, n, 0, out)
        run_kernel = emu.last_kernel()
        torch.cuda.synchronize()
        r = res.cpu().numpy().view(np.uint32)
        n_ev = np.minimum(out['summary'][:, 2].cpu().numpy().view(np.uint32).astype(np.int64), cfg.event_cap)
        gates, ev_bytes = int(r[0, :, 1].sum()), int(n_ev.sum()) * 16
        assert not r[0, :, 2].any() and not (r[0, :, 3] >> 31).any()          # every pulse has its entry; nothing dropped
        surv = qsim.survival(r, a.spg)
        rec = {'seqs': a.seqs, 'shots_per_seq': a.spg, 'depth': a.depth, 'rows': n, 'event_cap': cfg.event_cap,
               'lane_order': 'shot_major' if a.shot_major else 'core_major', 'over_rotation': a.over_rotation,
               'err': a.err, 'launches': a.launches, 'lib': a.lib, 'measure': a.measure, 'gates': gates,
               'gates_per_row': gates / n,
               'event_bytes': ev_bytes, 'survival_mean': float(surv.mean()),
               'p00_mean': float((pops[0, :, 0].double() / 2.0 ** 60).mean().item()),
               'errors_per_row': float((r[0, :, 3] & 0xFFFF).mean()), 'run_kernel': run_kernel}
        q, k = spread(ms[1::per]), spread(ms[0::per])
        q.update(gates_per_s=gates / (q['ms_median'] * 1e-3), event_bytes_per_s=ev_bytes / (q['ms_median'] * 1e-3))
        rec['qsim_kernel'], rec['run_kernel_ms'] = q, k
        rec['qsim_to_run_ratio'] = q['ms_median'] / k['ms_median']
        if gs_decay is not None:
            d, c = spread(ms[2::per]), counts_d.cpu().numpy().view(np.uint32)[0]
            rec['decay'] = {'t1': t1, 't2': t2, 'kernel': d, 'ratio_to_meas': d['ms_median'] / q['ms_median'],
                            'jumps_per_row': float(c[:, [0, 2]].sum(axis=1).mean()),
                            'flips_per_row': float(c[:, [1, 3]].sum(axis=1).mean())}
    line = json.dumps(rec)
    print(line)
    if a.out:
        with open(a.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
