"""Kernel time of iq_stats_kernel by the library's own event
pairs (dpemu_set_kernel_timing / dpemu_kernel_times), beside a torch.clone of
the same acc tensor in the same process as the bandwidth yardstick (it reads
and writes the tensor once: 2 x its bytes).  Shape: config 3's, --shots x
--cores lanes, shot-major, --meas-cap readouts each (default 1.25e6 x 8 x 2 =
160 MB of acc); acc is random int32, counts a summary-shaped tensor (n_meas
every --count-stride words, 8 as a run writes it).  --warmup launches of both,
then --launches interleaved pairs.  Prints one JSON line -- medians, min and
max of both and their ratio -- and appends it to --out."""

import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from distributed_processor_amd import _abi                      # noqa: E402
from distributed_processor_amd.emulator import Emulator         # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shots', type=int, default=1250000)
    ap.add_argument('--cores', type=int, default=8)
    ap.add_argument('--meas-cap', type=int, default=2)
    ap.add_argument('--count-stride', type=int, default=8, choices=(2, 8))
    ap.add_argument('--by-slot', action='store_true')
    ap.add_argument('--bits', action='store_true')
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--lib', default=None, help='another build of libdpemu.so (A/B)')
    ap.add_argument('--out', default=os.path.join(REPO, 'profiles', 'iq_stats_time.jsonl'))
    a = ap.parse_args()
    import torch
    n = a.shots * a.cores
    cfg = _abi.make_config(a.cores, meas_cap=a.meas_cap, lane_order=_abi.LANES_SHOT_MAJOR, p1=0.5,
                           demod=dict(drv_elem=1, axis=0.7, thr=1000))
    g = torch.Generator(device='cuda').manual_seed(1)
    acc = torch.randint(-2 ** 31, 2 ** 31, (a.meas_cap, n, 2), dtype=torch.int64, device='cuda', generator=g).to(torch.int32)
    counts = torch.zeros((n, a.count_stride), dtype=torch.int32, device='cuda')
    counts[:, 5 if a.count_stride == 8 else 0] = a.meas_cap
    bits = torch.empty((n,), dtype=torch.int32, device='cuda') if a.bits else None
    stats = None
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    clone_ms = []
    with Emulator(0, lib_path=a.lib) as emu:
        for k in range(a.warmup + a.launches):
            if k == a.warmup:
                torch.cuda.synchronize()
                emu.kernel_timing(True)
            stats, _ = emu.iq_stats(cfg, acc, counts, by_slot=a.by_slot, stats=stats, bits=bits)
            ev[0].record()
            c = torch.clone(acc)
            ev[1].record()
            ev[1].synchronize()
            if k >= a.warmup:
                clone_ms.append(ev[0].elapsed_time(ev[1]))
            del c
        ms = emu.kernel_times()
        emu.kernel_timing(False)
        name = emu.last_kernel()
        tab = stats.cpu().numpy()
    assert len(ms) == a.launches and int(tab[..., 0].sum()) == n * a.meas_cap
    readouts = n * a.meas_cap
    acc_bytes = 8 * readouts
    count_bytes = n * min(32, 4 * a.count_stride) * (a.meas_cap if a.by_slot else 1)   # a 32-B sector per column
    med, cmed = float(np.median(ms)), float(np.median(clone_ms))
    line = {'kernel': name, 'lib': a.lib, 'shots': a.shots, 'cores': a.cores, 'meas_cap': a.meas_cap, 'count_stride': a.count_stride,
            'by_slot': bool(a.by_slot), 'bits': bool(a.bits), 'launches': a.launches, 'readouts': readouts,
            'ms_median': med, 'ms_min': float(min(ms)), 'ms_max': float(max(ms)),
            'clone_ms_median': cmed, 'clone_ms_min': float(min(clone_ms)), 'clone_ms_max': float(max(clone_ms)),
            'ratio_to_clone': med / cmed, 'acc_bytes': acc_bytes, 'count_bytes': count_bytes,
            'readouts_per_s': readouts / (med * 1e-3), 'acc_bytes_per_s': acc_bytes / (med * 1e-3),
            'clone_bytes_per_s': 2 * acc_bytes / (cmed * 1e-3)}
    print(json.dumps(line))
    if a.out:
        with open(a.out, 'a') as f:
            f.write(json.dumps(line) + '\n')


if __name__ == '__main__':
    main()
