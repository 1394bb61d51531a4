"""bench.py as it is run for a measurement: a plain run times exactly --steps
steps, prints one lean JSON line and, with --dump-outputs, writes what its last
timed step computed -- checked here against oracle_fast, word for word."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHOTS, STEPS, WARMUP = 4096, 3, 1


@pytest.mark.gpu
@pytest.mark.fresh_process      # the benchmark is a process of its own: before this one touches the GPU
def test_plain_bench_run_dumps_the_last_steps_outputs(tmp_path):
    d = str(tmp_path / 'dump')
    r = subprocess.run([sys.executable, os.path.join(REPO, 'bench.py'), '--gpus', '1', '--steps', str(STEPS),
                        '--warmup', str(WARMUP), '--shots', str(SHOTS), '--dump-outputs', d],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith('{')]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line['steps'] == STEPS and line['warmup'] == WARMUP and line['n_gpus'] == 1
    assert line['unit'] == 'core-shots/s' and line['higher_is_better'] is True and line['dtype'] == 'u32'
    assert line['ms_per_step'] > 0
    assert line['value'] == pytest.approx(SHOTS * 8 / (line['ms_per_step'] * 1e-3), rel=1e-6)
    # nothing that takes runs of its own without --full
    for k in ('roofline', 'kernel_ms', 'cpu_baseline', 'timeline_gather', 'box', 'legs') + tuple(
            bench.ALL_LEGS.split(',')):
        assert k not in line, k

    got = {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}
    assert sorted(got) == ['events', 'hist', 'lanes', 'meas', 'summary']
    assert all(a.dtype == np.float64 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64 << 20
    ps, cfg = bench.ramsey_workload()
    ref = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, 0, SHOTS,
                          want=('summary', 'events', 'meas', 'hist'))
    np.testing.assert_array_equal(got['lanes'], np.arange(SHOTS * 8))      # every lane: they fit
    for k in ('summary', 'events', 'meas', 'hist'):
        assert got[k].shape == ref[k].shape, k
        np.testing.assert_array_equal(got[k], ref[k].astype(np.float64), err_msg=k)
