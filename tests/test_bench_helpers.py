"""bench.py on the CPU: the roofline / byte accounting helpers, the CPU
baseline's timing loop and thread count, and the committed bench line
(profiles/r02_bench.json) against the driver's JSON contract and its own
same-box rocprof evidence."""

import json
import os

import numpy as np
import pytest

import bench
from distributed_processor_amd import _abi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_hbm_roofline_caps_at_the_step_and_prefers_the_leg_profile(tmp_path, monkeypatch):
    prof = {'duration_ns': 200000.0, 'hbm_bytes_per_launch': 1.1e9}
    r = bench.hbm_roofline(1e9, kernel_ms=0.30, ms_per_step=0.25, kernel='k', prof=prof, rocprof_key='k')
    assert r['kernel_ms'] == 0.25 and r['kernel_ms_events'] == 0.30          # capped at the step
    assert r['achieved'] == pytest.approx(1e9 / 0.25e-3 / 1e9)
    assert r['frac'] == pytest.approx(r['achieved'] / bench.HBM_PEAK_GBS)
    assert r['traffic'] == 1.1e9
    assert r['kernel_ms_rocprof'] == pytest.approx(0.2)
    assert r['frac_rocprof'] == pytest.approx(1e9 / 0.2e-3 / 1e9 / bench.HBM_PEAK_GBS)
    # no per-leg duration: the --stats row of the kernel
    (tmp_path / (bench.PROFILE_TAG + '_kernel_stats.csv')).write_text('"Name","Calls","AverageNs"\n"void dpemu::my_kernel(x)",3,"150000"\n')
    monkeypatch.setattr(bench, 'PROFILE_DIR', str(tmp_path))
    r = bench.hbm_roofline(1e9, 0.2, 1.0, 'k', {'hbm_bytes_per_launch': None}, 'my_kernel')
    assert r['kernel_ms_rocprof'] == pytest.approx(0.15)
    assert 'kernel_ms_rocprof' not in bench.hbm_roofline(1e9, 0.2, 1.0, 'k', None, 'my_kernel')


def test_bytes_per_lane_counts_written_records_only():
    cfg = _abi.make_config(8, event_cap=8, meas_cap=2)
    s = np.zeros((3, 8), np.uint32)
    s[:, 2] = [0, 5, 20]          # n_events (20 > event_cap: 8 written)
    s[:, 5] = [0, 1, 9]           # n_meas (9 > meas_cap: 2 written)
    np.testing.assert_array_equal(bench.bytes_per_lane(s, cfg), [32.0, 32 + 80 + 8, 32 + 128 + 16])


def test_host_cores_respects_the_job_share(monkeypatch):
    aff = len(os.sched_getaffinity(0))
    monkeypatch.setenv('OMP_NUM_THREADS', '1')
    use, info = bench.host_cores()
    assert use == 1 and info['nproc'] == aff and info['omp_num_threads'] == '1'
    monkeypatch.delenv('OMP_NUM_THREADS')
    assert bench.host_cores()[0] == aff


def test_median_rate_times_a_fixed_sample():
    calls = []
    rate, n, times = bench.median_rate(lambda k: calls.append(k), units_per_n=8, n0=10, target_s=0.001, reps=5)
    assert len(calls) == 6 and calls[0] == 10 and set(calls[1:]) == {n} and len(times) == 5
    assert rate == pytest.approx(n * 8 / float(np.median(times)))


def _fake_outputs(cfg, n_shots, fill):
    """device-layout outputs on the CPU: every lane has written n_events = lane % 4
    and n_meas = lane % 3 records (more than meas_cap for some); the slots a run
    leaves untouched hold `fill`"""
    import torch
    L = n_shots * cfg.cores_per_shot
    lane = np.arange(L)
    summ = np.zeros((L, 8), np.uint32)
    summ[:, 0], summ[:, 2], summ[:, 5] = 0x80000000 + lane, lane % 4, lane % 3
    ev = np.full((cfg.event_cap, L, 4), fill, np.uint32)
    me = np.full((cfg.meas_cap, L, 2), fill, np.uint32)
    for j in range(cfg.event_cap):
        ev[j, lane % 4 > j] = (j << 24) + lane[lane % 4 > j, None] * 4 + np.arange(4)
    for j in range(cfg.meas_cap):
        me[j, lane % 3 > j] = 0xF0000000 + (j << 24) + lane[lane % 3 > j, None] * 2 + np.arange(2)
    out = {'summary': torch.from_numpy(summ.view(np.int32)), 'events': torch.from_numpy(ev.view(np.int32)),
           'meas': torch.from_numpy(me.view(np.int32))}
    return out, torch.arange(4 * 256, dtype=torch.int64).reshape(4, 256)


def test_sample_outputs_is_a_fixed_sample_free_of_unwritten_slots():
    cfg = _abi.make_config(8, n_groups=4, event_cap=3, meas_cap=1)
    a, hist = _fake_outputs(cfg, 500, 0xDEADBEEF)
    b, _ = _fake_outputs(cfg, 500, 0x12345678)            # another allocation's leftovers
    got = bench.sample_outputs(cfg, 500, a, hist, max_lanes=256)
    again = bench.sample_outputs(cfg, 500, b, hist, max_lanes=256)
    assert sorted(got) == ['events', 'hist', 'lanes', 'meas', 'summary']
    for k in got:
        assert got[k].dtype == np.float64
        np.testing.assert_array_equal(got[k], again[k])
    lanes = got['lanes'].astype(np.int64)
    assert len(lanes) == 256 and (np.diff(lanes) > 0).all() and lanes.max() < 4000
    assert len(set(lanes % 8)) == 8                       # not one core's lanes only
    assert got['summary'].shape == (256, 8) and got['events'].shape == (3, 256, 4) and got['meas'].shape == (1, 256, 2)
    np.testing.assert_array_equal(got['summary'][:, 0], 2.0 ** 31 + lanes)      # u32 words, exact
    for j in range(3):
        want = np.where((lanes % 4 > j)[:, None], (j << 24) + lanes[:, None] * 4 + np.arange(4), 0)
        np.testing.assert_array_equal(got['events'][j], want)
    want = np.where((lanes % 3 > 0)[:, None], 0xF0000000 + lanes[:, None] * 2 + np.arange(2), 0)
    np.testing.assert_array_equal(got['meas'][0], want)
    np.testing.assert_array_equal(got['hist'], np.arange(1024).reshape(4, 256))
    # everything when it fits
    small = bench.sample_outputs(cfg, 500, a, hist)
    np.testing.assert_array_equal(small['lanes'], np.arange(4000))
    assert small['events'].shape == (3, 4000, 4)


def _bench_line():
    with open(os.path.join(REPO, 'profiles', 'r02_bench.json')) as f:
        lines = [json.loads(x) for x in f if x.startswith('{')]
    assert len(lines) == 1, 'one JSON line'
    return lines[0]


def test_committed_bench_line_keeps_the_contract():
    d = _bench_line()
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['scaling'] == 'weak' and d['higher_is_better'] is True
    assert 'workload' in d['config']
    # value = emulated core-shots per second of the whole job
    assert d['value'] == pytest.approx(d['config']['shots_per_gpu'] * 8 / (d['ms_per_step'] * 1e-3), rel=1e-6)
    roof = d['roofline']
    for k in ('bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'):
        assert k in roof, k
    assert roof['frac'] == pytest.approx(roof['achieved'] / roof['peak'])
    cb = d['cpu_baseline']
    for k in ('value', 'unit', 'cores', 'kind', 'sample'):
        assert k in cb, k
    assert cb['kind'] in ('port', 'reference')


@pytest.mark.parametrize('leg', [None, 'dds', 'active_reset', 'rb'])
def test_committed_bench_agrees_with_its_same_box_rocprof(leg):
    """the bench's kernel time (HIP events inside real steps) and the rocprofv3
    kernel-trace average of the same launch, profiled on the same box"""
    d = _bench_line()
    x = d if leg is None else d[leg]
    roof = x['roofline']
    roof = roof.get('hbm', roof)
    assert roof['kernel_ms'] <= x['ms_per_step'] + 1e-9
    assert roof['kernel_ms_rocprof'] == pytest.approx(roof['kernel_ms'], rel=0.05)


def test_valu_view_recomputes_from_the_measured_peak():
    """the interpreter legs' VALU fractions: SQ_INSTS_VALU over the kernel time
    against the committed microbenchmark peak (profiles/r03_valu_peak_pmc.json)"""
    peak, cpi, variant = bench._valu_peak()
    assert 3e11 < peak < 1.3e12 and 2.0 <= cpi < 8.0 and 'kernel' in variant
    prof = {'SQ_INSTS_VALU': 1e8, 'duration_ns': 250000.0, 'valu_issue_pct': 50.0}
    v = bench.valu_view(prof, 0.2)
    assert v['achieved'] == pytest.approx(1e8 / 0.2e-3)
    assert v['frac'] == pytest.approx(1e8 / 0.2e-3 / peak)
    assert v['frac_rocprof'] == pytest.approx(1e8 / 0.25e-3 / peak)
    assert bench.valu_view({'duration_ns': 1.0}) is None
