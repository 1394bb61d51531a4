"""dpemu_iq_stats (csrc/iq_stats.hip) on the GPU: the table and the outcome
bits equal the numpy restatement (tests/iq_stats_ref.py) bit for bit on
synthetic accumulator buffers -- both layouts, both lane orders, partial waves,
waves that straddle a core boundary, several workgroups, 32 slots with and
without supplied states -- and on a DEMOD run;
the calibrate -> apply -> rerun loop of readout.py; the argument checks of the
C ABI; the kernel name and timing record."""

import ctypes as C
import math
import types

import numpy as np
import pytest

from distributed_processor_amd import _abi, workloads
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.dds import ChannelPlan, DemodPairTable
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from distributed_processor_amd.readout import ReadoutStats
from tests import iq_stats_ref

pytestmark = pytest.mark.gpu

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


def synthetic(n_cols, cap, stride, seed):
    """random int32 acc (cap, n_cols, 2) with the extremes in it, and a counts
    array (n_cols, stride) of garbage whose count word (5 of a summary row, 0
    of a result row) is 0 .. cap + 1"""
    rng = np.random.default_rng(seed)
    acc = rng.integers(INT32_MIN, INT32_MAX, size=(cap, n_cols, 2), endpoint=True).astype(np.int32)
    ext = [INT32_MIN, INT32_MAX, -1, 0]
    for k, (a, b) in enumerate((a, b) for a in ext for b in ext):
        acc[k % cap, (7 * k) % n_cols, :] = (a, b)
    counts = rng.integers(0, 2 ** 32, size=(n_cols, stride), dtype=np.uint64).astype(np.uint32)
    word = 5 if stride == 8 else 0
    counts[:, word] = rng.integers(0, cap + 1, size=n_cols, endpoint=True)
    counts[:min(n_cols, 16 * cap), word] = cap                      # the extremes are counted
    return acc, counts, counts[:, word]


def config(C_, lane_order=_abi.LANES_CORE_MAJOR, seed=0x1234ABCD5EED, p1=None, meas_cap=3):
    rng = np.random.default_rng(C_)
    cfg = _abi.make_config(C_, seed=seed, lane_order=lane_order, meas_cap=meas_cap,
                           demod=dict(drv_elem=1, axis=[float(a) for a in rng.uniform(-4, 4, C_)],
                                      thr=int(rng.integers(-10 ** 8, 10 ** 8))))
    thr = p1 if p1 is not None else [0, 0xFFFFFFFF, 1 << 31] + [int(v) for v in rng.integers(0, 2 ** 32, 64)]
    for c in range(C_):
        cfg.p1_threshold[c] = thr[c] if C_ > 1 else 1 << 31
    return cfg


def to_dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).cuda()


def host(stats, bits):
    import torch
    torch.cuda.synchronize()
    return stats.cpu().numpy(), None if bits is None else bits.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize('n_shots', [37, 300])
@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR], ids=['core_major', 'shot_major'])
@pytest.mark.parametrize('C_', [1, 8, 64])
def test_run_layout_bit_exact(emu, C_, lane_order, n_shots):
    """37 shots: partial waves, and in core-major order waves that straddle a
    core boundary; 300 shots: several workgroups, the last one partial.  Shots
    run across 2^32."""
    cfg = config(C_, lane_order)
    n_cols, shot0 = n_shots * C_, 2 ** 32 - 20
    acc, counts, cnt = synthetic(n_cols, 3, 8, 100 * C_ + n_shots)
    d_acc, d_counts = to_dev(acc), to_dev(counts)
    for by_slot in (False, True):
        want_t, want_b = iq_stats_ref.iq_stats(cfg, acc, cnt, shot_begin=shot0, by_slot=by_slot)
        stats, bits = emu.iq_stats(cfg, d_acc, d_counts, shot_begin=shot0, by_slot=by_slot, bits=True)
        assert emu.last_kernel() == 'iq_stats_kernel'
        got_t, got_b = host(stats, bits)
        assert got_t.shape == ((3 if by_slot else 1), C_, 2, 16)
        np.testing.assert_array_equal(got_b, want_b)
        np.testing.assert_array_equal(got_t, want_t)
    assert want_t[..., 0].sum() == cnt.clip(max=3).sum() and (want_t[..., 0].sum(axis=(0, 2)) > 0).all()


# ---- 32 slots: the outcome bit and the state bit of slot 31, 32 grid rows ----
SLOTS32 = {'c8_core_major': (8, _abi.LANES_CORE_MAJOR, 300), 'c8_shot_major': (8, _abi.LANES_SHOT_MAJOR, 300),
           'c64_shot_major': (64, _abi.LANES_SHOT_MAJOR, 37), 'explicit': (8, _abi.LANES_CORE_MAJOR, None)}
SLOTS32_SHOT0 = 2 ** 32 - 20


def slots32_case(which):
    """(cfg, kw, acc, counts, cnt, states) at meas_cap 32: ``synthetic`` with counts 0 .. 33 over C x n_shots run
    columns (C 8 at 300 shots: a thread takes several columns, and in core-major order changes core; C 64 at 37
    shots) or 900 explicit columns, and per-column full-range state words with 0, 0xFFFFFFFF, 0x80000000 and
    0x55555555 among them.  kw: the layout's keywords of iq_stats_ref.iq_stats"""
    C_, lane_order, n_shots = SLOTS32[which]
    k = list(SLOTS32).index(which)
    cfg = config(C_, lane_order, seed=0x5107532 + k, meas_cap=32)
    rng = np.random.default_rng(3200 + k)
    if n_shots is None:
        n = 900
        core = rng.integers(0, C_, n).astype(np.uint32)
        shot = rng.permutation(5000)[:n].astype(np.uint64)       # (no (shot, core) twice: the injected reference keys by it)
        shot[::7] += np.uint64(2 ** 32)
        kw, stride = dict(core=core, shot=shot), 2
    else:
        n, kw, stride = C_ * n_shots, dict(shot_begin=SLOTS32_SHOT0), 8
    acc, counts, cnt = synthetic(n, 32, stride, 3300 + k)
    states = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    states[[3, 40, 77, 130]] = [0, 0xFFFFFFFF, 0x80000000, 0x55555555]          # (columns that count all 32 slots)
    return cfg, kw, acc, counts, cnt, states


@pytest.mark.parametrize('which', list(SLOTS32))
def test_32_slots_bit_exact(emu, which):
    """meas_cap 32 (reach: tests/test_iq_stats.py test_32_slot_cases_reach_slot_31): bits |= o << 31, 32 grid rows
    by slot with row 0 discriminating every slot while it counts its own, and supplied state words read up to
    bit 31 -- table and bits against the references, base and injected"""
    from tests import qsim_meas_ref
    cfg, kw, acc, counts, cnt, states = slots32_case(which)
    C_ = cfg.cores_per_shot
    d_acc, d_counts, d_states = to_dev(acc), to_dev(counts), to_dev(states)
    call = dict(kw)
    if 'core' in kw:
        call = dict(pairs=types.SimpleNamespace(n_pairs=len(cnt), n_lanes=len(cnt), cols=dict(kw, lane=np.arange(len(cnt)))))
    for by_slot in (False, True):
        want_t, want_b = iq_stats_ref.iq_stats(cfg, acc, cnt, by_slot=by_slot, **kw)
        stats, bits = emu.iq_stats(cfg, d_acc, d_counts, by_slot=by_slot, bits=True, **call)
        assert emu.last_kernel() == 'iq_stats_kernel'
        got_t, got_b = host(stats, bits)
        assert got_t.shape == ((32 if by_slot else 1), C_, 2, 16)
        np.testing.assert_array_equal(got_b, want_b)
        np.testing.assert_array_equal(got_t, want_t)
        want_t, want_b = qsim_meas_ref.iq_stats_st(states, cfg, acc, cnt, by_slot=by_slot, **kw)
        got_t, got_b = host(*emu.iq_stats(cfg, d_acc, d_counts, by_slot=by_slot, bits=True, states=d_states, **call))
        np.testing.assert_array_equal(got_b, want_b, err_msg='states=')
        np.testing.assert_array_equal(got_t, want_t, err_msg='states=')


def explicit_case(seed=9):
    rng = np.random.default_rng(seed)
    n = 500
    cfg = config(8, seed=0xFEEDFACE)
    core = rng.integers(0, 8, n).astype(np.uint32)
    shot = rng.integers(0, 5000, n).astype(np.uint64)
    shot[::7] += np.uint64(2 ** 32)
    shot[5::31] = np.uint64(2 ** 64 - 1) - shot[5::31]
    acc, counts, cnt = synthetic(n, 4, 2, seed)
    return cfg, types.SimpleNamespace(n_pairs=n, cols={'core': core, 'shot': shot}), acc, counts, cnt


def test_explicit_layout_bit_exact(emu):
    """500 columns with shuffled cores and non-monotonic shots, counts as a
    demodulate result (stride 2); then the same call again (the cached column
    table) and another table of the same size (re-uploaded)"""
    cfg, cols, acc, counts, cnt = explicit_case()
    d_acc, d_counts = to_dev(acc), to_dev(counts)
    for by_slot in (False, True, False):
        want_t, want_b = iq_stats_ref.iq_stats(cfg, acc, cnt, core=cols.cols['core'], shot=cols.cols['shot'],
                                               by_slot=by_slot)
        got_t, got_b = host(*emu.iq_stats(cfg, d_acc, d_counts, pairs=cols, by_slot=by_slot, bits=True))
        np.testing.assert_array_equal(got_b, want_b)
        np.testing.assert_array_equal(got_t, want_t)
    cols.cols['core'] = (cols.cols['core'] + 3) % 8
    want_t, _ = iq_stats_ref.iq_stats(cfg, acc, cnt, core=cols.cols['core'], shot=cols.cols['shot'])
    np.testing.assert_array_equal(host(*emu.iq_stats(cfg, d_acc, d_counts, pairs=cols))[0], want_t)


def test_options(emu):
    """per-core axis / thr overrides, p1_threshold all 0 / all 0xFFFFFFFF, no
    bits, a stats buffer full of 0x5A, another stream, no columns"""
    import torch
    n_shots, C_ = 50, 8
    cfg = config(C_, _abi.LANES_SHOT_MAJOR)
    acc, counts, cnt = synthetic(n_shots * C_, 3, 8, 77)
    d_acc, d_counts = to_dev(acc), to_dev(counts)
    rng = np.random.default_rng(3)
    axis = [_abi.axis_word(a) for a in rng.uniform(-4, 4, C_)]
    thr = [int(v) for v in rng.integers(-2 ** 31, 2 ** 31, C_)]
    thr[0], thr[1] = INT32_MIN, INT32_MAX
    base_t, base_b = iq_stats_ref.iq_stats(cfg, acc, cnt)
    for kw in (dict(axis=axis), dict(thr=thr), dict(axis=axis, thr=thr)):
        want_t, want_b = iq_stats_ref.iq_stats(cfg, acc, cnt, **kw)
        assert not np.array_equal(want_b, base_b)
        got_t, got_b = host(*emu.iq_stats(cfg, d_acc, d_counts, bits=True, **kw))
        np.testing.assert_array_equal(got_b, want_b)
        np.testing.assert_array_equal(got_t, want_t)
    for p1 in (0, 0xFFFFFFFF):
        c2 = config(C_, _abi.LANES_SHOT_MAJOR, p1=[p1] * C_)
        want_t, _ = iq_stats_ref.iq_stats(c2, acc, cnt)
        assert not want_t[:, :, 0 if p1 else 1].any()
        stats, bits = emu.iq_stats(c2, d_acc, d_counts)                 # bits=None: no bits output
        assert bits is None
        np.testing.assert_array_equal(host(stats, None)[0], want_t)
    # stats is assigned: a buffer full of garbage, on another stream
    for by_slot in (False, True):
        S = 3 if by_slot else 1
        buf = torch.full((S * C_ * 2 * 16 * 8,), 0x5A, dtype=torch.uint8, device='cuda').view(torch.int64)
        buf = buf.view(S, C_, 2, 16)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        stats, _ = emu.iq_stats(cfg, d_acc, d_counts, by_slot=by_slot, stats=buf, stream=side)
        side.synchronize()
        assert stats is buf
        np.testing.assert_array_equal(buf.cpu().numpy(), iq_stats_ref.iq_stats(cfg, acc, cnt, by_slot=by_slot)[0])
    # no columns: all-zero stats
    buf = torch.full((1, C_, 2, 16), 0x5A5A5A5A, dtype=torch.int64, device='cuda')
    e_acc = torch.empty((3, 0, 2), dtype=torch.int32, device='cuda')
    e_cnt = torch.empty((0, 8), dtype=torch.int32, device='cuda')
    stats, bits = emu.iq_stats(cfg, e_acc, e_cnt, stats=buf, bits=True)
    torch.cuda.synchronize()
    assert not buf.any().item() and bits.numel() == 0
    # the Python layer's own checks
    with pytest.raises(DpemuError):
        emu.iq_stats(cfg, d_acc[:, :-1].contiguous(), d_counts[:-1].contiguous())       # not whole shots
    with pytest.raises(DpemuError):
        emu.iq_stats(cfg, d_acc, d_counts[:, :3].contiguous())
    with pytest.raises(DpemuError):
        emu.iq_stats(cfg, d_acc, d_counts, thr=thr[:-1])


def test_timing_records_the_kernel(emu):
    cfg = config(8)
    acc, counts, cnt = synthetic(80, 3, 8, 5)
    d_acc, d_counts = to_dev(acc), to_dev(counts)
    emu.kernel_times()
    emu.kernel_timing(True)
    try:
        emu.iq_stats(cfg, d_acc, d_counts)
        ms = emu.kernel_times()
    finally:
        emu.kernel_timing(False)
    assert len(ms) == 1 and 0 < ms[0] < 100
    assert emu.last_kernel() == 'iq_stats_kernel'


def test_refusals_at_the_c_abi(emu):
    """every argument check: -22 and a message that names the field, before any launch"""
    import torch
    cfg = config(8)
    acc, counts, cnt = synthetic(16, 3, 8, 1)
    d_acc, d_counts = to_dev(acc), to_dev(counts)
    stats = torch.zeros((3, 8, 2, 16), dtype=torch.int64, device='cuda')
    bits = torch.zeros((16,), dtype=torch.int32, device='cuda')
    core, shot = np.arange(16, dtype=np.uint32) % 8, np.arange(16, dtype=np.uint64)

    def call(cfg_=cfg, cols=True, acc_=d_acc.data_ptr(), counts_=d_counts.data_ptr() + 20, stats_=stats.data_ptr(),
             core_=None, shot_=None, **f):
        st = _abi.IQColumns(16, 3, 0, 8)
        for k, v in f.items():
            setattr(st, k, v)
        if core_ is not None:
            st.core = core_.ctypes.data
        if shot_ is not None:
            st.shot = shot_.ctypes.data
        rc = emu._L.dpemu_iq_stats(emu._h, C.addressof(cfg_) if cfg_ is not None else None,
                                   C.addressof(st) if cols else None, acc_, counts_, stats_, bits.data_ptr(), None)
        return rc, emu._L.dpemu_last_error(emu._h)

    assert call()[0] == 0 and call(core_=core, shot_=shot)[0] == 0    # the baseline calls are accepted
    torch.cuda.synchronize()
    stats.zero_()
    bits.zero_()
    bad_core = core.copy()
    bad_core[9] = 8
    bad_order = config(8)
    bad_order.lane_order = 2
    bad_c = config(8)
    bad_c.cores_per_shot = 6
    for kw, field in ((dict(cfg_=None), b'cfg'), (dict(cols=False), b'cols'), (dict(acc_=None), b'acc'),
                      (dict(counts_=None), b'counts'), (dict(stats_=None), b'stats'),
                      (dict(meas_cap=0), b'meas_cap'), (dict(meas_cap=33), b'meas_cap'), (dict(by_slot=2), b'by_slot'),
                      (dict(count_stride=0), b'count_stride'), (dict(core_=core), b'shot'), (dict(shot_=shot), b'core'),
                      (dict(core_=bad_core, shot_=shot), b'core 8'), (dict(n_cols=12), b'multiple of cores_per_shot'),
                      (dict(n_cols=2 ** 31, meas_cap=2), b'2^31'), (dict(acc_=d_acc.data_ptr() + 4), b'aligned'),
                      (dict(cfg_=bad_order), b'lane_order'), (dict(cfg_=bad_c), b'cores_per_shot')):
        rc, msg = call(**kw)
        assert rc == -22 and field in msg, (kw, rc, msg)
    torch.cuda.synchronize()
    assert not stats.any().item() and not bits.any().item()           # nothing was launched


def test_demod_run_end_to_end(emu):
    """config 3's active reset under the DEMOD model, 256 shots x 8 cores:
    iq_stats' bits with cfg's own discriminator are the run's meas_bits; on the
    acc of a 16-pair waveform demodulation they are its result bits; and the
    calibration loop -- a run whose axes are rotated by pi / 2 (fidelity ~ 1/2),
    fit().apply, rerun -- reaches at least the fidelity of the analytically set
    axes on the same seed.  sigma = 60: the model's noise is bounded, |z| <=
    131070 sigma = 7.9e6 per quadrature, at most 1.11e7 along any axis, inside
    the +-1.97e7 signal (workloads.config3_demod) with 8.6e6 to spare for the
    fit's own error (~1e5 at 256 readouts per class) and apply's tolerance
    (4e6): the analytic and the fitted discriminator both assign every readout
    right, whatever the draws.  (At config 3's own sigma = 220, 1 % of the
    readouts are wrong and the two differ by sampling error of either sign.)"""
    import torch
    ps = ProgramSet(workloads.config3_active_reset(8))
    demod = workloads.config3_demod(ps, sigma=60.0)
    kw = dict(n_groups=ps.n_groups, max_cycles=50000, event_cap=16, meas_cap=4,
              meas_latency=workloads.CONFIG3_DEMOD_LATENCY, seed=0x5EED, p1=0.5, lane_order=_abi.LANES_SHOT_MAJOR)
    cfg = _abi.make_config(8, demod=demod, **kw)
    n, shot0 = 256, 3000
    emu.load(ps)

    def run(cfg_):
        out = alloc_device_outputs(cfg_, n, want=('summary', 'events', 'acc'))
        emu.run_device(cfg_, n, shot0, out)
        stats, bits = emu.iq_stats(cfg_, out['acc'], out['summary'], shot_begin=shot0, bits=True)
        t, b = host(stats, bits)
        return out, ReadoutStats(t, cfg_), b

    out, rs, bits = run(cfg)
    s = _abi.unpack_summary(out['summary'].cpu().numpy().view(np.uint32))
    assert (s['n_meas'] == 2).all()
    np.testing.assert_array_equal(bits, s['meas_bits'] & 3)
    assert rs.n.sum() == 2 * n * 8 and rs.n.min() > 150
    # a 16-pair sample through the waveforms
    who = [(shot0 + s_, c) for s_ in range(0, n, 128) for c in range(8)]
    params = {e: (d['samples_per_clk'], d['interp_ratio']) for e, d in enumerate(workloads.ELEMS)}
    drv = ChannelPlan(ps, cfg, shot0, n, [(s_, c, workloads.RDRV) for s_, c in who], params)
    lo = ChannelPlan(ps, cfg, shot0, n, [(s_, c, workloads.RDLO) for s_, c in who], params)
    iq_d = emu.synthesize(drv, out, 3200 * params[workloads.RDRV][0])
    iq_l = emu.synthesize(lo, out, 3200 * params[workloads.RDLO][0])
    pt = DemodPairTable(cfg, drv, lo)
    acc_w, res = emu.demodulate(cfg, drv, iq_d, lo, iq_l, out, pairs=pt)
    st_w, bits_w = host(*emu.iq_stats(cfg, acc_w, res, pairs=pt, bits=True))
    res_h = res.cpu().numpy().view(np.uint32)
    assert pt.n_pairs == 16 and (res_h[:, 0] == 2).all()
    np.testing.assert_array_equal(bits_w, res_h[:, 1])
    assert st_w[..., 0].sum() == 32 and st_w[..., 1].sum() == sum(bin(int(b)).count('1') for b in res_h[:, 1])
    # calibrate -> apply -> rerun
    rot = dict(demod, axis=[a + math.pi / 2 for a in demod['axis']])
    cfg_r = _abi.make_config(8, demod=rot, **kw)
    _, rs_rot, _ = run(cfg_r)
    d = rs_rot.fit()
    assert d.fitted[:8].all()
    d.apply(cfg_r, tol=4000000)
    _, rs_fit, _ = run(cfg_r)
    print('fidelity: analytic', rs.fidelity(), 'rotated', rs_rot.fidelity(), 'fitted', rs_fit.fidelity(),
          'thr', cfg_r.ro_thr, d.thr.tolist())
    assert 0.4 < rs_rot.fidelity() < 0.6
    assert rs_fit.fidelity() >= rs.fidelity() > 0.99
    for c in range(8):
        assert rs_fit.fidelity(core=c) >= rs.fidelity(core=c)
