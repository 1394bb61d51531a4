"""GPU tests of dpemu_run_states (include/dpemu.h): the interpreter with every
readout's prepared state supplied by the caller, branch_kernel<FEAT | 128>.

oracle/ cannot take a states buffer, so the variant is pinned to it through
draw equivalence: with the STATE model, dpemu_run_states under seed A with the
words that pack seed B's Philox draws (tests/qsim_meas_ref.draw_words) must
equal oracle_fast under seed B in every output; with the READOUT model, where
the noise comes from the run's own seed, A = B and the result must equal both
the oracle and dpemu_run.  Then the bits at and above 32, states = NULL, and the
refusals."""

import ctypes as C
import functools

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, isa, workloads
from distributed_processor_amd._native import DpemuError
from distributed_processor_amd.emulator import Emulator, ProgramSet, alloc_device_outputs
from tests.feature_cases import compare, device_run, drawn_states, paths_differ, without_register_writes
from tests.progfuzz import random_case

pytestmark = pytest.mark.gpu

ALL_OUT = ('summary', 'events', 'trace', 'meas', 'regs', 'hist')
CM, SM = _abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR
SEED_A, SEED_B = 0xA11CE5EED, 0xB0B5EED00F
SPG = 32                # shots per program group: a workgroup spans few groups, so short programs are staged in LDS


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


# (fuzz seed, cores, fproc mode, n_shots, lane order, exec_flags, keep register writes, first shot, kind)
# kind: None = jumps / fproc / sync; 'straight' = pulse-only; 'linear' = branch-free with registers.
# Seeds: chosen on the CPU (oracle_fast alone) so that every case has a sync and an fproc read where its
# kind allows them, no lane measures more than 32 times, and seed B's draws change some lane's path.
CASES = [
    (9, 2, 'meas', 200, CM, 0, True, 0, None),
    (9, 2, 'meas', 37, SM, _abi.X_PROG_MAJOR, True, 0, None),
    (17, 8, 'lut', 37, CM, 0, True, 0, None),
    (17, 8, 'lut', 200, SM, _abi.X_PROG_MAJOR, True, 5000, None),
    (12, 16, 'meas', 37, SM, 0, True, 0, None),             # (too long to stage: workloads of 16 cores that are
    (9, 1, 'meas', 200, CM, 0, True, 0, None),              #  staged run in tests/test_gpu_cosim.py)
    (13, 8, 'meas', 200, SM, 0, False, 123457, None),       # 511 commands with the guards: staged, one below the cap
    (13, 8, 'meas', 37, CM, _abi.X_PROG_MAJOR, False, 0, None),
    (27, 2, 'lut', 200, CM, 0, False, 0, None),
    (9001, 8, 'meas', 200, CM, 0, True, 0, 'straight'),
    (15001, 2, 'meas', 37, SM, 0, True, 77, 'linear'),
]
CASE_IDS = ['{}{}-c{}-{}-n{}-{}-x{:x}{}'.format(k or 'fuzz', s, c, m, n, 'sm' if o else 'cm', f, '' if r else '-noregs')
            for s, c, m, n, o, f, r, _, k in CASES]


@functools.lru_cache(maxsize=None)
def programs_of(seed, C_, mode, regs, kind):
    case = random_case(seed, ncores=C_, mode=mode, allow_late=True, allow_hang=True, straight=kind == 'straight',
                       linear=kind == 'linear')
    progs = case['progs'] if regs else without_register_writes(case['progs'])
    groups = [[progs[case['table'][g * C_ + c]] for c in range(C_)] for g in range(case['n_groups'])]
    return ProgramSet(groups, cores_per_shot=C_)


def config_of(ps, seed, fuzz_seed, mode, order, flags, **kw):
    C_ = ps.cores_per_shot
    p1 = [(0.5, 0.3, 0.8, 0.05, 0.95, 0.6, 1.0, 0.0)[c % 8] for c in range(C_)]
    return _abi.make_config(C_, n_groups=ps.n_groups, shots_per_group=SPG, max_cycles=6000, event_cap=64,
                            trace_cap=64, meas_cap=16,
                            fproc_mode=_abi.FPROC_MEAS if mode == 'meas' else _abi.FPROC_LUT,
                            meas_latency=1 + fuzz_seed % 23, sync_latency=1 + fuzz_seed % 3, seed=seed, p1=p1,
                            lane_order=order, exec_flags=flags, **kw)


def staged_in_lds(ps, cfg):
    """csrc/launch_plan.h's rule for branch.hip: the programs of the groups a workgroup of 256 / C shots can span,
    each with its guard command, within BRANCH_LDS_MAX = 512 commands, unless DPEMU_X_PROG_MAJOR keeps the global fetch"""
    C_, ng = cfg.cores_per_shot, cfg.n_groups
    w = 1 if ng == 1 else (256 // C_ - 1) // cfg.shots_per_group + 2
    if w * C_ > 256 or cfg.exec_flags & _abi.X_PROG_MAJOR:
        return False
    gl = [sum(int(ps.n_instr[ps.table[g * C_ + c]]) + 1 for c in range(C_)) for g in range(ng)]
    best = max(sum(gl[(g + i) % ng] for i in range(w % ng)) for g in range(ng))
    return (w // ng) * sum(gl) + best <= 512


def outs_of(cfg):
    return tuple(k for k in ALL_OUT if k != 'hist' or cfg.cores_per_shot <= 12)


# ---- 4. draw equivalence, STATE model ----

@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_states_from_another_seeds_draws_equal_the_oracle_under_that_seed(emu, case):
    fuzz_seed, C_, mode, n_shots, order, flags, regs, shot0, kind = case
    ps = programs_of(fuzz_seed, C_, mode, regs, kind)
    cfg_a = config_of(ps, SEED_A, fuzz_seed, mode, order, flags)
    cfg_b = config_of(ps, SEED_B, fuzz_seed, mode, order, flags)
    outs = outs_of(cfg_a)
    ora = lambda cfg: oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, shot0, n_shots, want=outs)
    fa, fb = ora(cfg_a), ora(cfg_b)
    n_meas = fb['summary'].reshape(-1, 8)[:, 5]
    assert n_meas.max() <= 32, n_meas.max()             # every readout's state is a bit of the lane's word
    assert (fa['summary'].reshape(-1, 8)[:, 6] != fb['summary'].reshape(-1, 8)[:, 6]).any()   # the draws differ
    if kind is None:
        ops = {isa.decode(int(w[0]) | int(w[1]) << 32 | int(w[2]) << 64 | int(w[3]) << 96)['op'] for w in ps.words}
        assert 'sync' in ops or C_ == 1
        assert ops & {'alu_fproc', 'jump_fproc'}
        assert regs == bool(ops & {'alu_fproc', 'reg_alu'})
        assert paths_differ(fa, fb).any()               # some lane takes a branch it would not take under seed A
    states = drawn_states(cfg_b, n_shots, shot0, max(1, int(n_meas.max())))
    got = device_run(emu, ps, cfg_a, n_shots, shot0, states, outs)
    name = emu.last_kernel()
    want_feat = 0x80 | (0 if kind == 'straight' else 0x20 if regs else 0)
    feat = int(name.split('feat=0x')[1].split(',')[0].rstrip('>'), 16)
    assert name.startswith('branch_kernel<feat=0x') and feat & 0xA0 == want_feat, name
    assert bool(feat & 8) == staged_in_lds(ps, cfg_a), name             # LDS-staged, or the global fetch
    assert name.endswith(',c8>') == (C_ == 8), name
    compare(got, fb, 'oracle under seed B')


# ---- 5. READOUT model: the noise is the run's own, so A = B ----

@pytest.mark.parametrize('case', [CASES[0], CASES[3], CASES[6]], ids=[CASE_IDS[0], CASE_IDS[3], CASE_IDS[6]])
def test_readout_model_with_its_own_draws_is_dpemu_run(emu, case):
    fuzz_seed, C_, mode, n_shots, order, flags, regs, shot0, kind = case
    ps = programs_of(fuzz_seed, C_, mode, regs, kind)
    # the fuzz programs' amplitude words are uniform in [0, 2^16): s = sep A >> 16 spans [0, 3000) against a noise
    # sigma of 0.02 * 37838 = 757, so readouts on both sides of the threshold are common
    cfg = config_of(ps, SEED_A, fuzz_seed, mode, order, flags, readout=dict(sep=3000, sigma=0.02, thr=0))
    assert cfg.meas_model == _abi.MEAS_READOUT
    outs = outs_of(cfg)
    f = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, shot0, n_shots, want=outs)
    n_meas = f['summary'].reshape(-1, 8)[:, 5]
    assert n_meas.max() <= 32
    states = drawn_states(cfg, n_shots, shot0, max(1, int(n_meas.max())))
    # the model matters: some outcome is not its prepared state
    lanes = np.flatnonzero(n_meas > 0)
    m0 = f['meas'].reshape(cfg.meas_cap, -1, 2)[0, lanes, 1]
    assert (m0 != (states[lanes] & 1)).any()
    got = device_run(emu, ps, cfg, n_shots, shot0, states, outs)
    assert emu.last_kernel().startswith('branch_kernel<feat=0x')
    compare(got, f, 'oracle')
    base = device_run(emu, ps, cfg, n_shots, shot0, None, outs)
    compare(got, base, 'dpemu_run')


# ---- 6. bits at and above 32 ----

def test_readouts_from_the_33rd_on_are_prepared_in_zero(emu):
    n_ro, n_shots = 34, 37
    words = [isa.pulse_reset()]
    words += [isa.pulse_i(freq_word=1, phase_word=0, amp_word=1000, env_word=0x004001, cfg_word=workloads.RDLO,
                          cmd_time=10 + 8 * k) for k in range(n_ro)]
    words.append(isa.done_cmd())
    ps = ProgramSet([[words]], cores_per_shot=1)
    cfg = _abi.make_config(1, max_cycles=4000, event_cap=40, meas_cap=32, meas_latency=3, seed=1, p1=0.0)
    outs = ('summary', 'events', 'meas', 'hist')
    got = device_run(emu, ps, cfg, n_shots, 0, np.full(n_shots, 0xFFFFFFFF, np.uint32), outs)
    assert emu.last_kernel().startswith('branch_kernel<feat=0x8')
    s = got['summary'].reshape(-1, 8)
    assert (s[:, 6] == 0xFFFFFFFF).all() and (s[:, 5] == n_ro).all()
    assert ((s[:, 1] >> 24) & _abi.F_MEAS_OVF).all() and ((s[:, 1] >> 16) & 0xFF == _abi.ST_DONE).all()
    assert (got['meas'].reshape(32, n_shots, 2)[:, :, 1] == 1).all()
    # the histogram key's bit is the LAST outcome, readout 33's: prepared in 0 (a shift by 33 & 31 would read bit 1)
    assert got['hist'].reshape(-1).tolist() == [n_shots, 0]
    # and everything but the outcomes is what the draws at p1 = 1 give
    one = _abi.make_config(1, max_cycles=4000, event_cap=40, meas_cap=32, meas_latency=3, seed=1, p1=1.0)
    f = oracle.fast_run(one, ps.words, ps.offsets, ps.n_instr, ps.table, 0, n_shots, want=outs)
    compare({k: got[k] for k in ('summary', 'events', 'meas')}, {k: f[k] for k in ('summary', 'events', 'meas')}, 'p1 = 1')
    assert f['hist'].reshape(-1).tolist() == [0, n_shots]


# ---- 7. states = NULL is dpemu_run; the refusals ----

def raw_entry(emu, cfg, n_shots, shot0, ptr_of):
    """dpemu_run_states called through the binding with the states pointer ptr_of(tensor) gives"""
    def entry(dev, st):
        o = _abi.Outputs()
        for name, _ in _abi.Outputs._fields_:
            setattr(o, name, dev[name].data_ptr() if name in dev else None)
        emu._call('dpemu_run_states', (C.addressof(cfg), int(shot0), int(n_shots), C.addressof(o), ptr_of(st)), None)
    return entry


@pytest.mark.parametrize('which', ['config1', 'config3'])
def test_null_states_is_dpemu_run(emu, which):
    if which == 'config1':
        ps = ProgramSet(workloads.config1_linear())
        cfg = _abi.make_config(1, max_cycles=10000, event_cap=8, trace_cap=8, meas_cap=4)
    else:
        ps = ProgramSet(workloads.config3_active_reset(8))
        cfg = _abi.make_config(8, max_cycles=50000, event_cap=16, trace_cap=16, meas_cap=4,
                               meas_latency=workloads.CONFIG3_MEAS_LATENCY)
    n_shots = 200
    base = device_run(emu, ps, cfg, n_shots, 11, None, ALL_OUT)
    name = emu.last_kernel()
    assert name.startswith('straight_kernel<' if which == 'config1' else 'branch_kernel<feat=0xb,c8>')
    got = device_run(emu, ps, cfg, n_shots, 11, None, ALL_OUT, entry=raw_entry(emu, cfg, n_shots, 11, lambda st: None))
    assert emu.last_kernel() == name
    compare(got, base, 'dpemu_run')
    # n_shots = 0 behaves as dpemu_run and does not touch states (a pointer that could not be read)
    none = _abi.Outputs()
    emu._call('dpemu_run_states', (C.addressof(cfg), 0, 0, C.addressof(none), C.c_void_p(4096)), None)


def test_refusals(emu):
    import torch
    ps = ProgramSet(workloads.config3_active_reset(8))
    emu.load(ps)
    n_shots = 37
    cfg = _abi.make_config(8, max_cycles=50000, event_cap=16, meas_cap=4, meas_latency=workloads.CONFIG3_MEAS_LATENCY)
    dev = alloc_device_outputs(cfg, n_shots, want=('summary', 'events'))
    ok = torch.zeros(n_shots * 8 + 1, dtype=torch.int32, device='cuda')
    # Python: size, dtype, device
    for bad in (ok, ok[:-2], ok[:-1].to(torch.int64), ok[:-1].cpu(), ok[:-1].reshape(n_shots, 8), [0] * (n_shots * 8)):
        with pytest.raises(DpemuError, match='states'):
            emu.run_device(cfg, n_shots, 0, dev, states=bad)
    emu.run_device(cfg, n_shots, 0, dev, states=ok[:-1])
    # C: a misaligned pointer (two bytes into the buffer), before any launch
    before = emu.last_kernel()
    entry = raw_entry(emu, cfg, n_shots, 0, lambda st: C.c_void_p(st.data_ptr() + 2))
    with pytest.raises(DpemuError, match='4-byte aligned'):
        entry(dev, ok)
    # everything dpemu_run refuses
    worse = _abi.make_config(8, max_cycles=50000, event_cap=16, meas_cap=4)
    worse.meas_cap = 33
    with pytest.raises(DpemuError):
        emu.run_device(worse, n_shots, 0, dev, states=ok[:-1])
    # DEMOD with states: the C message, in Python and in C (with the frequency tables loaded, so nothing else is wrong)
    demod = _abi.make_config(8, max_cycles=50000, event_cap=16, meas_cap=4,
                             meas_latency=workloads.CONFIG3_DEMOD_LATENCY, demod=workloads.config3_demod(ps))
    with pytest.raises(DpemuError, match='DEMOD with states'):
        emu.run_device(demod, n_shots, 0, dev, states=ok[:-1])
    emu._demod_tables(demod)
    entry = raw_entry(emu, demod, n_shots, 0, lambda st: C.c_void_p(st.data_ptr()))
    with pytest.raises(DpemuError, match='DEMOD with states'):
        entry(dev, ok)
    entry = raw_entry(emu, demod, n_shots, 0, lambda st: None)      # ... and without states a DEMOD run is dpemu_run
    entry(dev, ok)
    assert emu.last_kernel().startswith('branch_kernel<feat=0x4') and before.startswith('branch_kernel<feat=0x8b')
    torch.cuda.synchronize()
