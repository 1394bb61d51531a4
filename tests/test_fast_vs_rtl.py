"""oracle_fast (event-driven closed forms) vs oracle_rtl (per clock), bit for bit.

Every lane of every fuzzed shot must agree on: terminal state (t_end, ip,
qclk_end, instruction count, final registers), the full pulse-event stream
(cstrobe snapshots and pulse_reset), the register/qclk trace and the
measurement records.  Lanes that never finish (late triggers, deadlocks,
hang opcodes, runaway loops) are compared on every event up to the
simulated horizon.
"""

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi
from tests.progfuzz import pack_programs, random_case

HORIZON = 6000
EV_CAP, TR_CAP, MEAS_CAP = 128, 128, 16


def demod_tables(rng, n_programs):
    """random DEMOD frequency tables, one (drive, LO) pair per program: lengths
    0..600 (the fuzzer's 9-bit freq indices also land past them: words 0)"""
    tabs = [tuple(np.array([rng.getrandbits(32) for _ in range(rng.choice([0, 1, 5, 600]))], np.uint32)
                  for _ in range(2)) for _ in range(n_programs)]
    lens = [len(t) for pair in tabs for t in pair]
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint32)
    words = np.concatenate([t for pair in tabs for t in pair] + [np.zeros(0, np.uint32)]).astype(np.uint32)
    return tabs, (words, offs[0::2], np.array(lens[0::2], np.uint32), offs[1::2], np.array(lens[1::2], np.uint32))


def demod_params(rng, C, meas_elem=2):
    return dict(drv_elem=rng.choice([e for e in range(4) if e != meas_elem]), cpw=rng.randint(1, 8),
                delay=rng.choice([0, rng.randint(0, 40), 300]), theta=(rng.uniform(-4, 4), rng.uniform(-4, 4)),
                gain=(rng.random(), rng.random()), axis=[rng.uniform(-4, 4) for _ in range(C)],
                sigma=rng.choice([0.0, 0.5, 3.0, 200.0]), thr=rng.randint(-2 ** 22, 2 ** 22))


def run_both(case, n_shots=4, seed=0x5EED, meas_latency=20, sync_latency=1, sync_mask=0, shot0=0, readout=None,
             demod=None, p1=0.5, tables=None, **cfg_kw):
    """tables: the DEMOD frequency tables (words, drv_off, drv_len, lo_off, lo_len), one (drive, LO) pair per program
    (default: drawn from the case's rng); cfg_kw: further make_config arguments (lut_mask, lut_table, meas_elem)"""
    C = case['ncores']
    mode = _abi.FPROC_MEAS if case['mode'] == 'meas' else _abi.FPROC_LUT
    cfg = _abi.make_config(C, n_groups=case['n_groups'], shots_per_group=1, max_cycles=HORIZON,
                           event_cap=EV_CAP, trace_cap=TR_CAP, meas_cap=MEAS_CAP, fproc_mode=mode,
                           meas_latency=meas_latency, sync_latency=sync_latency, sync_mask=sync_mask,
                           seed=seed, p1=p1, readout=readout, demod=demod, **cfg_kw)
    words, offs, ni = pack_programs(case['progs'])
    if tables is not None:
        w, d_off, d_len, l_off, l_len = (np.asarray(a, np.uint32) for a in tables)
        ro = (w, d_off, d_len, l_off, l_len)
        tabs = [(w[int(d_off[p]):int(d_off[p]) + int(d_len[p])], w[int(l_off[p]):int(l_off[p]) + int(l_len[p])])
                for p in range(len(case['progs']))]
    else:
        tabs, ro = demod_tables(case['rng'], len(case['progs'])) if demod is not None else (None, None)
    fast = oracle.fast_run(cfg, words, offs, ni, case['table'], shot0, n_shots, ro=ro)
    scfg = oracle.shot_cfg_from_config(cfg)
    rtl = []
    for s in range(n_shots):
        shot = shot0 + s
        g = shot % case['n_groups']
        prs = [int(case['table'][g * C + c]) for c in range(C)]
        progs = [np.asarray(__import__('distributed_processor_amd').isa.words_to_u32(case['progs'][p])) for p in prs]
        ok, lanes = oracle.rtl_run_shot(scfg, progs, shot, HORIZON + 16, EV_CAP, TR_CAP, MEAS_CAP,
                                        ro_tabs=[tabs[p] for p in prs] if tabs else None)
        rtl.append(lanes)
    return cfg, fast, rtl


def compare(cfg, fast, rtl, n_shots):
    C = cfg.cores_per_shot
    n_lanes = n_shots * C
    summ = _abi.unpack_summary(fast['summary'])
    stats = {'done': 0, 'other': 0, 'events': 0}
    for s in range(n_shots):
        for c in range(C):
            L = c * n_shots + s                     # core-major lanes
            r = rtl[s][c]
            ne = min(int(summ['n_events'][L]), EV_CAP)
            fev = fast['events'][:ne, L]
            nt = min(int(summ['n_trace'][L]), TR_CAP)
            ftr = fast['trace'][:nt, L]
            nm = min(int(summ['n_meas'][L]), MEAS_CAP)
            fms = fast['meas'][:nm, L]
            ctx = 'shot {} core {}'.format(s, c)
            if r['status'] == _abi.ST_DONE:
                stats['done'] += 1
                assert summ['status'][L] == _abi.ST_DONE, ctx
                assert summ['t_end'][L] == r['t_end'], ctx
                assert summ['ip'][L] == r['ip'], ctx
                assert summ['qclk_end'][L] == r['qclk_end'], ctx
                assert summ['n_instr'][L] == r['n_instr'], ctx
                assert summ['n_events'][L] == r['n_events'], ctx
                np.testing.assert_array_equal(fev, r['events'], err_msg=ctx)
                assert summ['n_trace'][L] == r['n_trace'], ctx
                np.testing.assert_array_equal(ftr, r['trace'], err_msg=ctx)
                assert summ['n_meas'][L] == r['n_meas'], ctx
                np.testing.assert_array_equal(fms, r['meas'], err_msg=ctx)
                if 'acc' in fast:
                    np.testing.assert_array_equal(fast['acc'][:nm, L], r['acc'], err_msg=ctx)
                assert summ['meas_bits'][L] == r['meas_bits'], ctx
                np.testing.assert_array_equal(fast['regs'][:, L], r['regs'], err_msg=ctx)
            else:
                stats['other'] += 1
                assert summ['status'][L] != _abi.ST_DONE, ctx
                lim = HORIZON - 16
                fe = fev[fev[:, 0] <= lim]
                re_ = r['events'][r['events'][:, 0] <= lim] if len(r['events']) else r['events']
                np.testing.assert_array_equal(fe, re_.reshape(-1, 4), err_msg=ctx)
                ft = ftr[ftr[:, 0] <= lim]
                rt = r['trace'][r['trace'][:, 0] <= lim] if len(r['trace']) else r['trace']
                np.testing.assert_array_equal(ft, rt.reshape(-1, 4), err_msg=ctx)
            stats['events'] += ne
    return stats


@pytest.mark.parametrize('seed', range(60))
def test_fuzz_fast_vs_rtl(seed):
    case = random_case(seed)
    n_shots = 3
    cfg, fast, rtl = run_both(case, n_shots=n_shots, shot0=seed * 7)
    compare(cfg, fast, rtl, n_shots)


@pytest.mark.parametrize('seed', range(20))
def test_fuzz_multicore_sync_fproc(seed):
    case = random_case(1000 + seed, ncores=4, mode='meas', allow_late=False, allow_hang=False)
    cfg, fast, rtl = run_both(case, n_shots=3, meas_latency=1 + seed % 5, sync_latency=1 + seed % 3)
    st = compare(cfg, fast, rtl, 3)
    assert st['events'] > 0


@pytest.mark.parametrize('seed', range(20))
def test_fuzz_lut(seed):
    case = random_case(2000 + seed, ncores=4, mode='lut', allow_late=False, allow_hang=False)
    cfg, fast, rtl = run_both(case, n_shots=3, meas_latency=2 + seed % 7)
    compare(cfg, fast, rtl, 3)


def test_fuzz_mostly_finishes():
    """guard against a fuzzer that only produces non-terminating lanes"""
    done = other = 0
    for seed in range(30):
        case = random_case(seed, allow_late=False, allow_hang=False, mode='meas')
        cfg, fast, rtl = run_both(case, n_shots=2)
        st = compare(cfg, fast, rtl, 2)
        done += st['done']
        other += st['other']
    assert done > 3 * other


@pytest.mark.parametrize('seed', range(10))
def test_fuzz_partial_sync_mask(seed):
    """cores outside sync_mask that execute SYNC never get ready (DEADLOCK);
    the participants' barriers complete without them"""
    case = random_case(3000 + seed, ncores=4, mode='meas', allow_late=False, allow_hang=False)
    cfg, fast, rtl = run_both(case, n_shots=2, sync_mask=0b0111, sync_latency=1 + seed % 4)
    compare(cfg, fast, rtl, 2)


@pytest.mark.parametrize('seed', range(16))
def test_fuzz_readout_model(seed):
    """meas_model READOUT (include/dpemu.h): outcomes from the discriminated
    readout of each strobe's amp word, driving fproc branches in both models"""
    case = random_case(4000 + seed, ncores=[1, 2, 4][seed % 3], mode=['meas', 'lut'][seed % 2],
                       allow_late=False, allow_hang=False)
    ro = dict(sep=[40000, 5000, -30000, 0][seed % 4], sigma=[0.5, 1.0, 0.1, 2.0][seed % 4], thr=[0, 1000, -500][seed % 3],
              win=[0, 7, 300, 4095][(seed // 4) % 4])
    cfg, fast, rtl = run_both(case, n_shots=3, meas_latency=1 + seed % 9, readout=ro)
    compare(cfg, fast, rtl, 3)


@pytest.mark.parametrize('seed', range(24))
def test_fuzz_demod_model(seed):
    """meas_model DEMOD (include/dpemu.h, oracle/readout.c): random drive / LO
    elements, windows, delays, frequency tables and discriminators; outcomes,
    meas_valid cycles and the accumulated {I, Q} agree per clock and event-driven,
    and drive fproc branches in both back ends"""
    import random
    case = random_case(5000 + seed, ncores=[1, 2, 4][seed % 3], mode=['meas', 'lut'][seed % 2],
                       allow_late=False, allow_hang=False)
    d = demod_params(random.Random(seed), case['ncores'])
    cfg, fast, rtl = run_both(case, n_shots=3, meas_latency=1 + seed % 9, demod=d)
    compare(cfg, fast, rtl, 3)
    assert 'acc' in fast
