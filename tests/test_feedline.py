"""The multiplexed readout stages (dpemu_feedline_adc / dpemu_demod_feedline,
include/dpemu.h; DESIGN.md §2 "Multiplexed readout") on the CPU: their numpy
restatement (tests/feedline_ref.py) applied to oracle_dds waveforms -- the
degenerate equivalence with dpemu_demod_iq, the orthogonality of tones spaced
by whole turns per window, the clipping converter and the per-member state
switching -- and the Python-side feedline table.  The GPU kernels are held to
the same restatement bit for bit in tests/test_gpu_feedline.py.

Tolerance of the tone tests: tests/test_demod_iq.py's flat_tolerance of the
neighbour's accumulator at its own LO (REL_TOL |acc| + ABS_TOL): the leakage is
that accumulator's sum with the tone's phase advancing by the detuning, so it
carries the same 12-bit carrier phases and 32767 / 32768 factors (relative)
and the same per-sample roundings (absolute)."""

import math

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, isa
from distributed_processor_amd._native import DpemuError
from tests import demod_iq_ref, feedline_ref
from tests.progfuzz import pack_programs
from tests.test_demod import RDLO, RDRV, ro_program
from tests.test_demod_iq import SQUARE, flat_tolerance, freq_buffer


def fl_cfg(C_, delay=0, theta=(0.3, 2.0), gain=(1.0, 1.0), p1=0.5, sigma=0.0, meas_cap=4, axis=0.0, seed=0x5EED,
           event_cap=16, thr=0):
    return _abi.make_config(C_, max_cycles=1 << 22, event_cap=event_cap, meas_cap=meas_cap, meas_latency=32, p1=p1,
                            seed=seed, demod=dict(drv_elem=RDRV, cpw=4, delay=delay, theta=theta, gain=gain,
                                                  sigma=sigma, axis=axis, thr=thr))


def synth_cores(progs, cfg, f_d, f_lo, spc, interp, env, n_clks, n_shots=1, shot0=0):
    """len(progs) cores (one group), core c running progs[c] with drive / LO
    frequency words f_d[c] / f_lo[c]: oracle.fast_run, then oracle.dds of the
    drive and LO channel of every (shot, core).  Pair s * C + c is (shot0 + s,
    core c), rows likewise.  Returns (outputs, pair columns, iq_drv, iq_lo)."""
    C_ = len(progs)
    assert C_ == cfg.cores_per_shot
    pw, offs, ni = pack_programs(progs)
    words = np.array([w for c in range(C_) for w in (f_d[c], f_lo[c])], np.uint32)
    idx = np.arange(C_, dtype=np.uint32)
    ro = (words, 2 * idx, np.ones(C_, np.uint32), 2 * idx + 1, np.ones(C_, np.uint32))
    out = oracle.fast_run(cfg, pw, offs, ni, idx, shot0, n_shots, ro=ro)
    assert ((out['summary'].view(np.uint32)[:, 1] >> 16) & 0xFF == _abi.ST_DONE).all()
    who = [(s_, c) for s_ in range(n_shots) for c in range(C_)]
    lanes = [int(_abi.lane_index(s_, c, n_shots, C_, cfg.lane_order)) for s_, c in who]
    iq = []
    for elem, f, s_, ip in ((RDRV, f_d, spc[0], interp[0]), (RDLO, f_lo, spc[1], interp[1])):
        fbs = [freq_buffer(int(f[c]), s_) for c in range(C_)]
        desc = [(lane, elem, s_, ip, 0, len(env), 16 * c, 16) for lane, (_, c) in zip(lanes, who)]
        assert all(len(b) == 16 for b in fbs)
        iq.append(oracle.dds(desc, out['summary'], out['events'], env, np.concatenate(fbs), n_clks * s_,
                             cfg.event_cap))
    n = len(who)
    pairs = dict(lane=np.array(lanes), core=np.array([c for _, c in who]),
                 shot=shot0 + np.array([s_ for s_, _ in who]), drv_row=np.arange(n), lo_row=np.arange(n),
                 spc_drv=[spc[0]] * n, spc_lo=[spc[1]] * n)
    return out, pairs, iq[0], iq[1]


def run_ref(cfg, pairs, lines, out, iq_d, iq_l, meas_cap=None):
    return feedline_ref.feedline(cfg, pairs, lines, out['summary'], out['events'], iq_d, iq_l,
                                 cfg.meas_cap if meas_cap is None else meas_cap)


def iq16(words):
    return demod_iq_ref.s16(words), demod_iq_ref.s16(np.asarray(words).view(np.uint32) >> 16)


def test_degenerate_equivalence():
    """one member per line, unit gains, windows that end before the lane's next
    readout strobe: acc and result are dpemu_demod_iq's exactly (16:4 and 1:1,
    noise on); with a gain below one they are not -- the gain is applied per
    sample here, to the sum there"""
    env = np.full(4 * 260, SQUARE, np.uint32)
    for spc in ((16, 4), (1, 1)):
        reads = [[dict(A=30000 + 9000 * c + 1000 * k, ph_d=9000 * k + c, ph_lo=555 * c, L_d=L, L_lo=L, lo_at=140,
                       gap=1300) for k, L in enumerate((1, 7, 250))] for c in range(2)]
        for gain, same in (((1.0, 1.0), True), ((0.6, 0.9), False)):
            cfg = fl_cfg(2, delay=140, gain=gain, sigma=40.0, axis=0.7, thr=-1000)
            out, pairs, iq_d, iq_l = synth_cores([ro_program(r) for r in reads], cfg, [0x1234567, 0x7654321],
                                                 [0x1234560, 0x7654300], spc, spc, env, 4100, n_shots=3, shot0=77)
            n = len(pairs['lane'])
            want = demod_iq_ref.demod_iq(cfg, pairs, out['summary'], out['events'], iq_d, iq_l, cfg.meas_cap)
            _, acc, res = run_ref(cfg, pairs, [[i] for i in range(n)], out, iq_d, iq_l)
            assert (res[:, 0] == 3).all() and np.abs(want[0][:3].astype(np.int64)).max() > 10 ** 6
            np.testing.assert_array_equal(res[:, 0], want[1][:, 0])
            assert np.array_equal(acc, want[0]) == same, (spc, gain)
            if same:
                np.testing.assert_array_equal(res, want[1])


def tone_case(det, L, seed):
    """two cores at 1:1 with square envelopes, the same timing and thetas:
    (acc_0 with both on the line, acc_0 alone, acc_1 alone), first readout"""
    rng = np.random.RandomState(seed)
    f0 = int(rng.randint(0, 2 ** 31))
    f = [f0, (f0 + det) & 0xFFFFFFFF]
    reads = [[dict(A=int(rng.randint(12000, 30000)), ph_d=int(rng.randint(0, 1 << 17)),
                   ph_lo=int(rng.randint(0, 1 << 17)), L_d=L + 1, L_lo=L, lo_at=3)] for _ in range(2)]
    cfg = fl_cfg(2, delay=0, theta=(1.1, 1.1))
    out, pairs, iq_d, iq_l = synth_cores([ro_program(r) for r in reads], cfg, f, f, (1, 1), (1, 1),
                                         np.full(4 * (L + 2), SQUARE, np.uint32), 4 * L + 40)
    adc, both, _ = run_ref(cfg, pairs, [[0, 1]], out, iq_d, iq_l)
    assert max(np.abs(v).max() for v in iq16(adc)) < 32767           # nothing clips
    _, alone, _ = run_ref(cfg, pairs, [[0], [1]], out, iq_d, iq_l)
    return both[0, 0].astype(np.int64), alone[0, 0].astype(np.int64), alone[0, 1].astype(np.int64)


def test_tone_orthogonality():
    """the neighbour's leakage L = acc_0(both) - acc_0(alone) over a window of N
    clocks at detuning D: zero when D N is a whole number of turns, and
    |acc_1| |sin(pi d N) / (N sin(pi d))|, d = D / 2^32, when it is half a turn
    off -- both within flat_tolerance(acc_1 at its own LO)"""
    worst = 0.0
    for L in (64, 256):
        N = 4 * L
        for turns in (1, 3, -2, 37):                     # D N = turns 2^32
            det = (turns * 2 ** 32 // N) & 0xFFFFFFFF
            assert (det * N) % 2 ** 32 == 0
            both, alone, other = tone_case(det, L, 100 + turns)
            tol = flat_tolerance(other)
            dev = float(np.abs(both - alone).max())
            worst = max(worst, dev / tol)
            print('L {} turns {}: leakage {} tolerance {:.1f}'.format(L, turns, both - alone, tol))
            assert np.hypot(*other.astype(float)) > 1e6 and dev <= tol, (L, turns, both, alone, other)
        for half in (1, 5, -3):                          # D N = half 2^31, half odd
            det = (half * 2 ** 31 // N) & 0xFFFFFFFF
            assert (det * N) % 2 ** 32 == 2 ** 31
            both, alone, other = tone_case(det, L, 200 + half)
            d = half / (2.0 * N)
            mag = float(np.hypot(*other.astype(float)))
            want = mag * abs(math.sin(math.pi * d * N) / (N * math.sin(math.pi * d)))
            got = float(np.hypot(*(both - alone).astype(float)))
            tol = flat_tolerance(other)
            worst = max(worst, abs(got - want) / tol)
            print('L {} half turns {}: |leakage| {:.1f} expected {:.1f} tolerance {:.1f}'.format(L, half, got, want, tol))
            assert want > 5 * tol and abs(got - want) <= tol, (L, half, got, want, tol)
    print('worst deviation / tolerance {:.3f}'.format(worst))


def test_clipping():
    """three in-phase, full-amplitude members: the summed return is three times
    the converter's range, and the ADC pins at +-32767 -- symmetric, never -32768"""
    read = [dict(A=65535, ph_d=0, ph_lo=0, L_d=64, L_lo=60, lo_at=4)]
    cfg = fl_cfg(4, delay=0, theta=(0.0, 0.0), p1=[0.5] * 4)
    f = [0x0A000000] * 4
    out, pairs, iq_d, iq_l = synth_cores([ro_program(read)] * 3 + [[isa.done_cmd()]], cfg, f, f, (4, 4), (4, 4),
                                         np.full(300, SQUARE, np.uint32), 300)
    adc, acc, _ = run_ref(cfg, pairs, [[0, 1, 2], [3]], out, iq_d, iq_l)
    one = feedline_ref.feedline_adc(cfg, pairs, [[0]], out['summary'], out['events'], iq_d, iq_l.shape[1], 4)
    i3, q3 = iq16(adc[0])
    i1, q1 = iq16(one[0])
    for v3, v1 in ((i3, i1), (q3, q1)):
        np.testing.assert_array_equal(v3, np.clip(3 * v1, -32767, 32767))
        assert v3.max() == 32767 and v3.min() == -32767
        assert (np.abs(3 * v1) > 32767).sum() > 100 and (np.abs(v1) > 0).any()
    assert not adc[1].any()                              # the idle core's own line is silent
    # the demodulator sees the clipped stream: less than three times one member's accumulator
    _, acc1, _ = run_ref(cfg, pairs, [[0], [1], [2], [3]], out, iq_d, iq_l)
    m3, m1 = np.hypot(*acc[0, 0].astype(float)), np.hypot(*acc1[0, 0].astype(float))
    assert m1 > 1e5 and 1.0 * m1 < m3 < 2.0 * m1, (m1, m3)


MEAS_CAP = 3


def switching_case(no_strobe):
    """four cores: core 0 reads at 200, 700, 1200; core 1 at 450, 950
    (staggered: from 700 core 0 is on draw 1 while core 1 is on draw 0 until
    950) -- or, with no_strobe, drives there but never reads; core 2 has LO
    pulses but no drive; core 3 reads 5 times, two more than MEAS_CAP keeps"""
    def prog(times, c, drive=True, lo=True):
        words = [isa.pulse_reset()]
        for k, t in enumerate(times):
            if drive:
                words.append(isa.pulse_cmd(freq_word=0, phase_word=7777 * k + c, amp_word=9000 + 1000 * c,
                                           env_word=100 << 12, cfg_word=RDRV, cmd_time=t))
            if lo:
                words.append(isa.pulse_cmd(freq_word=0, phase_word=333 * k, amp_word=0xFFFF, env_word=20 << 12,
                                           cfg_word=RDLO, cmd_time=t + 4))
        return words + [isa.done_cmd()]
    return [prog((200, 700, 1200), 0), prog((450, 950), 1, lo=not no_strobe), prog((300, 800), 2, drive=False),
            prog((100, 350, 600, 850, 1100), 3)]


def test_state_switching():
    """the return of member p at clock n carries the state of draw m_p(n): a
    single-member line equals, between its kept readout strobes, the ADC of the
    same run with every state forced to that draw's; a line of several members
    (no clipping) is the sum of its members' own lines -- with members whose
    readouts are staggered, one without a drive pulse, one without a readout
    strobe and one with more readouts than meas_cap"""
    env = np.full(500, SQUARE, np.uint32)
    f_d, f_lo = [0x03000000, 0x05100000, 0x07200000, 0x09300000], [0x03000100, 0x05100100, 0x07200100, 0x09300100]
    for variant in ('staggered', 'no_strobe'):
        ps = switching_case(variant == 'no_strobe')
        cfgs = {k: fl_cfg(4, delay=5, theta=(0.4, 2.9), gain=(0.5, 0.9), p1=p1, meas_cap=MEAS_CAP, seed=0xFEED)
                for k, p1 in (('mixed', 0.5), (0, 0.0), (1, 1.0))}
        runs = {k: synth_cores(ps, c, f_d, f_lo, (4, 4), (4, 4), env, 1500, n_shots=2, shot0=31)
                for k, c in cfgs.items()}
        out, pairs, iq_d, iq_l = runs['mixed']
        for k in (0, 1):                                 # the waveforms do not depend on the states
            np.testing.assert_array_equal(runs[k][2], iq_d)
            np.testing.assert_array_equal(runs[k][0]['events'], out['events'])
        cfg, n = cfgs['mixed'], len(pairs['lane'])
        singles = [[i] for i in range(n)]
        n_lo = iq_l.shape[1]
        adc1 = feedline_ref.feedline_adc(cfg, pairs, singles, out['summary'], out['events'], iq_d, n_lo, MEAS_CAP)
        forced = {k: feedline_ref.feedline_adc(cfgs[k], pairs, singles, out['summary'], out['events'], iq_d, n_lo,
                                               MEAS_CAP) for k in (0, 1)}
        seen_states, differ, dropped = set(), 0, 0
        for i in range(n):
            lane, core, shot = int(pairs['lane'][i]), int(pairs['core'][i]), int(pairs['shot'][i])
            ev = out['events'][:int(out['summary'][lane, 2]), lane]
            strobes = [int(e[0]) for e in ev if e[1] >> 28 == 0 and (e[1] >> 24) & 3 == RDLO]
            kept = strobes[:MEAS_CAP]
            edges = [0] + kept[1:] + [1500]              # draw 0 holds from clock 0 until the second kept strobe
            for m in range(max(len(kept), 1)):
                st = feedline_ref.state(cfg, shot, core, m)
                seen_states.add((core, m, st))
                a, b = 4 * edges[m], 4 * edges[m + 1]
                np.testing.assert_array_equal(adc1[i, a:b], forced[st][i, a:b])
                differ += int((forced[0][i, a:b] != forced[1][i, a:b]).sum())
            if core == 2:
                assert not adc1[i].any() and len(kept) == 2
            if core == 3:                                # two strobes beyond meas_cap change nothing
                assert len(strobes) == 5 and len(kept) == MEAS_CAP
                dropped += feedline_ref.state(cfg, shot, 3, MEAS_CAP) != feedline_ref.state(cfg, shot, 3, MEAS_CAP - 1)
            if core == 1:
                assert len(strobes) == (0 if variant == 'no_strobe' else 2) and adc1[i].any()
        assert differ > 1000                             # the two states' traces do differ where compared
        assert len({st for _, _, st in seen_states}) == 2
        assert dropped                                   # a dropped strobe's draw would have switched the state
        # at clocks 700..950 core 0 is on draw 1 while core 1 is still on draw 0: the draws are per member
        line_all = [[s_ * 4 + c for c in range(4)] for s_ in range(2)]
        adc4, acc, res = run_ref(cfg, pairs, line_all, out, iq_d, iq_l, MEAS_CAP)
        for l, line in enumerate(line_all):
            si = sum(iq16(adc1[i])[0] for i in line)
            sq = sum(iq16(adc1[i])[1] for i in line)
            assert max(np.abs(si).max(), np.abs(sq).max()) < 32767
            np.testing.assert_array_equal(iq16(adc4[l])[0], si)
            np.testing.assert_array_equal(iq16(adc4[l])[1], sq)
        want_counts = [3, 0 if variant == 'no_strobe' else 2, 2, 3] * 2
        assert res[:, 0].tolist() == want_counts
        assert acc[:, 2].any() and acc[:, 3].any()       # the silent member still hears its neighbours


def test_feedline_table():
    """FeedlineTable without a device: the default lines (one per shot, all of
    its pairs) and every refusal of the C side"""
    from distributed_processor_amd import FeedlineTable

    class PT:                                            # the columns FeedlineTable reads of a DemodPairTable
        def __init__(self, shots, spc_drv=None, spc_lo=None):
            self.n_pairs = len(shots)
            self.cols = dict(shot=np.array(shots, np.uint64),
                             spc_drv=np.array(spc_drv or [16] * len(shots), np.uint32),
                             spc_lo=np.array(spc_lo or [4] * len(shots), np.uint32))
    pt = PT([9, 9, 7, 9, 7, 8])
    ft = FeedlineTable(pt)
    assert ft.lines == [[0, 1, 3], [2, 4], [5]] and ft.n_lines == 3
    assert ft.line_first.tolist() == [0, 3, 5, 6] and ft.member.tolist() == [0, 1, 3, 2, 4, 5]
    assert ft.line_of.tolist() == [0, 0, 1, 0, 1, 2]
    st = ft.struct()
    assert st.n_lines == 3 and st.line_first == ft.line_first.ctypes.data and st.member == ft.member.ctypes.data
    assert ft.line_first.dtype == np.uint32 and ft.member.dtype == np.uint32
    part = FeedlineTable(pt, [[5, 0]])
    assert part.line_of.tolist() == [0, -1, -1, -1, -1, 0]
    assert FeedlineTable(PT(list(range(16)) * 1), [list(range(16))]).n_lines == 1
    for bad, word in (([], 'at least one line'), ([[0], []], 'members'), ([list(range(17))], 'members'),
                      ([[0, 6]], 'outside'), ([[0, -1]], 'outside'), ([[0, 1], [2, 1]], 'two lines'),
                      ([[0, 0]], 'two lines')):
        with pytest.raises(DpemuError, match=word):
            FeedlineTable(PT(list(range(17))) if len(bad) == 1 and len(bad[0]) == 17 else pt, bad)
    with pytest.raises(DpemuError, match='spc_drv'):
        FeedlineTable(PT([1, 1], spc_drv=[16, 8]))
    with pytest.raises(DpemuError, match='spc_lo'):
        FeedlineTable(PT([1, 1], spc_lo=[4, 2]))
    FeedlineTable(PT([1, 2], spc_lo=[4, 2]))             # different lines may differ
