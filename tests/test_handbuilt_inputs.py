"""The hand-built input sets of tests/handbuilt.py on the CPU: only the
references run here (tests/demod_iq_ref.py, tests/feedline_ref.py,
tests/resonator_ref.py, oracle.dds), and every condition that keeps
tests/test_gpu_readout_direct.py and test_gpu_dds.test_saturating_tables from
being vacuous is asserted from their outputs and from the references' own
formulas -- that a set reaches the chunk, the slot, the clamp or the wrap it
was built for is a property of the inputs, checked without a kernel."""

import numpy as np
import pytest

import oracle
from tests import handbuilt as hb
from tests import feedline_ref, resonator_ref
from tests.demod_iq_ref import noise, s16
from tests.test_demod import RDLO

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def strobes(c, lane):
    """the event indices of the lane's readout strobes, in the whole array and among the counted records"""
    w = c.events[:, lane, 1]
    at = np.flatnonzero((w >> 28 == 0) & ((w >> 24) & 3 == RDLO))
    return at, at[at < min(int(c.summary[lane, 2]), c.cfg.event_cap)]


def unclamped_returns(c):
    """per pair: ((d (x) (c, s_) + 2^14) >> 15 before symsat, I and Q) and the gain, at every LO sample, from
    the reference's own inputs (resonator_ref.member_inputs) and formulas (feedline_ref.feedline_adc)"""
    lut = oracle.dds_sin_lut().astype(np.int64)
    out = []
    for p in range(c.pt.n_pairs):
        d_i, d_q, st = resonator_ref.member_inputs(c.cfg, c.pt.cols, p, c.summary, c.events, c.iq_drv, c.n_lo,
                                                   c.cfg.meas_cap, c.cfg.event_cap)
        ti = np.array([((c.cfg.ro_theta[s] + (1 << 19)) >> 20) & 4095 for s in (0, 1)])[st]
        cs, sn = lut[(ti + 1024) & 4095], lut[ti]
        gain = np.array([c.cfg.ro_gain[0], c.cfg.ro_gain[1]], np.int64)[st]
        out.append(((d_i * cs - d_q * sn + (1 << 14)) >> 15, (d_i * sn + d_q * cs + (1 << 14)) >> 15, gain, st))
    return out


def window_sums(c, pair, m, a_i, a_q):
    """T of readout m of the pair for the mixed stream (a_I, a_Q): the references' S and scale lines"""
    j0, j1 = c.windows(pair)[m]
    lo = c.iq_lo[int(c.pt.cols['lo_row'][pair])][j0:j1]
    lo_i, lo_q = s16(lo), s16(lo >> 16)
    a_i, a_q = a_i[j0:j1], a_q[j0:j1]
    h = 15 + int(c.pt.cols['spc_lo'][pair]).bit_length() - 1
    S = (int((a_i * lo_i + a_q * lo_q).sum()), int((a_q * lo_i - a_i * lo_q).sum()))
    return [(S_c + (1 << (h - 1))) >> h for S_c in S]


def test_event_builder_fills_every_slot_with_what_must_not_count():
    for name in hb.CASES:
        c = hb.case(name)
        for lane in range(c.summary.shape[0]):
            t, w = c.events[:, lane, 0].astype(np.int64), c.events[:, lane, 1]
            assert (np.diff(t) >= 0).all()
            kind, elem = w >> 28, (w >> 24) & 3
            fill = [((kind == 0) & (elem != RDLO)).sum(), ((kind == 1) & (elem == RDLO)).sum(), (kind >= 2).sum()]
            assert min(fill) >= 1 and sum(fill) + len(strobes(c, lane)[0]) == c.cfg.event_cap
        assert (c.summary[:, [0, 1, 3, 4, 5, 6, 7]] != 0).any()


@pytest.mark.parametrize('name', ['scan_16_4', 'scan_1_1'])
def test_scan_case_reaches_every_chunk_and_slot(name):
    c, ref = hb.case(name), hb.reference(name)
    cfg = c.cfg
    assert (cfg.event_cap, cfg.meas_cap, c.summary.shape[0], c.pt.n_pairs) == (1024, 32, 8, 8)
    assert c.n_lo % 4 == 0 and c.n_lo % 64 != 0
    assert c.pt.cols['lane'].tolist() == list(range(8)) and sorted(len(ln) for ln in c.lines) == [1, 3, 4]
    a, b, cc, d, e, f, g, h = (strobes(c, lane) for lane in range(8))
    # (a) 40 readouts, one at least in each of the 16 chunks of 64 records; 32 kept from >= 12 chunks
    assert len(a[1]) == 40 and set(a[1] // 64) == set(range(16)) and {63, 64, 255, 256, 1023} <= set(a[1].tolist())
    assert len(set(a[1][:32] // 64)) >= 12 and a[1][31] // 64 == 13
    # (b) a count above event_cap, readouts in the last chunk; (c) 32, all at 992..1023
    assert c.summary[1, 2] == 1030 > cfg.event_cap and (b[1] >= 960).sum() >= 3
    assert cc[1].tolist() == list(range(992, 1024))
    assert len(d[0]) == 0 and e[1].tolist() == [1023]
    # (f) stale strobes behind the count
    assert c.summary[5, 2] == 700 and len(f[1]) == 3 and f[1].max() == 699 and (f[0] >= 700).sum() == 3
    # (g) two readouts at one clock; the first one's window holds the third one's strobe
    tg = [(int(c.events[i, 6, 0]), int(c.events[i, 6, 1] >> 12) & 0xFFF) for i in g[1]]
    assert tg[0][0] == tg[1][0] and tg[0][0] < tg[2][0] < tg[0][0] + tg[0][1] * cfg.ro_cpw
    assert len(h[1]) == 33
    # windows of 1..3 words, all inside the LO rows
    for p in range(8):
        assert all(0 < j1 - j0 <= 3 * cfg.ro_cpw * int(c.pt.cols['spc_lo'][p]) and j1 < c.n_lo for j0, j1 in c.windows(p))
    # the references keep what was planned
    for res in (ref['res_iq'], ref['fl'][1], ref['fl_res'][1]):
        assert res[:, 0].tolist() == hb.SCAN_COUNTS == [32, 6, 32, 0, 1, 3, 4, 32]
    for res in (ref['res_iq'], ref['fl'][1]):
        top = [int(res[p, 1]) >> 31 for p in (0, 2, 7)]
        assert 1 in top and 0 in top, top
    # thresholds 0, 0xFFFFFFFF and two mid values; the kept states differ along the lanes of the mid values
    assert sorted(cfg.p1_threshold[k] for k in range(4))[::3] == [0, 0xFFFFFFFF]
    states = {p: [feedline_ref.state(cfg, int(c.pt.cols['shot'][p]), int(c.pt.cols['core'][p]), q)
                  for q in range(max(len(c.reads(p)), 1))] for p in range(8)}
    assert all(len(set(states[p])) == 2 for p in (0, 1)) and set(states[2]) == {0} and set(states[7]) == {1}
    # the resonator reference's state sequence of lane (a), sample by sample
    st = resonator_ref.member_inputs(cfg, c.pt.cols, 0, c.summary, c.events, c.iq_drv, c.n_lo, 32, 1024)[2]
    assert (np.diff(st) != 0).sum() >= 10
    assert ref['y_peak'] < 2 ** 28


def test_full_range_thetas_cover_the_octants():
    used = set()
    for which in hb.FULL_RANGE:
        cfg = hb.case('full_range_' + which).cfg
        assert cfg.ro_theta[0] in hb.OCTANTS and cfg.ro_theta[1] in hb.OCTANTS
        used |= {hb.OCTANTS.index(cfg.ro_theta[0]), hb.OCTANTS.index(cfg.ro_theta[1])}
    assert used == set(range(8))
    g = hb.case('full_range_gains').cfg.ro_gain
    assert 0 < g[0] < 65536 and 0 < g[1] < 65536 and g[0] != g[1]


@pytest.mark.parametrize('which', list(hb.FULL_RANGE))
def test_full_range_case_saturates(which):
    c, ref = hb.case('full_range_' + which), hb.reference('full_range_' + which)
    cfg = c.cfg
    assert (cfg.event_cap, cfg.meas_cap) == (16, 4) and cfg.ro_sigma != 0
    for rows in (c.iq_drv, c.iq_lo, c.adc_in):
        assert all((rows == w).all(axis=1).any() for w in hb.CORNERS)
    assert sorted(c.pt.cols['drv_row'].tolist()) == sorted(c.pt.cols['lo_row'].tolist()) == list(range(12))
    ret = unclamped_returns(c)
    both = np.concatenate([np.concatenate([r_i, r_q]) for r_i, r_q, _, _ in ret])
    assert (both > 32767).mean() >= 0.01 and (both < -32767).mean() >= 0.01
    used = np.concatenate([st for _, _, _, st in ret])                         # both thetas are used
    assert 0.25 < used.mean() < 0.75 and sum(len(set(st.tolist())) == 2 for _, _, _, st in ret) >= 6
    # the feedline sums clip at both ends (there is no noise in this stage)
    clipped = [0, 0]
    for line in c.lines:
        for q in (0, 1):
            tot = sum((np.clip(ret[p][q], -32767, 32767) * ret[p][2] + (1 << 15)) >> 16 for p in line)
            clipped[0] += int((tot > 32767).sum())
            clipped[1] += int((tot < -32767).sum())
    assert min(clipped) >= 10
    halves = np.concatenate([s16(ref['adc']).ravel(), s16(ref['adc'] >> 16).ravel()])
    assert (halves == 32767).sum() >= 10 and (halves == -32767).sum() >= 10 and halves.min() == -32767
    # a window of 4,096 words that n_samples_lo clips, in every lane
    for p in range(12):
        t, pe = c.reads(p)[3]
        assert (pe >> 12) & 0xFFF == 0 and t * 4 < c.n_lo < (t + 4096 * cfg.ro_cpw) * 4 and c.windows(p)[3][1] == c.n_lo
    # the caller-made trace under the windows: I = -32768, and 0x80008000 under an LO word 0x80008000
    n_min = n_both = 0
    for p in range(12):
        a, lo = c.adc_in[c.ft.line_of[p]], c.iq_lo[int(c.pt.cols['lo_row'][p])]
        for j0, j1 in c.windows(p):
            n_min += int((a[j0:j1] & 0xFFFF == 0x8000).sum())
            n_both += int(((a[j0:j1] == 0x80008000) & (lo[j0:j1] == 0x80008000)).sum())
    assert n_min >= 100 and n_both >= 1
    # ... and they matter: reading I = -32768 as a 16-bit negation would (+32768 -> -32768) changes the result
    i = 3
    a = c.adc_in[c.ft.line_of[i]]
    T = window_sums(c, i, 0, s16(a), s16(a >> 16))
    T_neg16 = window_sums(c, i, 0, np.where(s16(a) == -32768, 32768, s16(a)), s16(a >> 16))
    assert T[1] != T_neg16[1]
    assert ref['y_peak'] < 2 ** 28


def test_clamp_case_reaches_the_clamp_where_one_can_be_reached():
    """The largest admissible ro_cpw (8) under a 4,096-word window at one LO sample per clock is 32,768 samples,
    and h = 15: T is the per-sample product at constant rows.
      * dpemu_demod_feedline reads any int16 pair: P_I = 2^31 at four halves of -32768, so T = 2^31 > INT32_MAX
        and sig clamps at INT32_MAX.  The most negative products are P_I = -2 * 32768 * 32767 and P_Q =
        -(2^30 + 32768 * 32767) = -(2^31 - 32768): T stays 32,768 above INT32_MIN.  No admissible input
        reaches the lower clamp, so none is asserted.
      * dpemu_demod_iq mixes a return that symsat holds to +-32767 and ro_gain <= 65536: |T| <= 2 * 32767 *
        32768 = 2^31 - 65536, 65,535 short of INT32_MAX.  Neither clamp can be reached; the noise still wraps
        acc from there."""
    c, ref = hb.case('clamp'), hb.reference('clamp')
    cfg = c.cfg
    from distributed_processor_amd import _abi
    assert cfg.ro_cpw == _abi.RO_CPW_MAX == 8 and c.windows(0)[0] == (4, 4 + 32768) and c.windows(0)[1] == (c.n_lo, c.n_lo)
    T_fl, T_iq = [], []
    ret = unclamped_returns(c)
    for p in range(4):
        a = c.adc_in[c.ft.line_of[p]]
        T_fl.append(window_sums(c, p, 0, s16(a), s16(a >> 16)))
        T_iq.append(window_sums(c, p, 0, np.clip(ret[p][0], -32767, 32767), np.clip(ret[p][1], -32767, 32767)))
    assert max(max(T) for T in T_fl) == 2 ** 31 == INT32_MAX + 1                # clamped by one
    assert min(min(T) for T in T_fl) == -(2 ** 31 - 32768) == INT32_MIN + 32768   # the margin of the lower clamp
    assert max(max(T) for T in T_iq) == 2 ** 31 - 65536 == INT32_MAX - 65535      # the margin of demod_iq's
    assert min(min(T) for T in T_iq) > INT32_MIN
    # the noise wraps acc in both stages (T_iq's gain is 65536: sig = T)
    assert (cfg.ro_gain[0], cfg.ro_gain[1]) == (65536, 65536)
    for T_all, acc in ((T_fl, ref['fl_in'][0]), (T_iq, ref['acc_iq'])):
        wraps = 0
        for p in range(4):
            _, zi, zq = noise(cfg.seed, int(c.pt.cols['shot'][p]), int(c.pt.cols['core'][p]), 0, cfg.ro_sigma)
            for q, z in enumerate((zi, zq)):
                v = max(INT32_MIN, min(INT32_MAX, T_all[p][q])) + z
                wraps += not INT32_MIN <= v <= INT32_MAX
                assert int(acc[0, p, q]) == ((v + 2 ** 31) & 0xFFFFFFFF) - 2 ** 31
        assert wraps >= 1


def test_edge_cases_sit_on_the_edges():
    c, ref = hb.case('edge_four_samples'), hb.reference('edge_four_samples')
    assert c.n_lo == 4 and c.windows(0) == [(0, 4), (3, 4), (4, 4), (4, 4)] and c.windows(1) == [(3, 4)]
    assert c.cfg.ro_delay == 0 and ref['adc'].all() and ref['acc_iq'][1, 0].any()
    assert ref['res_iq'][:, 0].tolist() == [4, 1, 2]

    c, ref = hb.case('edge_delay_past_every_clock'), hb.reference('edge_delay_past_every_clock')
    assert c.cfg.ro_delay > c.n_lo and not ref['adc'].any() and c.iq_drv.all() and ref['y_peak'] == 0
    assert ref['adc_res'].any()                                     # the converter's noise alone

    c, ref = hb.case('edge_short_drive'), hb.reference('edge_short_drive')
    cut = 4 * 50 + 2
    assert c.iq_drv.shape[1] == hb.EDGE_CUT == (cut // 4) * 16 + (cut % 4) * 4 < 16 * (c.n_lo // 4)
    assert ref['adc'][:, :cut].all() and not ref['adc'][:, cut:].any()
    assert all(any(j0 < cut < j1 for j0, j1 in c.windows(p)) for p in range(3)) and cut % 64 and cut % 4
    for name in ('edge_' + w for w in hb.EDGES):                    # the rows are permutations, none the identity
        cols = hb.case(name).pt.cols
        for f in ('drv_row', 'lo_row'):
            assert sorted(cols[f].tolist()) == [0, 1, 2] and cols[f].tolist() != [0, 1, 2]


@pytest.mark.parametrize('name', list(hb.SATURATING_CASES))
def test_saturating_tables_saturate(name):
    desc, summary, ev, env_tab, freq_tab, n_lanes, cap, n_samples = hb.saturating_case(name)
    # Q (the low half) is never -32768 in an env word or a rotation word: the Y-form sweeps stay eligible
    rot_words = freq_tab[3:][np.arange(len(freq_tab) - 3) % 16 != 0]
    assert (env_tab & 0xFFFF != 0x8000).all() and (rot_words & 0xFFFF != 0x8000).all()
    assert (env_tab >> 16 == 0x8000).any() and (rot_words >> 16 == 0x8000).any()
    assert {0, 1, 65535} <= set(ev[:, :, 3].ravel().tolist())
    ref = oracle.dds(desc, summary, ev, env_tab, freq_tab, n_samples, cap)
    chans = hb.dds_restated(desc, summary, ev, env_tab, freq_tab, n_samples, cap)
    np.testing.assert_array_equal(np.stack([ch['out'] for ch in chans]), np.asarray(ref).view(np.uint32))
    played = np.concatenate([ch['played'] for ch in chans])
    n = int(played.sum())
    assert n > 10000
    rot_i, rot_q = (np.concatenate([ch['rot'][q] for ch in chans]) for q in (0, 1))
    assert ((rot_i > 32767) | (rot_q > 32767)).sum() >= 0.01 * n
    assert ((rot_i < -32767) | (rot_q < -32767)).sum() >= 0.01 * n
    out = np.concatenate([ch['out'] for ch in chans])[played]
    o_i, o_q = s16(out), s16(out >> 16)
    assert ((o_i == 32767) | (o_q == 32767)).sum() >= 0.01 * n and ((o_i == -32768) | (o_q == -32768)).sum() >= 0.01 * n
    env = np.concatenate([ch['env'] for ch in chans])[played]
    assert (env >> 16 == 0x8000).any()
    rot_on = np.concatenate([ch['rot_on'] for ch in chans])
    assert (np.concatenate([ch['rotw'] for ch in chans])[rot_on] >> 16 == 0x8000).any()


# ---- many pairs at 32 slots -----------------------------------------------------------------------------------

def traces_of(c, adc, n_bins, bin_clocks, keep, by_slot=False):
    """the reference traces of the pairs ``keep`` alone, each still on its line's row of ``adc``"""
    from tests import traces_ref
    keep = list(keep)
    at = {p: i for i, p in enumerate(keep)}
    cols = {f: v[keep] for f, v in c.pt.cols.items()}
    lines = [[at[p] for p in ln if p in at] for ln in c.lines]
    return traces_ref.feedline_traces(c.cfg, cols, lines, c.summary, c.events, adc, c.iq_lo, c.cfg.meas_cap, n_bins,
                                      bin_clocks, by_slot=by_slot)


@pytest.mark.fresh_process        # builds and runs tests/trace_plan_test.cpp (tests/test_trace_plan.py)
@pytest.mark.parametrize('name', list(hb.MANY))
def test_many_pairs_case_crosses_a_staging_run(name):
    from collections import Counter
    from tests import test_traces as T
    from tests.test_trace_plan import case_plan
    c, ref = hb.case(name), hb.reference(name)
    cfg, cols = c.cfg, c.pt.cols
    spc_l, mc = int(cols['spc_lo'][0]), cfg.meas_cap
    assert (mc, spc_l) == {'many_pairs_16_4': (32, 4), 'many_pairs_1_1': (32, 1), 'many_pairs_16_4_cap17': (17, 4),
                           'many_pairs_1_1_cap17': (17, 1)}[name]
    assert cfg.cores_per_shot == 4 and cfg.ro_cpw == 4 and (cols['spc_lo'] == spc_l).all()
    # the groups, the shuffled table
    sizes = sorted(Counter(cols['core'].tolist()).values())
    assert sizes == [5, 32, 33, 72] and sizes[-1] >= 70
    assert cols['core'].tolist() != sorted(cols['core'].tolist())
    assert sorted(cols['lane'].tolist()) == list(range(c.pt.n_pairs)) != cols['lane'].tolist()
    assert len(set(zip(cols['shot'].tolist(), cols['core'].tolist()))) == c.pt.n_pairs
    assert set(len(ln) for ln in c.lines) >= {1, 16} and max(len(ln) for ln in c.lines) == 16
    assert max(cols['drv_row'].max(), cols['lo_row'].max()) < 8 < c.pt.n_pairs         # shared rows
    # the strobes: 0, 1, 2, 31, 32 and 40 of them, in an event_cap they and the filler fill
    n_str = [len(strobes(c, int(cols['lane'][p]))[1]) for p in range(c.pt.n_pairs)]
    assert set(n_str) == set(hb.MANY_COUNTS) == {0, 1, 2, 31, 32, 40} and cfg.event_cap == 40 + 3
    kept = ref['fl'][1][:, 0].tolist()
    assert kept == [min(k, mc) for k in n_str] == [len(c.reads(p)) for p in range(c.pt.n_pairs)]
    assert kept.count(mc) >= 20 and kept.count(0) >= 10 and (mc != 32 or 31 in kept)
    # windows of 1..3 words; some clipped by the rows; at 1:1 starts that are no multiple of 4
    words, clipped, unaligned = set(), 0, 0
    for p in range(c.pt.n_pairs):
        for (t, pe), (j0, j1) in zip(c.reads(p), c.windows(p)):
            L = (pe >> 12) & 0xFFF
            words.add(L)
            clipped += j0 < j1 == c.n_lo < (t + L * cfg.ro_cpw) * spc_l
            unaligned += j0 % 4 != 0 and j0 < j1
    assert words == {1, 2, 3} and clipped >= 3 and (spc_l != 1 or unaligned >= 100)
    # a workgroup's staging run and the smallest chunk of the big group
    pl = case_plan(name)
    run = min(pl['TRACE_ITEMS'] // mc, pl['BLOCK'])
    assert run == {32: 32, 17: 60}[mc] and c.pt.n_pairs % run != 0
    big = [ch for ch in pl['chunks'] if ch[0] == 2]
    first, end = big[0][2], big[0][3]
    assert end - first == pl['TRACE_PAIRS_PER_WG'] == 64 > run
    second = pl['perm'][first + run:end]                 # staged in the second run
    assert second and all(cols['core'][p] == 2 for p in second)
    _, adc, n_bins, bin_clocks = T.hb_trace_inputs(name)
    both = 0
    for p in second:
        alone = traces_of(c, adc, n_bins, bin_clocks, [p])
        both += all(alone[0, 2, st, :, 2].any() and alone[0, 2, st, :, 3].any() for st in (0, 1))
    assert both >= 1
    full = T.hb_trace_reference(name, False)
    rest = traces_of(c, adc, n_bins, bin_clocks, [p for p in range(c.pt.n_pairs) if p not in second])
    assert all((full[0, 2, st] != rest[0, 2, st]).any() for st in (0, 1))
    assert np.array_equal(full[0, [0, 1, 3]], rest[0, [0, 1, 3]])
    assert np.array_equal(traces_of(c, adc, n_bins, bin_clocks, range(c.pt.n_pairs)), full)
    # by slot: the last slot takes readouts of both states
    by_slot = T.hb_trace_reference(name, True)
    assert by_slot.shape[0] == mc and all(by_slot[mc - 1, :, st, :, 1].any() for st in (0, 1))


# ---- supplied states ----------------------------------------------------------------------------------------------

# where a state cannot show: no drive sample reaches the trace; both states' return phase and gain are the same
ST_SAME_AS_BASE = {'edge_delay_past_every_clock': ('adc', 'adc_res'), 'clamp': ('adc',)}


def test_supplied_states_plant_every_word():
    planted = set()
    for name in hb.CASES:
        words, plan = hb.states_plan(name)
        n = len(words)
        assert n == hb.case(name).summary.shape[0]
        for w in hb.ST_PLANTED:
            assert all(words[L] == w for L in plan.get(w, []))
        planted |= {w for w in hb.ST_PLANTED if plan.get(w)}
        assert n < 8 or all(plan.get(w) for w in hb.ST_PLANTED)
        assert len(plan['high_only']) >= (3 if n >= 12 else 1)
    assert planted == set(hb.ST_PLANTED) == {0, 0xFFFFFFFF, 0x80000000, 0x55555555}


@pytest.mark.parametrize('name', list(hb.CASES))
def test_supplied_states_are_read_below_the_count_alone(name):
    c = hb.case(name)
    words, plan = hb.states_plan(name)
    read, draws = hb.draws_read(name), hb.packed_draws(name)
    low = hb.low_mask(read)
    for p in range(c.pt.n_pairs):
        assert read[int(c.pt.cols['lane'][p])] == max(len(c.reads(p)), 1)
    # a word whose set bits are all at or above the count, on several lanes
    assert all(words[L] != 0 and words[L] & low[L] == 0 for L in plan['high_only'])
    # on a lane of 32 kept readouts the word is not the draws': bit 31 and a bit from 2 up differ
    if name.startswith(('scan', 'many_pairs')) and c.cfg.meas_cap == 32:
        (L,) = plan['flipped']
        diff = int(words[L]) ^ int(draws[L])
        assert read[L] == 32 and diff >> 31 == 1 and diff & 0x7FFFFFFC
    else:
        assert not plan['flipped'] and read.max() < 32
    st = hb.reference_st(name)
    # the packed draws give the base calls' outputs, the supplied words do not
    from tests import iq_stats_ref, test_traces as T
    ref = hb.reference(name)
    base = {'adc': ref['adc'], 'adc_res': ref['adc_res'], ('traces', False): T.hb_trace_reference(name, False),
            ('traces', True): T.hb_trace_reference(name, True)}
    base['stats'], base['bits'] = iq_stats_ref.iq_stats(c.cfg, ref['fl'][0], ref['fl'][1][:, 0], core=c.pt.cols['core'],
                                                       shot=c.pt.cols['shot'], by_slot=True)
    from_draws = hb.st_outputs(name, draws)
    for key, want in base.items():
        np.testing.assert_array_equal(from_draws[key], want, err_msg=str(key))
        if key == 'bits':                                # (the outcome bits do not depend on the prepared state)
            np.testing.assert_array_equal(st[key], want)
        else:
            assert np.array_equal(st[key], want) == (key in ST_SAME_AS_BASE.get(name, ())), key
    # the bits at or above a lane's count change nothing, cleared or flipped; the words the GPU gets have them set
    assert (words & low != words).sum() >= 2
    for other in (words & low, words ^ ~low):
        out = hb.st_outputs(name, other)
        for key, want in st.items():
            np.testing.assert_array_equal(out[key], want, err_msg=str(key))
