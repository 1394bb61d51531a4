"""CPU tests of the qubit-state stage (dpemu_qsim, include/dpemu.h): the
specification, through its Python-integer restatement tests/qsim_ref.py, and
the Python layer (qsim.GateSet, workloads.rb2q_gateset, survival, fit_decay).

The events are oracle_fast's of config 4 (as tests/test_rb2q.py builds them) or
written by hand.  tests/test_gpu_qsim.py holds the kernel to the same
reference bit for bit."""

import functools

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, qsim, workloads
from tests import qsim_ref

ONE = 1 << 30
FULL = 1 << 60
NEAR_ONE = FULL - (FULL >> 20)            # 2^60 (1 - 2^-20)
QUARTER = workloads.RB_QUARTER


@functools.lru_cache(maxsize=None)
def rb2q_events(n_cores, depth, n_seq, spg=1):
    """(cfg, summary, events) of oracle_fast over n_seq sequences x spg shots of config 4; nothing late or dropped"""
    ps = workloads.config4_rb2q_set(n_seq=n_seq, depth=depth, n_cores=n_cores)
    cfg = _abi.make_config(n_cores, n_groups=n_seq, shots_per_group=spg, max_cycles=1 << 22, event_cap=8 * depth + 16,
                           meas_cap=2)
    f = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, 0, n_seq * spg, want=('summary', 'events'))
    summary = f['summary'].view(np.uint32).reshape(-1, 8)
    s = _abi.unpack_summary(summary)
    assert (s['status'] == _abi.ST_DONE).all() and (s['flags'] == 0).all()
    ev = f['events'].view(np.uint32).reshape(cfg.event_cap, -1, 4)
    for a in (summary, ev):
        a.setflags(write=False)
    return cfg, summary, ev


def qdrv_counts(summary, ev):
    """drive strobes per lane"""
    k = np.arange(ev.shape[0])[:, None] < summary[:, 2][None, :]
    return (k & (ev[:, :, 1] >> 28 == 0) & ((ev[:, :, 1] >> 24) & 3 == workloads.QDRV)).sum(axis=0)


def hand_events(lanes, event_cap=None):
    """summary (n_lanes, 8) and events (event_cap, n_lanes, 4) from per-lane record lists [(t, w1, w2, w3)]"""
    cap = event_cap or max(1, max(len(r) for r in lanes))
    summary, ev = np.zeros((len(lanes), 8), np.uint32), np.zeros((cap, len(lanes), 4), np.uint32)
    for L, recs in enumerate(lanes):
        summary[L, 2] = len(recs)
        for k, r in enumerate(recs[:cap]):
            ev[k, L] = r
    return summary, ev


def strobe(t, freq, env, amp, phase, elem=workloads.QDRV):
    return (t, env | (elem << 24), (phase & 0x1FFFF) | (freq << 17), amp)


# ---- 1. the phase table ----

def test_phase_table():
    lut = qsim_ref.phase_lut()
    assert lut.shape == (768, 2)
    assert [tuple(lut[128 * k]) for k in range(4)] == [(ONE, 0), (0, ONE), (-ONE, 0), (0, -ONE)]
    assert tuple(lut[512]) == (ONE, 0)
    phi = np.arange(1 << 17)
    c, f = lut[phi >> 8], lut[512 + (phi & 255)]
    re = (c[:, 0] * f[:, 0] - c[:, 1] * f[:, 1] + (1 << 29)) >> 30
    im = (c[:, 0] * f[:, 1] + c[:, 1] * f[:, 0] + (1 << 29)) >> 30
    assert np.abs(re * re + im * im - FULL).max() <= 1 << 32
    ang = 2 * np.pi * phi / 2.0 ** 17
    assert np.abs(re - np.cos(ang) * ONE).max() <= 2 and np.abs(im - np.sin(ang) * ONE).max() <= 2
    assert qsim_ref.phase_factor(0x8000) == (0, ONE) and qsim_ref.phase_factor(0) == (ONE, 0)


def test_phase_table_matches_library():
    from distributed_processor_amd._native import load_library
    out = np.zeros((768, 2), np.int32)
    assert load_library().dpemu_qsim_phase_lut(out.ctypes.data) == 0
    np.testing.assert_array_equal(out, qsim_ref.phase_lut())


# ---- 2. ideal config 4 returns to |00> ----

@pytest.mark.parametrize('n_cores,depth', [(2, 40), (4, 15)])
def test_ideal_rb2q_returns_to_ground(n_cores, depth):
    n_seq = 16
    cfg, summary, ev = rb2q_events(n_cores, depth, n_seq)
    gs = workloads.rb2q_gateset(n_cores)
    pops, res = qsim_ref.qsim_gateset(cfg, gs, summary, ev, n_seq)
    cnt = qdrv_counts(summary, ev).reshape(n_cores, n_seq)           # core-major lanes
    per_row = cnt[0::2] + cnt[1::2]                                  # [register, shot]
    assert per_row.min() > 50
    assert (res[:, :, 2] == 0).all() and (res[:, :, 3] == 0).all()
    np.testing.assert_array_equal(res[:, :, 1], per_row)
    # each gate moves a component by a few Q30 LSB: populations are off by < n_gates 2^-25, n_gates <= 1,200
    assert per_row.max() <= 1200
    assert (pops[:, :, 0] >= NEAR_ONE).all() and (res[:, :, 0] == 0).all()


# ---- 3. against a complex128 product ----

def float_states(cfg, gs, summary, ev, n_shots):
    """per (register, shot) the final state of a complex128 product of the gate set's matrices, built from the
    header's formulas: U = Rz(phi) M Rz(-phi) on the acted qubit, the first core the first Kronecker factor"""
    table = {(e['core'], e['freq'], e['env'], e['amp']): e for e in gs.entries}
    out = []
    for c0, c1 in gs.reg_core.tolist():
        for sl in range(n_shots):
            lists = [qsim_ref.drive_strobes(summary, ev, qsim_ref.lane_of(cfg, sl, c, n_shots), cfg.event_cap, gs.drv_elem)
                     for c in (c0, c1)]
            psi = np.array([1, 0, 0, 0], np.complex128)
            for q, (t, k, w1, w2, w3) in qsim_ref.merged(*lists):
                e = table[((c0, c1)[q], w2 >> 17, w1 & 0xFFFFFF, w3 & 0xFFFF)]
                ph = np.exp(2j * np.pi * (w2 & 0x1FFFF) / 2.0 ** 17)
                rz = np.diag([1, ph])                                # Rz(phi) up to a phase that cancels in U
                u0, u1 = (rz @ m @ rz.conj() for m in e['u'])
                if e['kind'] == 1:
                    g = np.kron(np.diag([1, 0]), u0) + np.kron(np.diag([0, 1]), u1)
                else:
                    g = np.kron(u0, np.eye(2)) if q == 0 else np.kron(np.eye(2), u0)
                psi = g @ psi
            out.append(psi)
    return np.array(out)


@pytest.mark.parametrize('n_cores,depth', [(2, 40), (4, 15)])
def test_over_rotation_matches_floats(n_cores, depth):
    n_seq = 16
    cfg, summary, ev = rb2q_events(n_cores, depth, n_seq)
    gs = workloads.rb2q_gateset(n_cores, over_rotation=0.02)
    states = []
    pops, res = qsim_ref.qsim_gateset(cfg, gs, summary, ev, n_seq, states=states)
    got = np.array([[complex(re, im) for re, im in x] for x in states]) / ONE
    want = float_states(cfg, gs, summary, ev, n_seq)
    tol = res[:, :, 1].reshape(-1, 1) * 2.0 ** -24
    assert (np.abs(got.real - want.real) <= tol).all() and (np.abs(got.imag - want.imag) <= tol).all()
    np.testing.assert_allclose(pops.reshape(-1, 4) / FULL, np.abs(want) ** 2, atol=1e-6)
    if depth == 40:
        assert (pops[:, :, 0] < 0.99 * FULL).any()                   # the miscalibration shows


# ---- 4. conventions, by hand ----

HAND_KEYS = dict(x0=(0, 0x040000, 7000), cr=(1, 0x040000, 19660), x1=(0, 0x040000, 9000))   # (freq, env, amp)


def hand_gateset():
    gs = qsim.GateSet(drv_elem=workloads.QDRV)
    gs.add_rotation(0, *HAND_KEYS['x0'], np.pi / 2)
    gs.add_zx(0, 1, *HAND_KEYS['cr'], np.pi / 2)
    gs.add_rotation(1, *HAND_KEYS['x1'], np.pi / 2)
    return gs.registers([(0, 1)])


def test_conventions_by_hand():
    """The native CNOT of clifford2q: ZX90 on the control's drive at immediate phase 0, then X-90 (phase word
    0x10000, a half turn) on the target, the control's S-dagger being virtual.  Control 0: the target is rotated
    by +pi/2 and back, |00> stays.  Control 1 (two X90 first): by -pi/2 and a further -pi/2, |10> -> |11>.  With
    the sign of the ZX term reversed the outcomes would be |01> and |10>.
    One pulse at a quarter-turn phase word (0x8000) on |0>: U = Rz(pi/2) Rx(pi/2) Rz(-pi/2) = Ry(pi/2), so the
    |1> amplitude is +1/sqrt(2), real (-1/sqrt(2) if the phase word turned the axis the other way): a virtual Z of
    a quarter turn before an X90 makes it a Y90."""
    cfg = _abi.make_config(2, event_cap=8)
    gs = hand_gateset()
    x0, cr, x1 = (HAND_KEYS[k] for k in ('x0', 'cr', 'x1'))
    shots = [
        ([strobe(42, *cr, 0)], [strobe(58, *x1, 0x10000)]),                                       # CNOT |00>
        ([strobe(10, *x0, 0), strobe(26, *x0, 0), strobe(42, *cr, 0)], [strobe(58, *x1, 0x10000)]),   # CNOT |10>
        ([strobe(10, *x0, 0x8000)], []),                                                          # Z then X90
        ([strobe(10, *x0, 0), strobe(26, *x0, 0x10000)], []),                                     # X90, X-90
        ([strobe(10, *x0, 0x8000), strobe(26, *x0, 0x8000)], []),                                 # Y90, Y90
        ([strobe(10, *x0, 0), strobe(26, *x0, 0x8000)], []),                                      # X90, Y90
    ]
    n = len(shots)
    lanes = [s[0] for s in shots] + [s[1] for s in shots]           # core-major lanes
    summary, ev = hand_events(lanes)
    states = []
    pops, res = qsim_ref.qsim_gateset(cfg, gs, summary, ev, n, states=states)
    p = pops[0] / FULL
    expected = [(1, 0, 0, 0), (0, 0, 0, 1), (0.5, 0, 0.5, 0), (1, 0, 0, 0), (0, 0, 1, 0), (0.5, 0, 0.5, 0)]
    np.testing.assert_allclose(p, expected, atol=1e-8)
    assert res[0, :, 1].tolist() == [2, 4, 1, 2, 2, 2] and (res[0, :, 2:] == 0).all()
    r = ONE / np.sqrt(2)
    assert abs(states[2][2][0] - r) <= 2 and abs(states[2][2][1]) <= 2 and abs(states[2][0][0] - r) <= 2
    # a sampled outcome is the basis state wherever one population holds everything
    assert res[0, [0, 1, 3, 4], 0].tolist() == [0, 3, 0, 1]


# ---- 5. stochastic Pauli errors ----

ERR_SEQ, ERR_SPG, ERR_DEPTH = 32, 16, 12


@functools.lru_cache(maxsize=1)
def pauli_case():
    cfg, summary, ev = rb2q_events(2, ERR_DEPTH, ERR_SEQ, ERR_SPG)
    gs = workloads.rb2q_gateset(2, err_1q=2.0 ** -7, err_2q=2.0 ** -7)
    pops, res = qsim_ref.qsim_gateset(cfg, gs, summary, ev, ERR_SEQ * ERR_SPG)
    return cfg, summary, ev, gs, pops, res


def test_pauli_errors():
    """32 sequences x 16 shots at depth 12, an error after a pulse with probability 2^-7.  A row plays 71
    pulses on average, so 1 - (1 - 2^-7)^71 = 0.43 of the 512 rows should carry an error: 194 do, and 0.21 of
    those still read |00> (a random non-identity two-qubit Pauli has no X component with probability 3 / 15, a
    one-qubit one with 1 / 3; an early error is scrambled by the Cliffords after it).  Every counted error
    injects a Pauli: the count's modulo-2^16 wrap is far from any row here."""
    cfg, summary, ev, gs, pops, res = pauli_case()
    assert all(e['err_thr'] == 1 << 25 for e in gs.entries)
    pops, res = pops[0], res[0]
    hit = (res[:, 3] & 0xFFFF) >= 1
    assert (res[~hit, 0] == 0).all()
    assert (pops.max(axis=1) >= NEAR_ONE).all()          # a Pauli on a Clifford circuit ends in a basis state
    assert (res[np.arange(len(res)), 0] == np.array([0, 2, 1, 3])[pops.argmax(axis=1)]).all()
    assert hit.sum() >= 150                              # (a condition on the input)
    frac = (res[hit, 0] == 0).mean()
    assert 0.10 <= frac <= 0.45
    surv = qsim.survival(res[None], ERR_SPG)
    assert surv.shape == (1, ERR_SEQ) and abs(surv.mean() - (res[:, 0] == 0).mean()) < 1e-12


def test_pauli_errors_rebatched():
    """the draws are counter-based: a run from another shot_begin, in two halves, reproduces every row"""
    cfg, summary, ev, gs, pops, res = pauli_case()
    n = ERR_SEQ * ERR_SPG
    first = 5 * ERR_SPG                                  # whole groups: the events of shot s are those of its sequence
    for b, e in ((first, n // 2), (n // 2, n)):
        sub = slice(b, e)
        s2 = np.ascontiguousarray(summary.reshape(2, n, 8)[:, sub]).reshape(-1, 8)
        e2 = np.ascontiguousarray(ev.reshape(ev.shape[0], 2, n, 4)[:, :, sub]).reshape(ev.shape[0], -1, 4)
        p2, r2 = qsim_ref.qsim_gateset(cfg, gs, s2, e2, e - b, shot_begin=b)
        np.testing.assert_array_equal(p2[0], pops[0, sub])
        np.testing.assert_array_equal(r2[0], res[0, sub])


# ---- 6. Ramsey fringes from the drive detuning ----

def test_ramsey():
    taus = np.arange(64)
    key = (0, 0x040000, 7000)
    lanes = [[strobe(100, *key, 0), strobe(100 + int(tau), *key, 0)] for tau in taus]
    summary, ev = hand_events(lanes)
    cfg = _abi.make_config(1, event_cap=2)
    gs = qsim.GateSet().add_rotation(0, *key, np.pi / 2).registers([0])
    pops, res = qsim_ref.qsim_gateset(cfg, gs, summary, ev, len(taus))
    assert (pops[0, :, 2] >= NEAR_ONE).all() and (pops[0, :, [1, 3]] == 0).all()      # no detuning: X90 X90 = X
    delta = 5 / 512                                      # turns per clock: every delta t is a whole phase word
    gs.set_detune(0, delta)
    assert gs.detune[0] == 5 << 23
    pops, res = qsim_ref.qsim_gateset(cfg, gs, summary, ev, len(taus))
    p1 = pops[0, :, 2] / FULL
    assert np.abs(p1 - np.cos(np.pi * delta * taus) ** 2).max() <= 2.0 ** -20
    assert p1.min() < 0.01 and (res[0, :, 1] == 2).all()


# ---- 7. the Python layer ----

@pytest.mark.parametrize('n_cores,depth', [(2, 40), (4, 15)])
def test_gateset_keys_are_the_emitted_ones(n_cores, depth):
    cfg, summary, ev = rb2q_events(n_cores, depth, 16)
    gs = workloads.rb2q_gateset(n_cores, over_rotation=0.02, err_2q=0.25)
    seen = set()
    n = summary.shape[0] // n_cores
    for lane in range(summary.shape[0]):
        for t, k, w1, w2, w3 in qsim_ref.drive_strobes(summary, ev, lane, cfg.event_cap, workloads.QDRV):
            seen.add((lane // n, w2 >> 17, w1 & 0xFFFFFF, w3 & 0xFFFF))
    assert seen == gs.keys() and len(seen) == 3 * n_cores // 2
    assert {k[2] for k in seen} == {0x040000}
    assert gs.reg_core.tolist() == [[c, c + 1] for c in range(0, n_cores, 2)]
    cr = [e for e in gs.entries if e['kind'] == 1]
    assert [e['core'] for e in cr] == list(range(0, n_cores, 2)) and all(e['err_thr'] == 1 << 30 for e in cr)
    th = np.pi / 4 * 1.02
    c_, s_ = round(np.cos(th) * ONE), round(np.sin(th) * ONE)
    assert cr[0]['m'].tolist() == [[c_, 0, 0, -s_, 0, -s_, c_, 0], [c_, 0, 0, s_, 0, s_, c_, 0]]   # Rx(theta), Rx(-theta)
    st, keep = gs.struct(cfg, 16, 3)
    assert (st.n_regs, st.n_gates, st.n_lanes, st.event_cap, st.shot_begin, st.n_shots) == (
        n_cores // 2, len(gs.entries), 16 * n_cores, cfg.event_cap, 3, 16)
    assert st.detune is None and [keep[0][1].m[1][k] for k in range(8)] == cr[0]['m'][1].tolist()


def test_gateset_checks_and_fit():
    gs = qsim.GateSet().add_zx(0, 1, 1, 2, 3, np.pi / 2)
    with pytest.raises(ValueError):
        gs.registers([(1, 0)])
    with pytest.raises(ValueError):
        qsim.survival(np.zeros((1, 10, 4), np.int32), 3)
    m = np.array([1, 5, 10, 20, 50, 100])
    A, p = qsim.fit_decay(m, 0.7 * 0.98 ** m + 0.25)
    assert abs(A - 0.7) < 1e-9 and abs(p - 0.98) < 1e-9
    A, p = qsim.fit_decay(m, 0.5 * 0.9 ** m + 0.5, asymptote=0.5)
    assert abs(A - 0.5) < 1e-9 and abs(p - 0.9) < 1e-9


# ---- the 64-register inputs of tests/test_gpu_qsim.py and test_gpu_qsim_meas.py -----------------------------------

WIDE_LDS = {('1q', 1): 51200, ('1q', 5): (1536 + 53 * 176) * 4, ('1q', 37): (1536 + 8 * 176) * 4,
            ('2q', 1): 51200, ('2q', 5): 51200, ('2q', 37): (1536 + 16 * 176) * 4}


def check_wide_reach(which, n_shots, n_gates):
    """the slot windows of qsim_kernel's workgroups on a wide case, and the rows of ``n_gates`` [n_regs, n_shots]
    (the reference's count of applied gates) that make them matter"""
    from tests.test_gpu_qsim import wide_windows
    wgs, slot_first, lds = wide_windows(which, n_shots)
    n_regs = len(slot_first) - 1
    assert lds == WIDE_LDS[which, n_shots] and slot_first[-1] == 64 and n_regs == (64 if which == '1q' else 32)
    rows = n_gates.reshape(-1)
    assert len(rows) == n_regs * n_shots and len(wgs) == (len(rows) + 255) // 256
    deep = 0
    for w, (r_lo, r_hi, sl_lo, sl_hi) in enumerate(wgs):
        assert (1536 + (sl_hi - sl_lo) * 176) * 4 <= lds                     # what the workgroup stages fits
        for row in range(256 * w, min(256 * (w + 1), len(rows))):
            r = row // n_shots
            assert sl_lo <= slot_first[r] and slot_first[r + 1] <= sl_hi     # a row's slots are in the window
            deep += rows[row] > 0 and slot_first[r] > sl_lo
    assert deep >= 1                                     # gates found in slots that are not the window's first
    assert (rows[:256] > 0).any() and (rows[256 * (len(wgs) - 1):] > 0).any()     # in the first and the last workgroup
    widest = max(sl_hi - sl_lo for _, _, sl_lo, sl_hi in wgs)
    if n_shots == 1 or (which, n_shots) == ('2q', 5):
        assert widest == 64 and lds == 51200             # all 64 slots, the largest launch
    if len(wgs) > 1:
        assert any((256 * w) % n_shots for w in range(1, len(wgs)))          # a workgroup starts inside a register
    if n_shots == 37:
        assert {r_hi - r_lo + 1 for r_lo, r_hi, _, _ in wgs[:-1]} == {7, 8}
        assert len({sl_lo for _, _, sl_lo, _ in wgs}) == len(wgs) > 4        # every window starts elsewhere


def test_wide_gatesets_fill_1_to_8_entries():
    from tests.test_gpu_qsim import wide_entries, wide_gateset, wide_regs
    assert sorted(wide_regs('1q')) == list(range(64)) != list(wide_regs('1q'))
    pairs = wide_regs('2q')
    assert sorted(c for r in pairs for c in r) == list(range(64))
    assert 8 <= sum(a > b for a, b in pairs) <= 24
    assert {wide_entries(c) for c in range(64)} == set(range(1, 9))
    for which in ('1q', '2q'):
        gs = wide_gateset(which)
        per = {c: [e for e in gs.entries if e['core'] == c] for c in range(64)}
        assert all(len(per[c]) == wide_entries(c) + (c == 3) for c in range(64))
        firsts = {a for a, _ in pairs} if which == '2q' else set()
        kind1 = {e['core'] for e in gs.entries if e['kind'] == 1}
        assert kind1 == {c for c in firsts if wide_entries(c) >= 2} and (which == '1q' or len(kind1) >= 20)
        assert len(set(gs.detune_words(64).tolist())) >= 60


@pytest.mark.parametrize('n_shots', [1, 5, 37])
@pytest.mark.parametrize('which', ['1q', '2q'])
def test_wide_cases_reach_every_slot_window(which, n_shots):
    from tests.test_gpu_qsim import ORDERS, wide_reference, wide_seed
    for lane_order in ORDERS:
        pops, res = wide_reference(which, n_shots, lane_order, wide_seed(which, n_shots))
        check_wide_reach(which, n_shots, res[:, :, 1])
        assert (res[:, :, 2] > 0).any() and (n_shots == 1 or ((res[:, :, 3] & 0xFFFF) > 0).any())
