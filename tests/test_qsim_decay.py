"""CPU tests of the decaying qubit-state stage (dpemu_qsim_decay, include/dpemu.h;
DESIGN.md §2 "Decoherence"): the specification, through its Python-integer
restatement tests/qsim_decay_ref.py, on event records written by hand
(tests/test_qsim.py's helpers) -- the T1 and T2 experiments against their
exponentials, a 20-gate stream against a density matrix evolved through the
exact Kraus channels, the identity, re-batching, stepping and the edges of the
qubit clock -- and the Python layer (qsim.decay_tables, GateSet.set_decay).
tests/test_gpu_qsim_decay.py holds the kernels to the same reference bit for
bit."""

import functools

import numpy as np
import pytest

from distributed_processor_amd import _abi, qsim, workloads
from tests import qsim_decay_ref as dref, qsim_meas_ref as mref, qsim_ref
from tests.test_qsim import HAND_KEYS, hand_events, hand_gateset, strobe

ONE = 1 << 30
RDLO = workloads.RDLO
X0, CR, X1 = (HAND_KEYS[k] for k in ('x0', 'cr', 'x1'))
SEED = 0xDECA1D0C0FFEE
N = 4096                                                # shots of the T1 and T2 experiments
T1 = 5000


def cfg_of(C_, cap, **kw):
    return _abi.make_config(C_, event_cap=cap, seed=SEED, **kw)


def per_shot(lanes_of_shot, n_shots, C_):
    """core-major lane lists from one shot's per-core record lists, the same in every shot"""
    return [list(lanes_of_shot[c]) for c in range(C_) for _ in range(n_shots)]


def ro(t):
    return strobe(t, 3, 0x0FA000, 0xFFFF, 0x155, elem=RDLO)


def one_qubit(t1=None, t2=None):
    gs = qsim.GateSet(drv_elem=workloads.QDRV).add_rotation(0, *X0, np.pi / 2).registers([0])
    return gs.set_decay(0, t1, t2)


def run(cfg, gs, lanes, n_shots, cap=None, **kw):
    summary, ev = hand_events(lanes, cap)
    return dref.qsim_decay_gateset(cfg, gs, summary, ev, n_shots, event_cap=cap, **kw)


def p_one(pops, which=0):
    """normalised P(1) of qubit ``which`` per row of pops [n, 4]"""
    p = pops.astype(np.float64)
    ones = p[:, 2] + p[:, 3] if which == 0 else p[:, 1] + p[:, 3]
    return ones / p.sum(axis=1)


# ---- 1. the T1 experiment: two X90 at one strobe time, then tau clocks to t_final ----

T1_TAUS = (1000, 5000, 12000)


@functools.lru_cache(maxsize=None)
def t1_case(tau):
    """(cfg, gateset, lanes, t_final): a pi pulse as two X90 at t = 10 (the first finds |0>, where nothing can
    happen; the second no time), then the qubit waits"""
    return cfg_of(1, 2), one_qubit(T1), per_shot([[strobe(10, *X0, 0), strobe(10, *X0, 0)]], N, 1), 10 + tau


def check_t1(tau, pops, counts):
    """every row is |0> or |1>; the share of |1> is e^(-tau / T1) within 5 binomial standard errors; counts shows
    exactly the rows that jumped"""
    p1 = p_one(pops[0])
    assert (np.minimum(p1, 1 - p1) <= 2.0 ** -20).all()
    want = np.exp(-tau / T1)
    mean, se = float((p1 > 0.5).mean()), np.sqrt(want * (1 - want) / N)
    print('T1 tau', tau, 'mean', mean, 'want', want, 'in standard errors', (mean - want) / se)
    assert abs(mean - want) <= 5 * se
    assert ((counts[0, :, 0] == 1) == (p1 < 0.5)).all() and (counts[0, :, 0] <= 1).all() and not counts[0, :, 1:].any()


@pytest.mark.parametrize('tau', T1_TAUS)
def test_t1_experiment(tau):
    cfg, gs, lanes, t_final = t1_case(tau)
    pops, res, states, counts = run(cfg, gs, lanes, N, t_final=t_final)
    assert states is None and (res[0, :, 1] == 2).all()
    check_t1(tau, pops, counts)
    assert ((res[0, :, 0] == 1) == (counts[0, :, 0] == 0)).all()          # the sample of a basis state is that state


# ---- 2. the T2 experiment: X90, wait, X90 at phase words 0 and 0x10000 ----

T2_TAU = 2000
T2_CASES = ((2 * T1, 0), (2 * T1, 0x10000), (3000, 0), (3000, 0x10000))   # T2 = 2 T1 (no pure dephasing), then a shorter T2


@functools.lru_cache(maxsize=None)
def t2_case(t2, phase):
    return cfg_of(1, 2), one_qubit(T1, t2), per_shot([[strobe(10, *X0, 0), strobe(10 + T2_TAU, *X0, phase)]], N, 1)


def check_t2(t2, phase, pops):
    """the mean P(1) is (1 +- e^(-tau / T2)) / 2 within 5 standard errors; a row's P(1) lies in [0, 1], so its
    standard deviation is at most 1/2"""
    want = 0.5 * (1 + (-1 if phase else 1) * np.exp(-T2_TAU / t2))
    mean = float(p_one(pops[0]).mean())
    print('T2', t2, 'phase', hex(phase), 'mean', mean, 'want', want, 'in standard errors', (mean - want) / (0.5 / np.sqrt(N)))
    assert abs(mean - want) <= 5 * 0.5 / np.sqrt(N)


@pytest.mark.parametrize('t2,phase', T2_CASES)
def test_t2_experiment(t2, phase):
    cfg, gs, lanes = t2_case(t2, phase)
    pops, res, _, counts = run(cfg, gs, lanes, N)
    check_t2(t2, phase, pops)
    assert counts[0, :, 0].any() and (counts[0, :, 1].any() == (t2 < 2 * T1))     # flips only under pure dephasing


# ---- 3. against the density matrix ----

PHYS_N, PHYS_T1, PHYS_T2 = 2048, 4000, 2500
PHYS_ROT = ((0, 0x040000, 7000, np.pi / 2, 0.0), (1, 0x040000, 7100, 1.1, 0.3), (2, 0x040000, 7200, 2.7, 0.65))


@functools.lru_cache(maxsize=1)
def physics_case():
    """20 gates on one qubit, gaps of 3 .. 3,000 clocks, three rotations at random phase words, then 700 clocks"""
    rng = np.random.default_rng(2024)
    gs = qsim.GateSet(drv_elem=workloads.QDRV)
    for freq, env, amp, theta, axis in PHYS_ROT:
        gs.add_rotation(0, freq, env, amp, theta, axis)
    gs.registers([0]).set_decay(0, PHYS_T1, PHYS_T2)
    t, recs, gates = 0, [], []
    for _ in range(20):
        t += int(rng.choice([3, 17, 150, 800, 3000]))
        which, phase = int(rng.integers(0, 3)), int(rng.integers(0, 1 << 17))
        recs.append(strobe(t, *PHYS_ROT[which][:3], phase))
        gates.append((t, which, phase))
    return cfg_of(1, 20), gs, per_shot([recs], PHYS_N, 1), gates, t + 700


def density_matrix(gates, t_final):
    """complex128 rho through the exact channels: amplitude damping (Kraus K0 = diag(1, sqrt(1 - g)), K1 =
    sqrt(g) |0><1|, g = 1 - e^(-dt / T1)), then dephasing (rho -> (1 - p) rho + p Z rho Z, 1 - 2 p = e^(-dt / Tphi)),
    before every unitary Rz(phi) M Rz(-phi)"""
    rho = np.array([[1, 0], [0, 0]], np.complex128)
    z = np.diag([1.0, -1.0]).astype(np.complex128)
    rate_phi = 1.0 / PHYS_T2 - 1.0 / (2 * PHYS_T1)

    def wait(rho, dt):
        g = 1 - np.exp(-dt / PHYS_T1)
        k0, k1 = np.diag([1, np.sqrt(1 - g)]).astype(np.complex128), np.array([[0, np.sqrt(g)], [0, 0]], np.complex128)
        rho = k0 @ rho @ k0.conj().T + k1 @ rho @ k1.conj().T
        p = (1 - np.exp(-dt * rate_phi)) / 2
        return (1 - p) * rho + p * z @ rho @ z

    tl = 0
    for t, which, phase in gates:
        rho, tl = wait(rho, t - tl), t
        rz = np.diag([1, np.exp(2j * np.pi * phase / 2 ** 17)])
        u = rz @ qsim.rotation(*PHYS_ROT[which][3:]) @ rz.conj().T
        rho = u @ rho @ u.conj().T
    return wait(rho, t_final - tl)


def check_physics(pops):
    cfg, gs, lanes, gates, t_final = physics_case()
    rho = density_matrix(gates, t_final)
    p = pops[0].astype(np.float64)
    p /= p.sum(axis=1, keepdims=True)
    assert not p[:, [1, 3]].any()
    for j, want in ((0, rho[0, 0].real), (2, rho[1, 1].real)):
        mean, se = p[:, j].mean(), p[:, j].std(ddof=1) / np.sqrt(PHYS_N)
        print('population', j, 'mean', mean, 'want', want, 'in standard errors', (mean - want) / se)
        assert 0.05 < want < 0.95 and abs(mean - want) <= 5 * se          # (se <= 0.5 / sqrt N: the values lie in [0, 1])


def test_trajectories_match_the_density_matrix():
    cfg, gs, lanes, gates, t_final = physics_case()
    pops, res, _, counts = run(cfg, gs, lanes, PHYS_N, t_final=t_final)
    assert (res[0, :, 1] == 20).all() and counts[0, :, 0].any() and counts[0, :, 1].any()
    check_physics(pops)


# ---- 4. identity: all-2^30 tables are the base calls, on a fuzz stream ----

@pytest.mark.parametrize('lane_order', [_abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR], ids=['core_major', 'shot_major'])
def test_identity_tables_are_the_base_calls(lane_order):
    from tests.test_gpu_qsim_meas import C_FUZZ, fuzz_cfg, fuzz_gateset, fuzz_records
    n, shot0 = 16, 2 ** 32 - 7
    summary, ev = fuzz_records(n, lane_order, 416)
    cfg, gs = fuzz_cfg(lane_order), fuzz_gateset()
    tables = tuple(np.full((C_FUZZ, 32), ONE, np.uint32) for _ in range(2))
    advances = []
    got = dref.qsim_decay_gateset(cfg, gs, summary, ev, n, shot0, measure_readouts=True, tables=tables, advances=advances)
    want = mref.qsim_meas_gateset(cfg, gs, summary, ev, n, shot0)
    for g, w in zip(got[:3], want):
        np.testing.assert_array_equal(g, w)
    assert not got[3].any() and len(advances) > 100 and want[2].any()
    got = dref.qsim_decay_gateset(cfg, gs, summary, ev, n, shot0, tables=tables)
    want = qsim_ref.qsim_gateset(cfg, gs, summary, ev, n, shot0)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1])
    assert got[2] is None and not got[3].any()


# ---- 5. two qubits: the target's advance and its counter tag, jumps on both qubits, a long span ----

TWO_N, TWO_T1 = 256, 100000
TWO_FINAL = 420000


@functools.lru_cache(maxsize=1)
def two_qubit_case():
    """both qubits prepared in |1> at t = 10; the control's ZX90 (its slot 2) at t = 200,010 advances the control
    over dt = 200,000 = 0x30D40 (bits 16 and 17) and then the target; the target's own pulse at t = 300,010 is ITS
    slot 2, so the two advances of core 1 meet at one counter n and differ by their tags alone; a readout of each"""
    gs = hand_gateset().set_decay(0, TWO_T1, TWO_T1).set_decay(1, TWO_T1 // 2)
    lanes = [[strobe(10, *X0, 0), strobe(10, *X0, 0), strobe(200010, *CR, 0), ro(400000)],
             [strobe(10, *X1, 0), strobe(10, *X1, 0), strobe(300010, *X1, 0), ro(400000)]]
    return cfg_of(2, 4, meas_elem=RDLO), gs, per_shot(lanes, TWO_N, 2)


def test_two_qubit_reach():
    cfg, gs, lanes = two_qubit_case()
    advances = []
    pops, res, states, counts = run(cfg, gs, lanes, TWO_N, measure_readouts=True, t_final=TWO_FINAL, advances=advances)
    assert any(dt >> 16 for _, _, _, _, dt, _, _ in advances) and 200000 >> 16 == 3
    row0 = [(core, tag, n) for row, core, tag, n, _, _, _ in advances if row == 0]
    assert (1, dref.TARGET_CTR, 2) in row0 and (1, dref.OWN_CTR, 2) in row0 and (0, dref.OWN_CTR, 2) in row0
    assert (0, dref.FINAL_CTR, 0) in row0 and (1, dref.FINAL_CTR, 0) in row0
    assert counts[0, :, 0].any() and counts[0, :, 2].any() and counts[0, :, 1].any()      # a jump on each qubit; flips
    assert not counts[0, :, 3].any()                                                      # core 1: T2 = 2 T1
    assert (res[0, :, 1] == 6).all() and set(states.tolist()) == {0, 1}
    # with the target's tag on the own-record counter the rows would differ: the draws of the two tags do
    from tests.demod_iq_ref import philox4
    assert philox4(SEED, 0, dref.TARGET_CTR | 1, 2) != philox4(SEED, 0, dref.OWN_CTR | 1, 2)


# ---- 6. re-batching, stepping, the edges of the clock ----

def test_two_half_batches():
    """counter-based draws: shots [5, 21) and [21, 37) in two runs equal [5, 37) in one, on every output"""
    cfg, gs, lanes = two_qubit_case()
    lanes32, lanes16 = per_shot([lanes[0], lanes[TWO_N]], 32, 2), per_shot([lanes[0], lanes[TWO_N]], 16, 2)
    whole = run(cfg, gs, lanes32, 32, shot_begin=5, measure_readouts=True, t_final=TWO_FINAL)
    for b in (0, 16):
        part = run(cfg, gs, lanes16, 16, shot_begin=5 + b, measure_readouts=True, t_final=TWO_FINAL)
        for k in (0, 1, 3):
            np.testing.assert_array_equal(part[k], whole[k][:, b:b + 16])
        np.testing.assert_array_equal(part[2].reshape(2, 16), whole[2].reshape(2, 32)[:, b:b + 16])
    assert whole[3].any()


def test_an_unmatched_strobe_does_not_split_an_advance():
    """a drive strobe without a dictionary entry between two pulses advances nothing: the rows equal those of a
    stream with a record of another element in its slot (the later record keeps its slot k), n_unmatched apart"""
    n = 64
    cfg, gs = cfg_of(1, 4), one_qubit(800, 500)
    head, tail = [strobe(10, *X0, 0), strobe(10, *X0, 0)], [strobe(1500, *X0, 0x4000)]
    split = run(cfg, gs, per_shot([head + [strobe(700, 9, 9, 9, 0)] + tail], n, 1), n, t_final=1600)
    whole = run(cfg, gs, per_shot([head + [strobe(700, *X0, 0, elem=1)] + tail], n, 1), n, t_final=1600)
    np.testing.assert_array_equal(split[0], whole[0])
    np.testing.assert_array_equal(split[3], whole[3])
    assert (split[1][0, :, 2] == 1).all() and (whole[1][0, :, 2] == 0).all()
    np.testing.assert_array_equal(split[1][0][:, [0, 1, 3]], whole[1][0][:, [0, 1, 3]])
    assert split[3][0, :, 0].any() and split[3][0, :, 1].any() and len(np.unique(split[0][0], axis=0)) >= 3


def test_clock_edges():
    """a record with t <= tl advances nothing (out-of-order records are defined); t_final at or before the last
    advance does nothing"""
    n = 64
    cfg, gs = cfg_of(1, 4), one_qubit(800, 500)
    back, advances = per_shot([[strobe(1000, *X0, 0), strobe(400, *X0, 0x4000), strobe(1000, *X0, 0x123)]], n, 1), []
    got = run(cfg, gs, back, n, advances=advances)
    assert sorted({(k, dt) for _, _, _, k, dt, _, _ in advances}) == [(0, 1000)]
    same_t = per_shot([[strobe(1000, *X0, 0), strobe(1000, *X0, 0x4000), strobe(1000, *X0, 0x123)]], n, 1)
    want = run(cfg, gs, same_t, n)                      # (no detuning: a gate does not read its t)
    for g, w in zip(got, want):
        np.testing.assert_array_equal(g, w)
    for t_final in (1, 999, 1000):
        early = run(cfg, gs, back, n, t_final=t_final)
        for g, w in zip(early, got):
            np.testing.assert_array_equal(g, w)
    assert not np.array_equal(run(cfg, gs, back, n, t_final=1001 + 4000)[0], got[0])


def test_span_factor():
    damp, _ = qsim.decay_tables(5000)
    assert dref.span_factor(damp, 0) == ONE and dref.span_factor(damp, 1) == damp[0] and dref.span_factor(damp, 1 << 31) == damp[31]
    for dt in (3, 1000, 0x30D40, 0xFFFFFFFF):
        assert abs(dref.span_factor(damp, dt) / ONE - np.exp(-dt / 10000)) < 40 * 2.0 ** -30   # 32 roundings at most
    assert dref.span_factor(np.zeros(32, np.uint32), 5) == 0 and dref.span_factor(np.full(32, ONE), 0xFFFFFFFF) == ONE


# ---- 7. the Python layer ----

def test_set_decay_tables_and_refusals():
    damp, deph = qsim.decay_tables(5000, 3000)
    i = np.arange(32)
    assert damp.dtype == np.uint32 and damp.shape == deph.shape == (32,)
    assert (damp == np.rint(np.exp(-2.0 ** i / 10000) * ONE)).all()
    assert (deph == np.rint(np.exp(-2.0 ** i * (1 / 3000 - 1 / 10000)) * ONE)).all()
    assert damp[0] == 1073634455 and damp[31] == 0 and (np.diff(damp.astype(np.int64)) < 0)[:15].all()
    assert (qsim.decay_tables(5000)[1] == ONE).all() and (qsim.decay_tables(5000, 10000)[1] == ONE).all()   # T2 = 2 T1
    assert (qsim.decay_tables(None, 3000)[0] == ONE).all() and qsim.decay_tables(None, 3000)[1][0] == np.rint(np.exp(-1 / 3000) * ONE)
    assert all((t == ONE).all() for t in qsim.decay_tables())
    for bad in ((5000, 10001), (0, None), (-1, None), (5000, 0), (float('nan'), None), (float('inf'), None)):
        with pytest.raises(ValueError):
            qsim.decay_tables(*bad)
    gs = one_qubit()
    assert gs.decay and qsim.GateSet().decay == {}
    gs = qsim.GateSet().registers([0, 2]).set_decay(2, 5000, 3000)
    cfg = cfg_of(4, 4)
    st, (d, p) = gs.decay_struct(cfg, t_final=77)
    assert st.t_final == 77 and st.damp == d.ctypes.data and st.deph == p.ctypes.data
    assert d.shape == p.shape == (4, 32) and (d[[0, 1, 3]] == ONE).all() and (d[2] == damp).all() and (p[2] == deph).all()
    with pytest.raises(ValueError):
        gs.decay_struct(cfg_of(2, 4))                    # core 2 of 2
    with pytest.raises(ValueError):
        gs.decay_struct(cfg, t_final=2 ** 32)
    with pytest.raises(ValueError):
        gs.set_decay(2, 100, 201)
    rd, rp = dref.decay_words(gs, 4)
    assert (rd == d).all() and (rp == p).all()
