"""CPU reference of the readout statistics stage (dpemu_iq_stats,
include/dpemu.h; DESIGN.md §2 "Readout statistics"): a numpy restatement of
the specification, the sums in int64 exactly as the table holds them.  Not
test code of its own: tests/test_iq_stats.py validates the specification and
the Python layer with it on the CPU, tests/test_gpu_iq_stats.py holds the
kernel to it bit for bit."""

import numpy as np

from distributed_processor_amd import _abi

M32 = np.uint64(0xFFFFFFFF)
STAT_WORDS = 16


def philox_word0(seed, shot, core, m):
    """word 0 of Philox4x32-10, counter (shot low, shot high, core, m), key =
    seed, for arrays of shot (uint64), core and m: demod_iq_ref.philox4,
    vectorised in uint64 (a product of two 32-bit values fits)"""
    shot = np.asarray(shot, np.uint64)
    c = [shot & M32, shot >> np.uint64(32), np.asarray(core, np.uint64) & M32, np.asarray(m, np.uint64) & M32]
    c = [np.broadcast_to(x, np.broadcast(*c).shape).copy() for x in c]
    k0, k1 = np.uint64(int(seed) & 0xFFFFFFFF), np.uint64((int(seed) >> 32) & 0xFFFFFFFF)
    s32 = np.uint64(32)
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(0xD2511F53), c[2] * np.uint64(0xCD9E8D57)
        c = [(p1 >> s32) ^ c[1] ^ k0, p1 & M32, (p0 >> s32) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M32, (k1 + np.uint64(0xBB67AE85)) & M32
    return c[0]


def states(cfg, shot, core, m):
    """prepared state of readouts (shot, core, m): the draw against p1_threshold[core]"""
    thr = np.array([cfg.p1_threshold[c] for c in range(_abi.MAX_CORES)], np.uint64)[np.asarray(core, np.int64)]
    return ((thr == M32) | (philox_word0(cfg.seed, shot, core, m) < thr)).astype(np.int64)


def run_columns(cfg, n_cols, shot_begin=0):
    """(core, shot) of every column of the run layout (include/dpemu.h lane orders)"""
    C_ = cfg.cores_per_shot
    assert n_cols % C_ == 0
    col = np.arange(n_cols, dtype=np.int64)
    if cfg.lane_order == _abi.LANES_SHOT_MAJOR:
        core, sl = col % C_, col // C_
    else:
        core, sl = col // max(n_cols // C_, 1), col % max(n_cols // C_, 1)
    return core.astype(np.uint32), (sl + int(shot_begin)).astype(np.uint64)


def s16(v):
    return ((np.asarray(v, np.int64) & 0xFFFF) ^ 0x8000) - 0x8000


def readout_words(i, q, o):
    """the 16 int64 words of single readouts {I, Q} with outcome o: [..., 16]"""
    i, q = np.asarray(i, np.int64), np.asarray(q, np.int64)
    a_i, b_i, a_q, b_q = i >> 16, i & 0xFFFF, q >> 16, q & 0xFFFF
    z = np.zeros_like(i)
    return np.stack([z + 1, np.asarray(o, np.int64), i, q, a_i * a_i, a_i * b_i, b_i * b_i, a_q * a_q, a_q * b_q,
                     b_q * b_q, a_i * a_q, a_i * b_q + b_i * a_q, b_i * b_q, z, z, z], axis=-1)


def iq_stats(cfg, acc, counts, core=None, shot=None, shot_begin=0, by_slot=False, axis=None, thr=None):
    """acc int32 (meas_cap, n_cols, 2); counts (n_cols,) readouts per column;
    core / shot per column, or both None for the run layout.  axis: per-core
    Q15 words (default cfg.ro_axis), thr: per-core thresholds (default
    cfg.ro_thr).  Returns table int64 (S, C, 2, 16), bits uint32 (n_cols,)."""
    acc = np.asarray(acc)
    meas_cap, n_cols = acc.shape[:2]
    C_ = cfg.cores_per_shot
    if core is None:
        core, shot = run_columns(cfg, n_cols, shot_begin)
    core, shot = np.asarray(core, np.int64), np.asarray(shot, np.uint64)
    ax = np.array([cfg.ro_axis[c] for c in range(C_)] if axis is None else axis, np.int64)
    th = np.array([cfg.ro_thr] * C_ if thr is None else thr, np.int64)
    S = meas_cap if by_slot else 1
    table = np.zeros((S, C_, 2, STAT_WORDS), np.int64)
    bits = np.zeros(n_cols, np.uint32)
    count = np.minimum(np.asarray(counts, np.int64), meas_cap)
    for m in range(meas_cap):
        on = count > m
        if not on.any():
            continue
        i, q = acc[m, on, 0].astype(np.int64), acc[m, on, 1].astype(np.int64)
        cr = core[on]
        o = (((i * s16(ax[cr]) + q * s16(ax[cr] >> 16)) >> 15) > th[cr]).astype(np.int64)
        bits[on] |= (o << m).astype(np.uint32)
        st = states(cfg, shot[on], cr, m)
        np.add.at(table[m if by_slot else 0], (cr, st), readout_words(i, q, o))
    return table, bits
