"""Hand-built inputs for the readout and DDS kernels: event records, pair tables
and iq rows that the pipeline above them (dpemu_run on tiny programs,
dpemu_dds on well-formed tables) never produces.  Not test code of its own:
tests/test_handbuilt_inputs.py runs the CPU references on every input set and
asserts that each reaches what it was built to reach;
tests/test_gpu_readout_direct.py and tests/test_gpu_dds.py hold the kernels to
the same references on the same inputs (same builders, same seeds).

The builders follow tests/test_gpu_dds.py's hand-made ``ChannelPlan``
(``__new__`` plus hand-set fields).  The pair columns are given explicitly, so
nothing here depends on ``cfg.lane_order`` (the readout kernels do not read
it: a pair names its lane)."""

import functools

import numpy as np

from distributed_processor_amd import _abi
from distributed_processor_amd.dds import DemodPairTable, FeedlineTable
from distributed_processor_amd.hwconfig import DDSElementConfig
from tests import demod_iq_ref, feedline_ref, resonator_ref
from tests.test_demod import RDLO, RDRV

CORNERS = (0x80008000, 0x7FFF7FFF, 0x80007FFF, 0x7FFF8000, 0)      # constant rows: the box corners and zero
OCTANTS = [k * (1 << 29) for k in range(8)]                        # ro_theta words k * 45 degrees


def events(n_lanes, event_cap, meas_elem, readouts, counts=None, seed=0):
    """summary uint32 (n_lanes, 8) and events uint32 (event_cap, n_lanes, 4).

    ``readouts[lane]`` is {event index: (t, L)}: a readout strobe (kind 0,
    cfg & 3 == meas_elem, cfg's upper bits random) with time t and env word
    length field L (0: 4,096 words) and a random address field.  Every other
    slot holds a record that must not count, in turn a strobe of another
    element, a kind-1 record whose cfg bits equal meas_elem, and a record of
    kind >= 2; its time runs from the readout before it to the one after it,
    so a lane's times (in index order of the given readouts) do not decrease.
    ``counts[lane]`` is summary word 2 (default event_cap); the other summary
    words hold noise, which nothing may read."""
    rng = np.random.default_rng(seed)
    summary = rng.integers(0, 2 ** 32, (n_lanes, 8), dtype=np.uint64).astype(np.uint32)
    ev = np.zeros((event_cap, n_lanes, 4), np.uint32)
    i = np.arange(event_cap)
    for lane in range(n_lanes):
        reads = dict(readouts[lane]) if lane < len(readouts) else {}
        assert all(0 <= e < event_cap for e in reads)
        at = sorted(reads)
        t = np.interp(i, at, [reads[e][0] for e in at]).astype(np.uint64) if at else np.zeros(event_cap, np.uint64)
        other = (meas_elem + 1 + rng.integers(0, 3, event_cap)) & 3
        cfg = [other | (rng.integers(0, 4, event_cap) << 2), meas_elem | (rng.integers(0, 4, event_cap) << 2),
               rng.integers(0, 16, event_cap)]
        kind = [np.zeros(event_cap, np.int64), np.ones(event_cap, np.int64), rng.integers(2, 16, event_cap)]
        which = (i + lane) % 3
        w1 = rng.integers(0, 1 << 24, event_cap)
        w1 = w1 | (np.choose(which, cfg) << 24) | (np.choose(which, kind) << 28)
        for e, (t_e, L) in reads.items():
            t[e] = t_e
            w1[e] = int(rng.integers(0, 1 << 12)) | (L << 12) | ((meas_elem | (int(rng.integers(0, 4)) << 2)) << 24)
        ev[:, lane, 0] = t.astype(np.uint32)
        ev[:, lane, 1] = w1.astype(np.uint32)
        ev[:, lane, 2:] = rng.integers(0, 2 ** 32, (event_cap, 2), dtype=np.uint64).astype(np.uint32)
        summary[lane, 2] = event_cap if counts is None else counts[lane]
    return summary, ev


def pair_table(cols, n_lanes, event_cap, n_rows):
    """a DemodPairTable from its columns (DemodPairTable.FIELDS), with no plans"""
    pt = DemodPairTable.__new__(DemodPairTable)
    pt.cols = {f: np.ascontiguousarray(cols[f], np.uint64 if f == 'shot' else np.uint32) for f in DemodPairTable.FIELDS}
    pt.n_pairs = len(pt.cols['lane'])
    assert all(len(v) == pt.n_pairs for v in pt.cols.values())
    pt.n_lanes, pt.event_cap, pt.n_rows = int(n_lanes), int(event_cap), (int(n_rows[0]), int(n_rows[1]))
    return pt


def random_words(rng, shape):
    return rng.integers(0, 2 ** 32, shape, dtype=np.uint64).astype(np.uint32)


class Case:
    """one input set of tests/test_gpu_readout_direct.py: cfg, summary, events, the pair columns, lines, the two
    iq arrays, ``adc_in`` (a caller-made ADC trace, or None) and the seed of the resonator table"""

    def __init__(self, name, cfg, summary, ev, cols, lines, iq_drv, iq_lo, adc_in=None, res_seed=1):
        self.name, self.cfg, self.summary, self.events = name, cfg, summary, ev
        self.iq_drv, self.iq_lo, self.adc_in, self.res_seed = iq_drv, iq_lo, adc_in, res_seed
        self.pt = pair_table(cols, summary.shape[0], ev.shape[0], (iq_drv.shape[0], iq_lo.shape[0]))
        self.lines = [list(ln) for ln in lines]
        self.ft = FeedlineTable(self.pt, self.lines)
        self.n_lo = iq_lo.shape[1]
        assert cfg.event_cap == ev.shape[0] and self.n_lo % 4 == 0

    def resonators(self):
        from tests.test_gpu_resonator import random_table
        return random_table(self.pt, self.res_seed)

    def reads(self, pair):
        return feedline_ref.kept_readouts(self.cfg, self.summary, self.events, int(self.pt.cols['lane'][pair]),
                                          self.cfg.meas_cap, self.cfg.event_cap)

    def windows(self, pair):
        """[(j0, j1)] the LO samples of the pair's kept readouts"""
        spc_l = int(self.pt.cols['spc_lo'][pair])
        return [(min(t * spc_l, self.n_lo), min((t + ((pe >> 12 & 0xFFF) or 4096) * self.cfg.ro_cpw) * spc_l, self.n_lo))
                for t, pe in self.reads(pair)]


def cols_for(lanes, cores, shots, drv_rows, lo_rows, spc):
    n = len(lanes)
    return dict(lane=lanes, core=cores, shot=shots, drv_row=drv_rows, lo_row=lo_rows, spc_drv=[spc[0]] * n,
                spc_lo=[spc[1]] * n)


# ---- C1: the scan over all sixteen chunks ----

SCAN_COUNTS = [32, 6, 32, 0, 1, 3, 4, 32]            # the kept readouts of lanes (a) .. (h)
SCAN_A = ([5, 63, 64, 100, 130, 190, 200, 255, 256, 300, 330, 380, 390, 440, 450, 500, 520, 570, 580, 630, 650, 700,
           710, 760] + [770, 780, 790, 800, 810, 820, 830] + [832, 840, 850] + [900, 950] + [960, 1000, 1010, 1023])


def scan_case(spc):
    """event_cap 1,024, meas_cap 32, 8 lanes (a) .. (h), one pair per lane; windows of 1..3 words at ro_cpw 4"""
    n_clks = 1300                                    # 1,300 / 5,200 LO samples: multiples of 4, not of 64
    a = {e: (8 + 32 * r, 1 + r % 3) for r, e in enumerate(SCAN_A)}
    b = {e: (30 + 200 * r, 1 + r % 3) for r, e in enumerate((3, 500, 990, 1000, 1020, 1023))}
    c = {992 + r: (9 + 40 * r, 3 - r % 3) for r in range(32)}
    e_ = {1023: (640, 2)}
    f = {e: (100 + r, 2) for r, e in enumerate((10, 300, 699, 700, 800, 1023))}       # count 700: three are stale
    g = {100: (50, 3), 101: (50, 1), 400: (58, 2), 900: (300, 3)}    # a tie; 58 is inside the window [50, 62)
    h = {7 + 31 * r: (3 + 39 * r, 1 + (r + 1) % 3) for r in range(33)}
    summary, ev = events(8, 1024, RDLO, [a, b, c, {}, e_, f, g, h], counts=[1024, 1030, 1024, 1024, 1024, 700, 1024, 1024],
                         seed=101 + spc[0])
    rng = np.random.default_rng(202 + spc[0])
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=1024, meas_cap=32, meas_latency=32, seed=0xC3,
                           p1=[0.0, 1.0, 0.5, 0.4],
                           demod=dict(drv_elem=RDRV, cpw=4, delay=20, theta=(0.7, 3.9), gain=(0.8, 0.6),
                                      axis=[0.3, 1.9, 4.0, 5.5], sigma=90.0, thr=0))
    assert [cfg.p1_threshold[c_] for c_ in (0, 1)] == [0, 0xFFFFFFFF]
    lanes = list(range(8))
    cols = cols_for(lanes, [(L + 2) % 4 for L in lanes], [1000 + L // 4 for L in lanes], [3, 0, 7, 1, 6, 2, 5, 4],
                    [4, 6, 0, 2, 7, 1, 3, 5], spc)
    lines = [[0, 6, 3], [1, 2, 4, 7], [5]]
    return Case('scan', cfg, summary, ev, cols, lines, random_words(rng, (8, n_clks * spc[0])),
                random_words(rng, (8, n_clks * spc[1])), res_seed=301)


# ---- C2: full-range words ----

FULL_RANGE = {'oct01': (0, 1, None), 'oct23': (2, 3, None), 'oct45': (4, 5, None), 'oct67': (6, 7, None),
              'gains': (1, 6, (41234, 57001))}


def full_range_case(which):
    """12 pairs at 16:4 on 7 lines, four readouts each (one with L = 0, clipped by n_samples_lo); random and
    constant corner rows of drive, LO and a caller-made ADC; ro_theta on two of the eight octants"""
    o0, o1, gains = FULL_RANGE[which]
    n_pairs, n_clks, spc = 12, 1001, (16, 4)
    rng = np.random.default_rng(400 + o0)
    reads = [{2: (5 + 3 * L, 10), 5: (200 + L, 1 + L), 9: (420 - 7 * L, 3), 14: (700 + 20 * L, 0)} for L in range(n_pairs)]
    summary, ev = events(n_pairs, 16, RDLO, reads, counts=[16] * 11 + [15], seed=500 + o0)
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=16, meas_cap=4, meas_latency=32, seed=0xC2 + o0,
                           p1=[0.5, 0.4, 0.6, 0.5],
                           demod=dict(drv_elem=RDRV, cpw=4, delay=3, axis=[0.3, 1.9, 4.0, 5.5], sigma=120.0, thr=-5000))
    cfg.ro_theta[0], cfg.ro_theta[1] = OCTANTS[o0], OCTANTS[o1]
    if gains is not None:
        cfg.ro_gain[0], cfg.ro_gain[1] = gains
    assert gains is not None or (cfg.ro_gain[0], cfg.ro_gain[1]) == (65536, 65536)

    def rows(n_random, n):
        r = random_words(rng, (n_random + len(CORNERS), n))
        for k, w in enumerate(CORNERS):
            r[n_random + k] = w
        return r
    iq_drv, iq_lo = rows(7, 16 * 1000), rows(7, 4 * n_clks)        # the drive rows end one clock before the LO rows
    lanes = list(range(n_pairs))
    # pair 3: LO row 7 = 0x80008000 under line 1's ADC row 0x80008000; pairs 9, 10: corner drives under random LOs
    cols = cols_for(lanes, [L % 4 for L in lanes], [77 + L // 4 for L in lanes], [4, 9, 0, 7, 11, 2, 8, 5, 10, 1, 6, 3],
                    [2, 10, 5, 7, 0, 8, 3, 11, 6, 1, 9, 4], spc)
    lines = [[0, 1, 2], [3, 4], [5], [6, 7], [8], [9, 10], [11]]
    adc = random_words(rng, (7, 4 * n_clks))
    adc[0, ::7] = (adc[0, ::7] & 0xFFFF0000) | 0x8000               # I = -32768 on every seventh word
    adc[6, ::5] = (adc[6, ::5] & 0xFFFF0000) | 0x8000
    for k, w in enumerate(CORNERS):
        adc[1 + k] = w
    return Case('full_range_' + which, cfg, summary, ev, cols, lines, iq_drv, iq_lo, adc_in=adc, res_seed=302)


# ---- C3: the int32 clamp of sig and the wrap of acc ----

def clamp_case():
    """4 pairs at 1:1, constant corner rows under one 4,096-word window at the largest ro_cpw (8): 32,768 LO samples"""
    n_lo = 4 + 4096 * _abi.RO_CPW_MAX + 4                           # 32,776: a multiple of 4, not of 64
    reads = [{3: (4, 0), 9: (40000, 2)} for _ in range(4)]
    summary, ev = events(4, 16, RDLO, reads, seed=600)
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=16, meas_cap=4, meas_latency=32, seed=0xC4, p1=0.5,
                           demod=dict(drv_elem=RDRV, cpw=_abi.RO_CPW_MAX, delay=0, theta=(0.0, 0.0), axis=0.4,
                                      sigma=255.0, thr=0))

    def const_rows(words):
        return np.repeat(np.array(words, np.uint32)[:, None], n_lo, axis=1)
    lanes = list(range(4))
    cols = cols_for(lanes, lanes, [9] * 4, [0, 0, 1, 0], [0, 3, 1, 2], (1, 1))
    adc = const_rows([0x80008000, 0x80008000, 0x80008000, 0x7FFF7FFF])
    return Case('clamp', cfg, summary, ev, cols, [[0], [1], [3], [2]], const_rows(CORNERS[:2]), const_rows(CORNERS[:4]),
                adc_in=adc, res_seed=303)


# ---- C4: buffer edges ----

EDGES = ('four_samples', 'delay_past_every_clock', 'short_drive')
EDGE_CUT = 16 * 50 + 8                                              # short_drive: the drive rows end inside clock 50


def edge_case(which):
    rng = np.random.default_rng(700 + EDGES.index(which))
    spc, delay = (1, 1), 0
    if which == 'four_samples':
        # windows from sample 0, at the last LO sample, one clock past the end and far past it
        n_lo, n_drv = 4, 4
        reads = [{0: (0, 1), 7: (3, 2), 8: (4, 1), 15: (3000000000, 0)}, {4: (3, 0)}, {1: (1, 1), 2: (2, 1)}]
    elif which == 'delay_past_every_clock':
        n_lo, n_drv, delay = 260, 260, 300
        reads = [{1: (10, 5), 6: (100, 0)}, {3: (259, 1)}, {5: (0, 3)}]
    else:
        # 16:4, 100 clocks of LO; the drive index runs off its row at LO sample 4 * 50 + 2 = 202, inside the window
        # [160, 240) of every lane and inside the resonator's tile [192, 256)
        spc, n_lo, n_drv = (16, 4), 400, EDGE_CUT
        reads = [{2: (40, 5), 11: (90, 0)}, {0: (40, 5)}, {9: (40, 5), 10: (45, 1)}]
    summary, ev = events(3, 16, RDLO, reads, seed=800 + EDGES.index(which))
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=16, meas_cap=4, meas_latency=32, seed=0xC5, p1=0.5,
                           demod=dict(drv_elem=RDRV, cpw=4, delay=delay, theta=(0.3, 2.0), axis=0.4, sigma=30.0, thr=0))
    # drive words of magnitude >= 2,000 per component: every return before the cut-off is nonzero
    mag = rng.integers(2000, 30000, (2, 3, n_drv)) * rng.choice([-1, 1], (2, 3, n_drv))
    iq_drv = ((mag[0] & 0xFFFF) | ((mag[1] & 0xFFFF) << 16)).astype(np.uint32)
    cols = cols_for([0, 1, 2], [1, 2, 3], [5, 5, 5], [2, 0, 1], [1, 2, 0], spc)
    return Case('edge_' + which, cfg, summary, ev, cols, [[1], [2, 0]], iq_drv, random_words(rng, (3, n_lo)), res_seed=304)


# ---- C5: many pairs at 32 slots: more pairs of one (core, spc_lo) group than a trace workgroup stages at once ----

MANY_GROUPS = {2: 72, 0: 33, 3: 32, 1: 5}            # pairs per core (one spc_lo per case: a core is a group)
MANY_COUNTS = (0, 1, 2, 31, 32, 40)                  # readout strobes of a lane; 40 > meas_cap, 0: none
MANY_FILLER = (0, 22, 41)                            # the event slots left to hb.events' filler: one of each sort
MANY_EVENT_CAP = 40 + len(MANY_FILLER)
MANY_CLKS = 420                                      # 420 / 1,680 LO samples: multiples of 4, not of 64
MANY_LINE_SIZES = (16, 1, 7, 3, 16, 2, 9, 12, 5, 16, 4, 1, 11, 8, 13, 16, 2)


def many_pairs_case(spc, meas_cap=32):
    """142 pairs of 4 cores in groups of 72, 33, 32 and 5, the table shuffled, every pair on a lane of its own (a
    permutation); per pair 0, 1, 2, 31, 32 or 40 readouts with windows of 1..3 words at ro_cpw 4, 13 clocks apart:
    the 32nd of a lane starts at clock 403 + lane % 17 and is clipped by, or lies past, the 420 clocks of the rows;
    lanes of 1 or 2 readouts start anywhere in the rows, every fifth within their last four clocks.  Pairs share 8 drive and 8 LO rows; lines of 1..16
    members across the cores.  ``meas_cap`` 17: the same inputs, 60 pairs to a staging run instead of 32"""
    n = sum(MANY_GROUPS.values())
    rng = np.random.default_rng(900 + spc[0])
    cores = np.array([c_ for c_, k in MANY_GROUPS.items() for _ in range(k)])[rng.permutation(n)]
    shots = np.zeros(n, np.int64)
    for c_ in MANY_GROUPS:
        shots[cores == c_] = 3000 + np.arange(MANY_GROUPS[c_])
    lanes = rng.permutation(n)
    n_strobes = np.array(MANY_COUNTS)[(np.arange(n) + np.arange(n) // 6) % 6]
    free = [i for i in range(MANY_EVENT_CAP) if i not in MANY_FILLER]
    reads = [None] * n
    for p in range(n):
        lane, k = int(lanes[p]), int(n_strobes[p])
        at = sorted(rng.choice(free, k, replace=False).tolist())
        t0 = lane % 17 if k > 2 else MANY_CLKS - 1 - lane % 4 if lane % 5 == 0 else (lane * 37) % (MANY_CLKS - 2)
        reads[lane] = {e: (t0 + 13 * r, 1 + (r + lane) % 3) for r, e in enumerate(at)}
    summary, ev = events(n, MANY_EVENT_CAP, RDLO, reads, seed=901 + spc[0])
    cfg = _abi.make_config(4, max_cycles=1 << 20, event_cap=MANY_EVENT_CAP, meas_cap=meas_cap, meas_latency=32, seed=0xC6,
                           p1=[0.5, 0.3, 0.6, 0.5],
                           demod=dict(drv_elem=RDRV, cpw=4, delay=7, theta=(0.7, 3.9), gain=(0.8, 0.6),
                                      axis=[0.3, 1.9, 4.0, 5.5], sigma=90.0, thr=0))
    cols = cols_for(lanes.tolist(), cores.tolist(), shots.tolist(), ((3 * np.arange(n) + 1) % 8).tolist(),
                    ((5 * np.arange(n) + 2) % 8).tolist(), spc)
    order, lines, k = rng.permutation(n).tolist(), [], 0
    while order:
        size = MANY_LINE_SIZES[k % len(MANY_LINE_SIZES)]
        lines.append(order[:size])
        order, k = order[size:], k + 1
    name = 'many_pairs_{}_{}'.format(*spc) + ('' if meas_cap == 32 else '_cap{}'.format(meas_cap))
    return Case(name, cfg, summary, ev, cols, lines, random_words(rng, (8, MANY_CLKS * spc[0])),
                random_words(rng, (8, MANY_CLKS * spc[1])), res_seed=305)


MANY = {'many_pairs_16_4': ((16, 4), 32), 'many_pairs_1_1': ((1, 1), 32), 'many_pairs_16_4_cap17': ((16, 4), 17),
        'many_pairs_1_1_cap17': ((1, 1), 17)}


CASES = dict([('scan_16_4', lambda: scan_case((16, 4))), ('scan_1_1', lambda: scan_case((1, 1)))]
             + [('full_range_' + w, functools.partial(full_range_case, w)) for w in FULL_RANGE]
             + [('clamp', clamp_case)] + [('edge_' + w, functools.partial(edge_case, w)) for w in EDGES]
             + [(k, functools.partial(many_pairs_case, *v)) for k, v in MANY.items()])


@functools.lru_cache(maxsize=None)
def case(name):
    return CASES[name]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """every reference output of a case, computed once per process and not to be modified: acc_iq / res_iq
    (dpemu_demod_iq), adc (dpemu_feedline_adc), adc_res (dpemu_feedline_adc_res with Case.resonators()), and
    (acc, result) of dpemu_demod_feedline on each of those traces and on the caller-made one: fl, fl_res, fl_in"""
    c = case(name)
    cfg, cols, mc = c.cfg, c.pt.cols, c.cfg.meas_cap
    out = {}
    out['acc_iq'], out['res_iq'] = demod_iq_ref.demod_iq(cfg, cols, c.summary, c.events, c.iq_drv, c.iq_lo, mc)
    out['adc'] = feedline_ref.feedline_adc(cfg, cols, c.lines, c.summary, c.events, c.iq_drv, c.n_lo, mc)
    tab, peak = c.resonators(), []
    out['adc_res'] = resonator_ref.feedline_adc_res(cfg, cols, c.lines, tab.coef, tab.adc_sigma, c.summary, c.events,
                                                    c.iq_drv, c.n_lo, mc, y_peak=peak)
    out['y_peak'] = peak[0]
    for key, adc in (('fl', out['adc']), ('fl_res', out['adc_res']), ('fl_in', c.adc_in)):
        if adc is not None:
            out[key] = feedline_ref.demod_feedline(cfg, cols, c.lines, c.summary, c.events, adc, c.iq_lo, mc)
    for v in out.values():
        for a in (v if isinstance(v, tuple) else (v,)):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return out


# ---- supplied states (the *_st entry points) on every case above ----

ST_PLANTED = (0, 0xFFFFFFFF, 0x80000000, 0x55555555)


def draws_read(name):
    """per lane, how many low bits of its state word the stages read: the kept readouts of the lane's pair, and 1
    for a pair without readouts (its resonator and its return take draw 0: include/dpemu.h)"""
    c = case(name)
    out = np.ones(c.summary.shape[0], np.int64)
    for p in range(c.pt.n_pairs):
        out[int(c.pt.cols['lane'][p])] = max(len(c.reads(p)), 1)
    return out


def packed_draws(name):
    """per lane the word whose bit m is the p1_threshold draw of its pair's readout m: the base calls' states"""
    from tests import qsim_meas_ref
    c = case(name)
    out = np.zeros(c.summary.shape[0], np.uint32)
    out[c.pt.cols['lane'].astype(np.int64)] = qsim_meas_ref.draw_words(c.cfg, c.pt.cols['shot'], c.pt.cols['core'])
    return out


@functools.lru_cache(maxsize=None)
def states_plan(name):
    """(words uint32 [n_lanes], {what: lanes}): full-range random words with, as far as the case has lanes for
    them, ST_PLANTED, words whose only set bits are at or above draws_read ('high_only': the results must be the
    all-zero word's) and, on a lane of 32 kept readouts, the packed draws with bits 2 and 31 (and random ones in
    between) flipped ('flipped')"""
    c = case(name)
    n = c.summary.shape[0]
    k = list(CASES).index(name)
    rng = np.random.default_rng(1600 + k)
    words, read = random_words(rng, n), draws_read(name)
    order = np.roll(rng.permutation(n), k).tolist()
    plan = {}
    full = [L for L in order if read[L] == 32][:1]
    for L in full:
        words[L] = packed_draws(name)[L] ^ np.uint32(0x80000004 | (int(rng.integers(0, 1 << 28)) << 3))
    plan['flipped'] = full
    high = [L for L in order if read[L] < 32 and L not in full][:max(1, min(6, n // 4))]
    for L in high:
        words[L] = np.uint32(((int(rng.integers(1, 2 ** 32)) | 1) << int(read[L])) & 0xFFFFFFFF)
    plan['high_only'] = high
    rest = [L for L in order if L not in full and L not in high]
    planted = ST_PLANTED[k % 4:] + ST_PLANTED[:k % 4]                 # a case of few lanes takes those it has room for
    for w, L in zip(planted, rest):
        words[L] = w
        plan[w] = [L]
    words.setflags(write=False)
    return words, plan


def states(name):
    return states_plan(name)[0]


def low_mask(read):
    return (0xFFFFFFFF >> (32 - np.asarray(read, np.int64))).astype(np.uint32)


def st_outputs(name, words):
    """the four *_st references of a case on per-lane state ``words``: adc, adc_res, traces (by_slot off, on: on
    test_traces.hb_trace_inputs' trace and bins), and (stats, bits) of iq_stats by slot on reference(name)['fl']"""
    from tests import qsim_meas_ref as mref, test_traces as T
    c, ref = case(name), reference(name)
    cfg, cols, mc = c.cfg, c.pt.cols, c.cfg.meas_cap
    tab = c.resonators()
    _, adc, n_bins, bin_clocks = T.hb_trace_inputs(name)
    acc, res = ref['fl']
    out = {'adc': mref.feedline_adc_st(words, cfg, cols, c.lines, c.summary, c.events, c.iq_drv, c.n_lo, mc),
           'adc_res': mref.feedline_adc_res_st(words, cfg, cols, c.lines, tab.coef, tab.adc_sigma, c.summary, c.events,
                                               c.iq_drv, c.n_lo, mc)}
    for by_slot in (False, True):
        out['traces', by_slot] = mref.feedline_traces_st(words, cfg, cols, c.lines, c.summary, c.events, adc, c.iq_lo, mc,
                                                         n_bins, bin_clocks, by_slot)
    out['stats'], out['bits'] = mref.iq_stats_st(np.asarray(words)[cols['lane'].astype(np.int64)], cfg, acc, res[:, 0],
                                                 core=cols['core'], shot=cols['shot'], by_slot=True)
    return out


@functools.lru_cache(maxsize=None)
def reference_st(name):
    """st_outputs on states(name), computed once per process and not to be modified"""
    out = st_outputs(name, states(name))
    for a in out.values():
        a.setflags(write=False)
    return out


# ---- D: saturating DDS tables ----

SATURATING_CASES = {   # (samples per clock, interp) of the four elements
    'cycle_interp1': ((16, 1), (16, 1), (16, 1), (16, 1)),
    'cycle_interp4': ((16, 4), (16, 4), (16, 4), (16, 4)),
    'quad_spc8': ((8, 1), (8, 4), (8, 8), (8, 16)),
    'quad_spc4': ((4, 1), (4, 4), (4, 8), (4, 16)),
    'generic_spc3': ((3, 1), (3, 4), (3, 2), (3, 16)),
    'generic_interp3': ((16, 3), (8, 3), (4, 3), (16, 3)),
}


def box_halves(rng, n, allow_min):
    """n int16 values drawn from {+-32767, 0, +-20000, random} and, with allow_min, -32768"""
    pool = np.array([32767, -32767, 0, 20000, -20000] + ([-32768] if allow_min else []))
    v = pool[rng.integers(0, len(pool), n)]
    return np.where(rng.random(n) < 0.2, rng.integers(-32767, 32768, n), v)


def saturating_case(name):
    """(desc, summary, events, env_tab, freq_tab, n_lanes, cap, n_samples) of test_gpu_dds.test_saturating_tables:
    test_sweep_edges' timelines with amp words from {0, 1, 65535, random} and env / rotation words whose halves
    come from box_halves -- I (the high half) down to -32768, Q never, so the Y-form sweeps stay eligible"""
    from tests.test_gpu_dds import synthetic_timelines
    rng = np.random.default_rng(1300 + list(SATURATING_CASES).index(name))
    cap, n_lanes, n_cycles, n_env = 48, 6, 2000, 301
    env_tab = ((box_halves(rng, n_env, True) & 0xFFFF) << 16 | (box_halves(rng, n_env, False) & 0xFFFF)).astype(np.uint32)
    freq_tab = np.concatenate([np.zeros(3, np.uint32)] + [DDSElementConfig(samples_per_clk=16).get_freq_buffer([f])
                              for f in (91.7e6, -13.1e6, 250e6)])
    rot = ((box_halves(rng, 48, True) & 0xFFFF) << 16 | (box_halves(rng, 48, False) & 0xFFFF)).astype(np.uint32)
    rot[[1, 16 + 2, 32 + 1]] |= 0x80000000                           # (words that every spc >= 3 plays)
    rot[[1, 16 + 2, 32 + 1]] &= 0x8000FFFF
    keep = np.arange(48) % 16 == 0                                   # word 0 of an entry is its frequency
    freq_tab[3:] = np.where(keep, freq_tab[3:], rot)
    summary, ev = synthetic_timelines(rng, n_lanes, cap, n_cycles, 280, 3)
    amp = np.array([0, 1, 65535, 65535])[rng.integers(0, 4, (cap, n_lanes))]
    ev[:, :, 3] = np.where(rng.random((cap, n_lanes)) < 0.3, rng.integers(0, 65536, (cap, n_lanes)), amp)
    desc = []
    for L in range(n_lanes):
        for e, (spc, interp) in enumerate(SATURATING_CASES[name]):
            desc.append((L, e, spc, interp, (0, 1, 5, 2)[e], (280, 279, 290, 301 - 2)[e], 3, len(freq_tab) - 3))
    desc = np.array(desc, np.uint32)
    n_samples = max(spc for spc, _ in SATURATING_CASES[name]) * n_cycles + 4 * 37
    return desc, summary, ev, env_tab, freq_tab, n_lanes, cap, n_samples


def dds_restated(desc, summary, ev, env_tab, freq_tab, n_samples, cap):
    """the rotate and mix lines of oracle/dds_ref.c in numpy, per channel: dict of played (bool [n]), the env and
    rotation words under every sample, rot (the unclamped rotation's two components, 0 where k == 0) and out (the
    output words).  Sample by sample for the pulse lookup, vectorised for the arithmetic."""
    import oracle
    lut = oracle.dds_sin_lut().astype(np.int64)
    res = []
    for lane, elem, spc, interp, env_off, env_len, freq_off, freq_len in np.asarray(desc, np.int64).tolist():
        n_ev = min(int(summary[lane, 2]), cap)
        j = np.arange(n_samples, dtype=np.int64)
        n, k = j // spc, j % spc
        t = ev[:n_ev, lane, 0].astype(np.int64)
        w1 = ev[:n_ev, lane, 1].astype(np.int64)
        # the cursor of dds_ref.c: the events before the first one with t > n have been applied
        cut = np.argmax(np.concatenate([t[None, :] > n[:, None], np.ones((n_samples, 1), bool)], axis=1), axis=1)
        is_st = (w1 >> 28 == 0) & ((w1 >> 24) & 3 == elem)
        is_rs = w1 >> 28 == 1
        idx = np.arange(n_ev)
        last_st = np.maximum.accumulate(np.where(is_st, idx, -1)) if n_ev else np.zeros(0, np.int64)
        last_rs = np.maximum.accumulate(np.where(is_rs, idx, -1)) if n_ev else np.zeros(0, np.int64)
        st = np.where(cut > 0, np.concatenate([[-1], last_st])[cut], -1)
        rs = np.where(cut > 0, np.concatenate([[-1], last_rs])[cut], -1)
        have = st >= 0
        s_ = np.maximum(st, 0)
        st_t, env_w = (t[s_], w1[s_] & 0xFFFFFF) if n_ev else (0 * j, 0 * j)
        pf, amp = (ev[:n_ev, lane, 2].astype(np.int64)[s_], ev[:n_ev, lane, 3].astype(np.int64)[s_] & 0xFFFF) if n_ev \
            else (0 * j, 0 * j)
        t_ref = np.where(rs >= 0, t[np.maximum(rs, 0)], 0) if n_ev else 0 * j
        A, L = env_w & 0xFFF, (env_w >> 12) & 0xFFF
        es = np.where(L > 0, ((j - st_t * spc) & 0xFFFFFFFF) // interp, 0)
        widx = 4 * A + es
        fi, phase = pf >> 17, pf & 0x1FFFF
        played = have & ((L == 0) | (es < 4 * L)) & (widx < env_len) & (16 * fi + 15 < freq_len)
        ew = env_tab.astype(np.int64)[np.where(played, env_off + widx, 0)]
        fbase = np.where(played, freq_off + 16 * fi, 0)
        f0, rw = freq_tab.astype(np.int64)[fbase], freq_tab.astype(np.int64)[fbase + k]
        theta = (f0 * ((n - t_ref) & 0xFFFFFFFF) + (phase << 15)) & 0xFFFFFFFF
        ti = theta >> 20
        a_i, a_q = (lut[(ti + 1024) & 4095] * amp + (1 << 15)) >> 16, (lut[ti] * amp + (1 << 15)) >> 16
        r_i, r_q = demod_iq_ref.s16(rw >> 16), demod_iq_ref.s16(rw)
        rot_i, rot_q = (a_i * r_i - a_q * r_q + (1 << 14)) >> 15, (a_i * r_q + a_q * r_i + (1 << 14)) >> 15
        b_i = np.where(k > 0, np.clip(rot_i, -32767, 32767), a_i)
        b_q = np.where(k > 0, np.clip(rot_q, -32767, 32767), a_q)
        e_i, e_q = demod_iq_ref.s16(ew >> 16), demod_iq_ref.s16(ew)
        o_i = np.clip((e_i * b_i - e_q * b_q + (1 << 14)) >> 15, -32768, 32767)
        o_q = np.clip((e_i * b_q + e_q * b_i + (1 << 14)) >> 15, -32768, 32767)
        out = np.where(played, (o_i & 0xFFFF) | ((o_q & 0xFFFF) << 16), 0).astype(np.uint32)
        rot_on = played & (k > 0)
        res.append(dict(played=played, env=ew, rotw=np.where(rot_on, rw, 0), rot_on=rot_on,
                        rot=(np.where(rot_on, rot_i, 0), np.where(rot_on, rot_q, 0)), out=out))
    return res
