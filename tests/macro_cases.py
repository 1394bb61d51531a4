"""Programs and launch shapes that send csrc/macro.hip down each of its
wave-uniform paths with the register trace OFF: the lean chunk
(lean_chunk_ok), the lean macro (lean_ok), the simple macro (simple_ok), the
batched slots (alu_step / pulse_step) and the general slots.  Not test code of
its own: tests/test_macro_cases.py asserts on the CPU (the image tool of
tests/test_program_image.py, the plan tool of tests/test_launch_plan.py, a
timing model and oracle_fast) that every case reaches the path, the kernel and
the lane endings it was chosen for; tests/test_gpu_macro_paths.py holds the
kernels to oracle_fast on the same cases.

A case names its tests/progfuzz.py macro_shape_case call, the cores per shot C,
the program groups, shots_per_group, the run's shots and first shot, the lane
order, the caps, meas_elem, whether the run asks for the `trace` output, and
the kernel name a run of it must report (dpemu_last_kernel, `,addid` kept).
The trace is off either by trace_cap = 0 or by a run that does not request the
`trace` output under trace_cap > 0: both clear MacroLane::tr_on.

Families:
 F  every program of a case has the same macro count M and every macro >= 1 is
    MACRO_SIMPLE: whatever programs a wave holds, every wave with a running
    lane passes lean_chunk_ok (2 registers) or simple_ok (3) in every chunk
    that does not hold the terminal macro, while max_cycles is loose
 G  mixed: one breaker (idle, pulse write, pulse reset, inc_qclk) in an
    otherwise simple program of one wave-uniform run (g_single_*), and fuzzed
    sets with unequal lengths, breakers and late triggers (g_fuzz_*)
 H  two programs swept over a stride-1 window of max_cycles across the values
    at which lean_chunk_ok (2 registers) / simple_ok (3) change their verdict"""

import functools
import random

from distributed_processor_amd import _abi
from distributed_processor_amd.emulator import ProgramSet
from tests.progfuzz import BREAKERS, macro_shape_case

BLOCK, CHUNK = 256, 16                  # csrc/uop.h BLOCK, MACRO_CHUNK
NO_TRACE = ('summary', 'events', 'meas', 'regs', 'hist')
ALL_OUT = ('summary', 'events', 'trace', 'meas', 'regs', 'hist')
CAP0 = dict(max_cycles=6000, event_cap=96, trace_cap=0, meas_cap=16)        # trace off: no trace rows at all
UNASKED = dict(CAP0, trace_cap=16)                                          # ... or rows nobody asks for


def kernel_name(C, n_groups, spg, order, n_regs, addid=False, direct=False):
    """csrc/launch_plan.h's choice for a macro image, restated (tests/test_launch_plan.py checks it)"""
    shots_run = max(1, 64 // C) if order else min(BLOCK // C, 64)
    cores_w = min(C, 64) if order else 64 // shots_run
    need = (1 if n_groups == 1 else min(n_groups, -(-(shots_run - 1) // spg) + 1)) * cores_w
    nr = 2 if n_regs <= 2 else 16
    if direct or need > 12 or (need > 8 and nr != 2):
        return 'macro_kernel'
    return 'macro_staged_kernel<{}{}{}>'.format(nr, ',addid' if addid else '', ',12' if need > 8 else '')


class Case:
    def __init__(self, name, family, gen, C, n_groups, spg, n_shots, shot0, order=0, caps=CAP0, outputs=None,
                 meas_elem=2, seed=1, addid=False, M=None, reach=()):
        self.name, self.family = name, family
        self.gen = dict(gen)                # macro_shape_case's keyword arguments (ncores / n_groups added)
        self.C, self.n_groups, self.spg = C, n_groups, spg
        self.n_shots, self.shot0, self.order = n_shots, shot0, order
        self.caps = dict(caps)
        self.outputs = tuple(outputs) if outputs else NO_TRACE      # no `trace` unless the case asks for it
        self.trace_on = 'trace' in self.outputs and self.caps['trace_cap'] > 0
        self.meas_elem, self.seed = meas_elem, seed
        self.n_regs = len(set(self.gen['regs']))
        self.addid = addid                  # every ALU op of the image is id0 / add
        self.kernel = kernel_name(C, n_groups, spg, order, self.n_regs, addid)
        self.M = M                          # family F: the macro count of every program
        self.reach = tuple(reach)

    def __repr__(self):
        return self.name


def _g(seed, regs, macros, **kw):
    return dict(seed=seed, regs=regs, macros=macros, **kw)


VG, ONE, LDS3 = (2, 9), (5,), (1, 4, 7)

FAMILY_F = [
    # M = 33: the terminal macro alone in the last chunk; 48: the last full chunk holds it; 47
    Case('f_vgpr_33', 'F', _g(501, VG, 33), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 77, shot0=0, M=33),
    Case('f_vgpr_48', 'F', _g(502, VG, 48), C=2, n_groups=9, spg=10, n_shots=64 * 5 + 13, shot0=25, order=1,
         caps=UNASKED, M=48),
    Case('f_vgpr_47', 'F', _g(503, VG, 47), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 40, shot0=7, caps=UNASKED,
         M=47),
    Case('f_one_reg_c1', 'F', _g(504, ONE, 52), C=1, n_groups=9, spg=10, n_shots=256 + 99, shot0=3, M=52),
    Case('f_one_reg_c4', 'F', _g(505, ONE, 49), C=4, n_groups=6, spg=10, n_shots=64 * 4 + 21, shot0=12, order=1,
         caps=UNASKED, M=49),
    Case('f_lds', 'F', _g(506, LDS3, 52), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 77, shot0=5, M=52),
    # 4 shots per group: a core-major wave of 64 shots spans 13 programs and more, past the wide slots
    Case('f_spg4', 'F', _g(507, VG, 50), C=2, n_groups=13, spg=4, n_shots=128 * 2 + 50, shot0=9, caps=UNASKED,
         M=50),
    Case('f_addid_wide', 'F', _g(508, VG, 56, ops=(0, 1), rs_rate=1.0), C=2, n_groups=9, spg=10,
         n_shots=128 * 2 + 77, shot0=11, addid=True, M=56),
    Case('f_addid_wide_shot', 'F', _g(509, VG, 56, ops=(0, 1), rs_rate=1.0), C=2, n_groups=9, spg=10,
         n_shots=64 * 5 + 13, shot0=11, order=1, caps=UNASKED, addid=True, M=56),
    # every trigger a readout: n_meas passes 32 and both caps overflow by counts that advanced in lean chunks
    Case('f_meas', 'F', _g(510, VG, 64, elem=2), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 77, shot0=0,
         caps=dict(CAP0, event_cap=5, meas_cap=4), M=64, reach=('meas',)),
    # a late trigger at macro 37 (chunk 2) of every second program
    Case('f_late', 'F', _g(511, VG, 64, late_at=[(37,) if i % 2 else () for i in range(18)]), C=2, n_groups=9,
         spg=10, n_shots=64 * 5 + 13, shot0=4, order=1, M=64, reach=('late',)),
    # 276 shots from shot 34 (group 3): the last workgroup holds 20 shots -- per core one wave with 20
    # valid lanes and one with none
    Case('f_partial', 'F', _g(501, VG, 33), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 20, shot0=34, caps=UNASKED,
         M=33, reach=('partial',)),
]
# the same programs with the register trace requested: the slot paths (alu_step / pulse_step)
TRACE_TWINS = {'f_trace_on_vgpr': 'f_vgpr_33', 'f_trace_on_lds': 'f_lds'}
FAMILY_F += [
    Case('f_trace_on_vgpr', 'F', _g(501, VG, 33), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 77, shot0=0,
         caps=dict(CAP0, trace_cap=16), outputs=ALL_OUT, M=33),
    Case('f_trace_on_lds', 'F', _g(506, LDS3, 52), C=2, n_groups=9, spg=10, n_shots=128 * 2 + 77, shot0=5,
         caps=dict(CAP0, trace_cap=16), outputs=ALL_OUT, M=52),
]

# one program, one group, C = 1: every lane of every wave holds the same macros.  80 macros: chunks 0
# (macro 0) and 4 (terminal) are MIXED by construction, 1 and 3 lean, 2 holds the breaker at macro 37
G_BREAK_AT = 2 * CHUNK + 5
FAMILY_G_SINGLE = [
    Case('g_single_{}{}'.format(b, '_lds' if regs is LDS3 else ''), 'G',
         _g(600 + 10 * i + len(regs), regs, 80, breaks={G_BREAK_AT: b}), C=1, n_groups=1, spg=1, n_shots=256 + 70,
         shot0=i, caps=UNASKED if i % 2 else CAP0, M=80)
    for i, b in enumerate(BREAKERS) for regs in (VG, LDS3)
]


def _fuzz_case(seed):
    rr = random.Random(7000 + seed)
    C = [1, 2, 4][seed % 3]
    order = (seed // 2) % 2
    spg = [5, 10, 16, 32][seed % 4]
    n_groups = rr.randint(9, 12) if spg == 5 else rr.randint(6, 12)     # spg 5: 9-12 programs per wave, the wide slots
    regs = tuple(rr.sample(range(16), 1 + seed % 4))
    macros = [rr.randint(20, 80) for _ in range(n_groups * C)]
    breaks, late = [], []
    for M in macros:
        b = {p: rr.choice(BREAKERS) for p in range(1, M - 1) if rr.random() < 1 / 24}
        breaks.append(b)
        late.append(tuple(p for p in range(1, M - 1) if p not in b and rr.random() < 1 / 40))
    caps = dict(UNASKED if seed % 4 < 2 else CAP0)
    if seed % 2:                            # tight caps on half
        caps.update(max_cycles=350 + 90 * seed, event_cap=3, meas_cap=1)
    return Case('g_fuzz_{}'.format(seed), 'G', _g(700 + seed, regs, macros, breaks=breaks, late_at=late), C=C,
                n_groups=n_groups, spg=spg, n_shots=256 + 64 * (seed % 5) + 7 * seed, shot0=seed * 31, order=order,
                caps=caps, meas_elem=seed % 4, seed=seed)


FAMILY_G_FUZZ = [_fuzz_case(seed) for seed in range(8)]
FAMILY_G = FAMILY_G_SINGLE + FAMILY_G_FUZZ

# the bound: two programs of 50 macros with different trigger spacing, one group; H_WINDOW consecutive
# max_cycles values from the start tests/test_macro_cases.py computes (h_window)
H_WINDOW, H_TWIN_WINDOW = 400, 64
H_GAPS = [(0, 3), (2, 8)]
FAMILY_H = [
    Case('h_vgpr', 'H', _g(801, VG, 50, gap=H_GAPS), C=2, n_groups=1, spg=1, n_shots=256, shot0=0, M=50),
    Case('h_vgpr_shot', 'H', _g(801, VG, 50, gap=H_GAPS), C=2, n_groups=1, spg=1, n_shots=256, shot0=0, order=1, M=50),
    Case('h_lds', 'H', _g(802, LDS3, 50, gap=H_GAPS), C=2, n_groups=1, spg=1, n_shots=256, shot0=0, M=50),
    Case('h_lds_shot', 'H', _g(802, LDS3, 50, gap=H_GAPS), C=2, n_groups=1, spg=1, n_shots=256, shot0=0, order=1,
         M=50),
    # beyond the 50 macros: with 80, max_cycles at the bound of chunk c stops the lanes inside chunks c + 1
    # and c + 2, which are lean-chunk candidates themselves (the window spans every bound, +- 40)
    Case('h_vgpr_80_shot', 'H', _g(803, VG, 80, gap=H_GAPS), C=2, n_groups=1, spg=1, n_shots=256, shot0=0, order=1,
         M=80),
]

ALL = FAMILY_F + FAMILY_G + FAMILY_H
BY_NAME = {c.name: c for c in ALL}
assert len(BY_NAME) == len(ALL)


@functools.lru_cache(maxsize=None)
def _built(name):
    c = BY_NAME[name]
    fz = macro_shape_case(ncores=c.C, n_groups=c.n_groups, **c.gen)
    groups = [[fz['progs'][fz['table'][g * c.C + k]] for k in range(c.C)] for g in range(c.n_groups)]
    return fz, ProgramSet(groups, cores_per_shot=c.C)


def fuzz_case(c):
    """the case's macro_shape_case result (the programs as word lists), built once"""
    return _built(c.name)[0]


def program_set(c):
    return _built(c.name)[1]


def config(c, **over):
    """a fresh dpemu config of the case"""
    kw = dict(n_groups=c.n_groups, shots_per_group=c.spg, meas_latency=3 + c.seed % 20, seed=c.seed,
              lane_order=c.order, meas_elem=c.meas_elem, **c.caps)
    kw.update(over)
    return _abi.make_config(c.C, **kw)


# ---- the timing of a branch-free program (hdl/ctrl.v's decode-to-decode latencies), for the CPU checks
def op4(w):
    return (w >> 124) & 15


def macros_of(words, slots):
    """csrc/program_image.h build_macros restated: per image macro ([ALU command indices], pulse-slot
    command index or None), up to the first terminal command"""
    out, k = [], 0
    while True:
        alus = []
        while len(alus) < slots and op4(words[k]) in (1, 6):
            alus.append(k)
            k += 1
        slot = None
        if op4(words[k]) not in (1, 6):
            slot = k
            k += 1
        out.append((alus, slot))
        if slot is not None and op4(words[slot]) in (0x0, 0xA, 0xD, 0xE, 0xF):
            return out


def timing(words):
    """per command of a branch-free program run without a max_cycles stop: (decode cycle D, the qclk
    anchor (qa_t, qa_q) at D, the cycle tT at which a trigger / idle fires or None, late).  reg_alu
    D + 4; inc_qclk (immediate add) reloads qclk to imm + qclk(D) + 3 at D + 3, next decode D + 4; a
    trigger or idle fires at tT = max(D, the cycle of its cmd_time) -- in the reset hold (D < qa_t)
    at D for cmd_time 0 -- and the next decode is tT + 3; late: the cmd_time is behind qclk(D), the
    core never fires.  The list ends at a late command or the terminal one."""
    out = []
    D, qa_t, qa_q = 0, 1, 0
    for w in words:
        o = op4(w)
        qD = 0 if D < qa_t else (qa_q + D - qa_t) & 0xFFFFFFFF
        tT, late = None, False
        nD = None
        if o == 1:
            nD = D + 4
        elif o == 6:
            assert (w >> 120) & 15 == 1, 'inc_qclk: immediate add only'
            imm = (w >> 88) & 0xFFFFFFFF
            nD, n_qa = D + 4, (D + 3, (imm + qD + 3) & 0xFFFFFFFF)
        elif o in (0x8, 0xB):
            nD = D + 3
        elif o in (0x9, 0xC):
            T = (w >> 5) & 0xFFFFFFFF
            if D < qa_t:
                tT = D if T == 0 else qa_t + ((T - qa_q) & 0xFFFFFFFF)
            else:
                tT = D + ((T - qD) & 0xFFFFFFFF)
            late = tT - D >= 1 << 31
            nD = tT + 3
        out.append((D, (qa_t, qa_q), tT, late))
        if nD is None or late:
            return out
        if o == 6:
            qa_t, qa_q = n_qa
        D = nD
    raise AssertionError('no terminal command')


def lean_bounds(words):
    """per chunk of a 2-register program: (decode cycle of the chunk's first command, qclk anchor there,
    the smallest max_cycles at which macro.hip lean_chunk_ok passes the lane, or None for a MIXED
    chunk).  A chunk is MIXED when it holds macro 0, the terminal macro or a macro that is not
    MACRO_SIMPLE; else B = max(decode of its first command, cycle of its largest cmd_time + 3) and
    lean_chunk_ok asks B + 16 CHUNK + 8 <= max_cycles.  Chunks behind a late trigger are left out."""
    mac, tm = macros_of(words, 3), timing(words)
    out = []
    for c in range(-(-len(mac) // CHUNK)):
        first = (mac[c * CHUNK][0] + [mac[c * CHUNK][1]])[0]
        if first >= len(tm) or any(t[3] for t in tm[:first]):
            break
        D, (qa_t, qa_q), _, _ = tm[first]
        bound = None
        if lean_candidate(words, mac, c):
            trig = [(words[s] >> 5) & 0xFFFFFFFF for _, s in mac[c * CHUNK:(c + 1) * CHUNK] if s is not None]
            tc = (max(trig) if trig else 0) + qa_t
            bound = max(D, tc - qa_q + 3 if tc > qa_q else 0) + 16 * CHUNK + 8
        out.append((D, (qa_t, qa_q), bound))
    return out


def lean_chunk_verdicts(words, max_cycles):
    """macro.hip lean_chunk_ok restated for one lane of the program: {chunk the lane enters running:
    verdict} (decode times only grow, so a lane whose chunk starts within max_cycles was not stopped
    before it); the verdict also needs that qclk cannot wrap before max_cycles"""
    out = {}
    for c, (D, (qa_t, qa_q), bound) in enumerate(lean_bounds(words)):
        if D > max_cycles:
            break
        out[c] = bound is not None and qa_q + max_cycles < (1 << 32) + qa_t and bound <= max_cycles
    return out


def macro_verdict(words, j, max_cycles, slots):
    """macro.hip simple_ok (3 registers: two ALU slots, SPAN = 8) / lean_ok (2 registers: three slots,
    SPAN = 12) for one lane entering macro j running: the macro is MACRO_SIMPLE-shaped and decodes
    at t with t + SPAN <= max_cycles"""
    mac, tm = macros_of(words, slots), timing(words)
    first = (mac[j][0] + [mac[j][1]])[0]
    return is_simple(words, mac, j) and tm[first][0] + 4 * slots <= max_cycles


def h_window(c):
    """family H, 2 registers: the first max_cycles of the lean-chunk sweep and its length, H_WINDOW
    values (more where the bounds span more: 40 to either side) placed so that the lean-chunk bounds
    of every lean chunk of both programs lie strictly inside"""
    flips = [b for w in fuzz_case(c)['progs'] for _, _, b in lean_bounds(w) if b is not None]
    n = max(H_WINDOW, max(flips) - min(flips) + 80)
    return min(flips) - (n - (max(flips) - min(flips))) // 2, n


def h_macro_window(c):
    """family H: H_TWIN_WINDOW values of max_cycles around t + SPAN of macros 30 and 31 of program 0, the
    per-macro tests (simple_ok with 3 registers, SPAN = 8; lean_ok with 2, SPAN = 12: below every
    lean-chunk bound, so the chunks run macro by macro)"""
    slots = 3 if c.n_regs <= 2 else 2
    w = fuzz_case(c)['progs'][0]
    mac, tm = macros_of(w, slots), timing(w)
    t30 = tm[(mac[30][0] + [mac[30][1]])[0]][0]
    return t30 + 4 * slots - 16, H_TWIN_WINDOW


def lean_candidate(words, mac, c):
    """csrc/program_image.h mark_lean_chunks: chunk c does not reach the terminal macro and every macro
    of it is MACRO_SIMPLE.  (Its marker is the largest cmd_time, so a chunk whose largest cmd_time is
    0xFFFFFFFF reads as MACRO_CHUNK_MIXED: it takes the per-macro tests, which is always allowed.)"""
    if (c + 1) * CHUNK >= len(mac) or not all(is_simple(words, mac, j) for j in range(c * CHUNK, (c + 1) * CHUNK)):
        return False
    return max([(words[s] >> 5) & 0xFFFFFFFF for _, s in mac[c * CHUNK:(c + 1) * CHUNK] if s is not None] + [0]) \
        != 0xFFFFFFFF


def is_simple(words, mac, j):
    """MACRO_SIMPLE (csrc/uop.h): not the first macro, reg_alu ALU slots, a trigger or no pulse slot"""
    alus, slot = mac[j]
    return j != 0 and all(op4(words[k]) == 1 for k in alus) and (slot is None or op4(words[slot]) == 0x9)
