"""Random distproc machine-code programs for differential testing.

Programs exercise every opcode class of hdl/ctrl.v: pulse write/trigger
(immediate and register-sourced fields), idle, pulse_reset, reg_alu (all 8
ALU ops, imm/reg forms), inc_qclk (all ALU ops via raw words), jump_i,
jump_cond (forward skips and bounded backward loops), alu_fproc/jump_fproc,
sync, done, hang opcodes, and late triggers.  A running qclk estimate keeps
most triggers in the future; the estimate only ever over-shoots, which is
safe (the core simply waits longer).

random_case draws every core's program independently, which above 8 or 16 cores
nearly always leaves some core astray (a skipped barrier, a read of a core that
never measures) and the shot in deadlock; wide_case writes the programs of a
shot of 16, 32 or 64 cores from one plan, so that barriers release, reads see
planned measurements and the meas_lut FSM fires.
"""

import random

import numpy as np

import distributed_processor_amd.isa as isa

ALU = ['id0', 'add', 'sub', 'eq', 'le', 'ge', 'id1', 'zero']


def raw(op4, in0_reg=0, alu_op=0, imm=0, rs0=0, rs1=0, rd=0, target=0, fproc_id=0, cmd_time=0):
    w = (((op4 << 4) | (in0_reg << 3) | alu_op) << 120)
    if in0_reg:
        w |= rs0 << 116
    else:
        w |= (imm & 0xFFFFFFFF) << 88
    w |= (rs1 & 15) << 84
    w |= (rd & 15) << 80
    w |= (target & 0xFFFF) << 68 if op4 in (2, 3, 5) else 0
    w |= (fproc_id & 0xFF) << 52 if op4 in (4, 5) else 0
    w |= (cmd_time & 0xFFFFFFFF) << 5 if op4 in (9, 12) else 0
    return w


class Gen:
    def __init__(self, rng, ncores, mode='meas', allow_late=False, allow_hang=False, meas_latency=20,
                 straight=False, linear=False, regs=None, late_from=0):
        self.late_from = late_from        # no late trigger / hang ending before this command index
        self.regs = list(regs) if regs else list(range(16))   # register indices the ALU / pulse fields name
        self.straight = straight          # pulse / idle / pulse_reset / done only
        self.linear = linear              # plus reg_alu / inc_qclk: no jump, fproc or sync
        self.shape = None                 # fixed opcode-kind sequence (shaped_case)
        self.rng = rng
        self.ncores = ncores
        self.mode = mode
        self.allow_late = allow_late
        self.allow_hang = allow_hang
        self.meas_latency = meas_latency

    def pulse_fields(self):
        r = self.rng
        f = dict(freq_word=r.randint(0, 511), phase_word=r.randint(0, 2 ** 17 - 1),
                 amp_word=r.randint(0, 2 ** 16 - 1), env_word=r.randint(0, 2 ** 24 - 1),
                 cfg_word=r.randint(0, 15))
        for k in list(f):
            if k != 'cfg_word' and r.random() < 0.25:
                del f[k]
        if r.random() < 0.2:
            k = r.choice(['freq', 'phase', 'amp', 'env'])
            f.pop(k + '_word', None)
            f[k + '_regaddr'] = r.randint(0, 15) if len(self.regs) == 16 else r.choice(self.regs)
        if r.random() < 0.1:
            f.pop('cfg_word', None)
        return f

    def block(self, words, q, n):
        """append ~n random instructions; returns the qclk estimate at the next decode"""
        r = self.rng
        i = 0
        while i < n:
            if self.shape is not None:
                kind = self.shape[i]
            else:
                kind = r.choices(['trig', 'pw', 'idle', 'prst', 'alu', 'incq', 'jc', 'ji', 'loop', 'fproc'],
                                 [10, 3, 2, 1, 0, 0, 0, 0, 0, 0] if self.straight else
                                 [10, 3, 2, 1, 6, 2, 0, 0, 0, 0] if self.linear else
                                 [10, 3, 2, 1, 6, 2, 2, 1, 1, 2])[0]
            if kind == 'trig':
                if self.allow_late and r.random() < 0.05 and len(words) >= self.late_from:
                    t = (q - r.randint(1, 4)) & 0xFFFFFFFF
                else:
                    t = (q + r.randint(0, 12)) & 0xFFFFFFFF
                words.append(isa.pulse_cmd(cmd_time=t, **self.pulse_fields()))
                q = (t + 3) & 0xFFFFFFFF
            elif kind == 'pw':
                words.append(isa.pulse_cmd(**self.pulse_fields()))
                q += 3
            elif kind == 'idle':
                t = (q + r.randint(0, 30)) & 0xFFFFFFFF
                words.append(isa.idle(t))
                q = (t + 3) & 0xFFFFFFFF
            elif kind == 'prst':
                words.append(isa.pulse_reset())
                q += 3
            elif kind == 'alu':
                op = r.randrange(8)
                # (the default register set draws exactly as before: same random streams)
                reg = (lambda: r.randint(0, 15)) if len(self.regs) == 16 else (lambda: r.choice(self.regs))
                dst = (lambda: r.randint(0, 7)) if len(self.regs) == 16 else (lambda: r.choice(self.regs))
                if r.random() < 0.5:
                    words.append(raw(1, 0, op, imm=r.choice([r.randint(-40, 40), r.getrandbits(32)]),
                                     rs1=reg(), rd=dst()))
                else:
                    words.append(raw(1, 1, op, rs0=reg(), rs1=reg(), rd=dst()))
                q += 4
            elif kind == 'incq':
                ops = [1, 1, 1, 0, 6, 7] + ([2] if self.allow_late and len(words) >= self.late_from else [])
                op = r.choice(ops)
                v = r.randint(-3, 40)
                words.append(raw(6, 0, op, imm=v))
                res = {1: v + q, 0: v, 6: q, 7: 0, 2: v - q}[op]
                q = (res + 4) & 0xFFFFFFFF
            elif kind == 'jc':
                skip = r.randint(1, 3)
                op = r.randrange(8)
                words.append(('jc', skip, op, r.randint(-3, 3), r.randint(0, 15)))
                q += 6
            elif kind == 'ji':
                words.append(('ji', r.randint(1, 2)))
                q += 4
            elif kind == 'loop':
                reg = r.randint(8, 15)
                cnt = r.randint(1, 4)
                words.append(raw(1, 0, 0, imm=cnt, rd=reg))                    # reg = cnt
                start = len(words)
                words.append(raw(1, 0, 1, imm=-1, rs1=reg, rd=reg))            # reg = -1 + reg
                body = r.randint(0, 2)
                for _ in range(body):
                    words.append(isa.pulse_cmd(**self.pulse_fields()))
                words.append(raw(3, 0, 4, imm=0, rs1=reg, target=start))       # if 0 < reg goto start
                self.loops.append((start - 1, len(words) - 1))
                q += 4 + cnt * (4 + 3 * body + 6)
            elif kind == 'fproc':
                op = r.randrange(8)
                if self.mode == 'meas':
                    fid = r.randrange(max(self.ncores, 1)) if r.random() < 0.9 else r.randint(0, 255)
                else:
                    fid = 0 if r.random() < 0.6 else r.randint(1, 3)
                in0r = r.random() < 0.3
                if r.random() < 0.5:
                    words.append(raw(4, int(in0r), op, imm=r.randint(-2, 2), rs0=r.randint(0, 15),
                                     rd=r.randint(0, 7), fproc_id=fid))
                    q += 6
                else:
                    words.append(('jf', r.randint(1, 2), op, int(in0r), r.randint(-2, 2), r.randint(0, 15), fid))
                    q += 8
                if self.mode == 'lut':
                    q += self.meas_latency + 400
            i += 1
        return q

    def program(self, n_sync, body_len):
        self.loops = []
        words = []
        q = 0
        for s in range(n_sync + 1):
            q = self.block(words, q, body_len)
            if s < n_sync:
                words.append(isa.sync(self.rng.randint(0, 255)))
                q = 1
        if self.allow_hang and self.rng.random() < 0.1 and len(words) >= self.late_from:
            words.append(raw(self.rng.choice([13, 14, 15])))
        else:
            words.append(isa.done_cmd() if self.rng.random() < 0.8 else 0)
        # resolve relative jumps (targets may point past the end: reads 0 = DONE)
        def fix(t):
            for a, b in self.loops:      # never jump into a loop's interior
                if a < t <= b:
                    return b + 1
            return t
        out = []
        for idx, w in enumerate(words):
            if isinstance(w, tuple):
                if w[0] == 'jc':
                    _, skip, op, imm, rs1 = w
                    out.append(raw(3, 0, op, imm=imm, rs1=rs1, target=fix(idx + 1 + skip)))
                elif w[0] == 'ji':
                    out.append(raw(2, target=fix(idx + 1 + w[1])))
                else:
                    _, skip, op, in0r, imm, rs0, fid = w
                    out.append(raw(5, in0r, op, imm=imm, rs0=rs0, target=fix(idx + 1 + skip), fproc_id=fid))
            else:
                out.append(w)
        return out


def pack_programs(progs):
    """list of word lists -> (words (n,4) u32, offsets, n_instr)"""
    offsets, n_instr, rows = [], [], []
    off = 0
    for p in progs:
        offsets.append(off)
        n_instr.append(len(p))
        rows.append(isa.words_to_u32(p))
        off += len(p)
    words = np.concatenate(rows) if rows else np.zeros((0, 4), np.uint32)
    return words, np.array(offsets, np.uint32), np.array(n_instr, np.uint32)


def random_case(seed, ncores=None, mode=None, allow_late=True, allow_hang=True, n_groups=None, straight=False,
                linear=False, regs=None, body=None, late_from=0):
    """body: commands per block, an int or a (lo, hi) range drawn per program
    (default: one draw from 3..14 for the whole case); late_from: Gen's"""
    rng = random.Random(seed)
    ncores = ncores or rng.choice([1, 2, 4])
    mode = mode or rng.choice(['meas', 'meas', 'lut'])
    n_groups = n_groups or rng.choice([1, 2])
    n_sync = 0 if (straight or linear) else (rng.choice([0, 0, 1, 2]) if ncores > 1 else rng.choice([0, 1]))
    g = Gen(rng, ncores, mode, allow_late, allow_hang, straight=straight, linear=linear, regs=regs,
            late_from=late_from)
    if body is None:
        body = rng.randint(3, 14)
    draw = (lambda: rng.randint(*body)) if isinstance(body, tuple) else (lambda: body)
    progs = [g.program(n_sync, draw()) for _ in range(n_groups * ncores)]
    table = np.arange(n_groups * ncores, dtype=np.uint32)
    return dict(ncores=ncores, mode=mode, n_groups=n_groups, progs=progs, table=table, rng=rng)


def shaped_case(seed, ncores, n_groups=4, allow_late=True, allow_hang=True, linear=False, length=None,
                late_from=0):
    """branch-free programs that share one opcode sequence with random
    parameters (cmd_times, pulse fields, ALU operands, late triggers) per
    (group, core), and a random final command: the batched-experiment shape
    whose lanes agree on the opcode at every step until their endings differ.
    linear: reg_alu / inc_qclk commands in the sequence too; length: commands
    before the final one (default: drawn from 3..16); late_from: Gen's"""
    rng = random.Random(seed)
    g = Gen(rng, ncores, 'meas', allow_late, allow_hang, straight=not linear, linear=linear, late_from=late_from)
    kinds, weights = (['trig', 'pw', 'idle', 'prst', 'alu', 'incq'], [10, 3, 2, 1, 6, 2]) if linear else \
        (['trig', 'pw', 'idle', 'prst'], [10, 3, 2, 1])
    g.shape = rng.choices(kinds, weights, k=length or rng.randint(3, 16))
    progs = [g.program(0, len(g.shape)) for _ in range(n_groups * ncores)]
    table = np.arange(n_groups * ncores, dtype=np.uint32)
    return dict(ncores=ncores, mode='meas', n_groups=n_groups, progs=progs, table=table, rng=rng)


def dead_tail_program():
    """two named registers up to `done`, then reg_alu on r3..r5 that never runs"""
    pulse = isa.pulse_i(freq_word=3, phase_word=0, amp_word=100, env_word=1 | (4 << 12), cfg_word=0, cmd_time=40)
    return [isa.reg_alu_i(7, 'id0', 0, 1), isa.reg_alu(1, 'add', 1, 2), pulse, isa.done_cmd(),
            isa.reg_alu(3, 'add', 4, 5), isa.reg_alu_i(1, 'sub', 5, 3), isa.done_cmd()]


BREAKERS = ('idle', 'pw', 'prst', 'incq', 'incq_neg')


def _per_program(v, n, scalar):
    """v as one value per program: a scalar (scalar(v) true) for all of them, or a sequence of n"""
    if scalar(v):
        return [v] * n
    assert len(v) == n
    return list(v)


def macro_shape_case(seed, ncores, n_groups, regs, macros, ops=range(8), rs_rate=0.5, breaks=(), late_at=(),
                     elem=None, gap=(0, 12)):
    """branch-free register programs written macro by macro (csrc/program_image.h
    build_macros): command 0 is a pulse_reset (macro 0, never MACRO_SIMPLE),
    every further macro 0-4 reg_alu and one pulse trigger, the last one `done`.
    An image macro holds 3 ALU slots when the programs name at most 2 registers
    (len(regs) <= 2), else 2, so a unit of more ALU commands than that spills
    into a macro with an absent pulse slot; positions below count image macros.

    regs: the registers rs0 / rs1 / rd and the register-sourced pulse fields name
    macros: image macros of every program (an int, or one per program), the
        terminal `done` macro included
    ops: the reg_alu ops drawn; half the reg_alu take an immediate
        (randint(-40, 40) or getrandbits(32)), half the register form of in0
    rs_rate: probability that one of env / phase / freq / amp of a trigger is
        register-sourced
    breaks: {macro position: breaker} (or one dict per program): 'idle', 'pw'
        (pulse write without trigger), 'prst' in place of the trigger; 'incq' /
        'incq_neg' an inc_qclk (by 0..40 / to 200..400 below zero: qclk wraps back
        through 2^32 that many cycles later) in the macro's first ALU slot
    late_at: macro positions (or one sequence per program) whose trigger gets a
        cmd_time 1-4 below the qclk of its decode
    elem: the cfg element bits of every trigger (readouts under meas_elem = elem)
    gap: (lo, hi) of the trigger's cmd_time above the qclk estimate (or one pair
        per program)

    The qclk estimate is exact here (command 0 decodes at cycle 0 and the next
    command at qclk 2), so a late_at trigger is late by 1-4 cycles."""
    rng = random.Random(seed)
    g = Gen(rng, ncores, 'meas', regs=regs)
    regs, ops = list(regs), list(ops)
    n_prog = n_groups * ncores
    slots = 3 if len(set(regs)) <= 2 else 2
    macros = _per_program(macros, n_prog, lambda v: isinstance(v, int))
    breaks = _per_program(breaks if breaks else {}, n_prog, lambda v: isinstance(v, dict))
    late_at = _per_program(tuple(late_at), n_prog, lambda v: not v or isinstance(v[0], int))
    gap = _per_program(gap, n_prog, lambda v: isinstance(v[0], int))

    def alu(words):
        op = rng.choice(ops)
        if rng.random() < 0.5:
            words.append(raw(1, 0, op, imm=rng.choice([rng.randint(-40, 40), rng.getrandbits(32)]),
                             rs1=rng.choice(regs), rd=rng.choice(regs)))
        else:
            words.append(raw(1, 1, op, rs0=rng.choice(regs), rs1=rng.choice(regs), rd=rng.choice(regs)))

    def fields():
        f = {k: v for k, v in g.pulse_fields().items() if not k.endswith('_regaddr')}
        if rng.random() < rs_rate:
            k = rng.choice(['env', 'phase', 'freq', 'amp'])
            f.pop(k + '_word', None)
            f[k + '_regaddr'] = rng.choice(regs)
        if elem is not None:
            f['cfg_word'] = (rng.randint(0, 3) << 2) | elem
        return f

    progs = []
    for pi in range(n_prog):
        M, brk, late, (g_lo, g_hi) = macros[pi], breaks[pi], set(late_at[pi]), gap[pi]
        assert M >= 2 and all(0 < p < M - 1 and b in BREAKERS for p, b in brk.items()) and \
            all(0 < p < M - 1 for p in late) and not late & set(brk)
        special = set(brk) | late
        words = [isa.pulse_reset()]
        q, m = 2, 1                     # qclk at the next decode; the image macro the next command opens
        while m < M - 1:
            b = brk.get(m)
            n = rng.randint(0, 4)
            if m in special or m + 1 in special or m + 1 == M - 1:
                n = min(n, slots)       # one macro: the unit ends in macro m
            if b in ('incq', 'incq_neg'):
                n = min(n, slots - 1)
                v = rng.randint(0, 40) if b == 'incq' else -(q + rng.randint(200, 400))
                words.append(raw(6, 0, 1, imm=v))
                q = (q + v + 4) & 0xFFFFFFFF
            for _ in range(n):
                alu(words)
                q = (q + 4) & 0xFFFFFFFF
            m += max(1, -(-n // slots)) if b not in ('incq', 'incq_neg') else 1
            if b == 'idle':
                t = (q + rng.randint(0, 30)) & 0xFFFFFFFF
                words.append(isa.idle(t))
                q = (t + 3) & 0xFFFFFFFF
            elif b == 'pw':
                words.append(isa.pulse_cmd(**fields()))
                q = (q + 3) & 0xFFFFFFFF
            elif b == 'prst':
                words.append(isa.pulse_reset())
                q = (q + 3) & 0xFFFFFFFF
            else:
                t = (q - rng.randint(1, 4) if m - 1 in late else q + rng.randint(g_lo, g_hi)) & 0xFFFFFFFF
                words.append(isa.pulse_cmd(cmd_time=t, **fields()))
                q = (t + 3) & 0xFFFFFFFF
        words.append(isa.done_cmd())
        progs.append(words)
    table = np.arange(n_prog, dtype=np.uint32)
    return dict(ncores=ncores, mode='meas', n_groups=n_groups, progs=progs, table=table, rng=rng)


# ---- wide shots that make progress ----

WIDE_OPS = {'jump': ((3, 1), (3, 0), (6, 0)),           # (alu op, immediate): eq 1, eq 0, id1
            'alu': ((6, 0), (1, 5), (3, 1), (3, 0))}    # id1, add 5, eq 1, eq 0


def wide_case(seed, ncores, n_groups, mode='meas', rounds=3, reads=2, block=2, meas_elem=2, drv_elem=None,
              ro_words=2, ro_clocks=8, sync_mask=0, lut_mask=0, quiet=(), skip=None, lut_rounds=None, short=False):
    """the programs of shots of 16, 32 or 64 cores that make progress: written core by core from one plan that
    all program groups share (the groups differ in every drawn parameter: times, pulse fields, register traffic).

    A program is a prelude and `rounds` rounds, each opened by a `sync`; in every stretch a core strobes a readout
    or not (the plan says which), all cores then idle until every readout of the stretch is valid, and read:

    * mode 'meas': up to `reads` alu_fproc / jump_fproc per core and stretch, each naming a core that has strobed
      a readout by then: in another 16-lane row or the other 32-lane half as often as not, and with an id at or
      above C (up to 255, the `& (C - 1)` wrap) one time in three;
    * mode 'lut': one read per core and stretch: id 0 right after the core's own strobe (its own next meas_valid),
      or a nonzero id before the stretch's fire.  The cores of `lut_mask` strobe in every stretch, after every
      other core's strobe, so the FSM fires once per stretch, at the last masked meas_valid (needs ro_clocks >= 8, with drv_elem 14).
      Cores in `quiet` never strobe: a lut_mask that names one never fires.  lut_rounds: the stretches (0 = the
      prelude) that may hold nonzero-id reads (default: all);
    * a jump_fproc skips a pulse pair or not, an alu_fproc writes a register of its own (r8..r15) that sources the
      amplitude of the next pulse: a wrong bit shows in the events.  plan['reads'] lists every read with what it
      must see, plan['base_events'] the events of a lane no jump of which skips anything;
    * before every sync each core idles for a random time, and plan['last'][k] idles past all others: the last
      arrival of barrier k, in each 16-lane row in turn;
    * cores outside `sync_mask` execute every sync and strobe only in the prelude (they end in DEADLOCK at the first
      sync); skip = {core: k}: the core leaves out sync k (k >= 1) and strobes only in the prelude: barrier k
      releases with the core's next sync, and the other participants end in DEADLOCK at the last one;
    * reg_alu on r0..r7 (any source register) and pulses with a register-sourced field run between the reads
      (`block` per stretch, drawn as Gen draws them, with a cfg word that is no readout).

    ro_words: the envelope length field of the readout strobes (the DEMOD window); ro_clocks: clocks from a
    readout strobe to its meas_valid (meas_latency; DEMOD: + ro_words * ro_cpw); drv_elem: a readout-drive
    strobe before every readout strobe (DEMOD).  short: 7-command programs (no prelude, one stretch with one read
    and one conditional pulse between two syncs) that fit the LDS staging of 16 and 32 cores."""
    rng = random.Random(seed)
    C, R = ncores, rounds
    g = Gen(rng, C, mode)
    part = [c for c in range(C) if not sync_mask or (sync_mask >> c) & 1]
    outside = [c for c in range(C) if c not in part]
    skip, quiet = dict(skip or {}), set(quiet)
    masked = [c for c in range(C) if (lut_mask >> c) & 1] if mode == 'lut' else []
    assert part and not set(skip) - set(part) and all(1 <= k <= R for k in skip.values())
    assert mode == 'meas' or (ro_clocks >= (14 if drv_elem is not None else 8) and not skip and
                              not set(masked) & set(outside))
    if short:
        assert mode == 'meas' and R == 2 and not skip and not outside
    lut_rounds = set(range(R + 1)) if lut_rounds is None else set(lut_rounds)
    rows = max(1, C // 16)
    safe = [e for e in range(4) if e != meas_elem]

    # -- the plan: who strobes in which stretch, who reads what, who arrives last --
    strobes, readplan, seen = [], [], set()
    for k in range(R + 1):
        if short and k != 1:
            strobes.append(set())
            readplan.append([[] for _ in range(C)])
            continue
        live = [c for c in range(C) if c not in quiet and (k == 0 or (c in part and c not in skip))]
        st = {c for c in live if c in masked or rng.random() < 0.75}
        for r in range(rows):                   # every 16-lane row strobes in every stretch
            cand = [c for c in live if c // 16 == r % rows]
            if cand and not st & set(cand):
                st.add(rng.choice(cand))
        strobes.append(st)
        seen |= st
        per_core = []
        for c in range(C):
            if k > 0 and c in outside:          # deadlocked at the first sync
                per_core.append([])
                continue
            rd = []
            if mode == 'meas':
                for _ in range(1 if short else rng.randint(0, reads)):
                    far = rng.random() < 0.6
                    pool = [t for t in sorted(seen) if (t // 16 != c // 16) == far] or sorted(seen)
                    t = rng.choice(pool)
                    fid = t + C * rng.randint(1, (255 - t) // C) if rng.random() < 0.34 else t
                    rd.append(dict(kind=rng.choice(['jump', 'alu']), fid=fid, target=t))
            else:
                own = c in st and (rng.random() < 0.4 or k not in lut_rounds)
                if own:
                    rd.append(dict(kind=rng.choice(['jump', 'alu']), fid=0, target=c))
                elif k in lut_rounds and rng.random() < 0.7:
                    rd.append(dict(kind=rng.choice(['jump', 'alu']), fid=rng.randint(1, 255), target=None))
            per_core.append(rd)
        readplan.append(per_core)
    steady = [c for c in part if c not in skip]
    last = [None] + [rng.choice([c for c in steady if c // 16 == (k + seed) % rows] or steady) for k in range(1, R + 1)]

    progs, base_events, reads_out, last_T = [], [], [], []
    for grp in range(n_groups):
        W = [[] for _ in range(C)]
        q = [0] * C
        ev = [0] * C
        n_strobed = [0] * C             # readouts strobed so far
        n_alu = [0] * C
        info = [[] for _ in range(C)]
        lt = [None]

        def fields(c):
            f = g.pulse_fields()
            f['cfg_word'] = (rng.randint(0, 3) << 2) | rng.choice(safe)
            return f

        def trig(c, lo=0, hi=12, **f):
            t = q[c] + rng.randint(lo, hi)
            W[c].append(isa.pulse_cmd(cmd_time=t, **f))
            q[c] = t + 3
            ev[c] += 1
            return t

        def blk(c, n):
            for _ in range(n):
                kind = rng.choices(['trig', 'pw', 'alu'], [5, 1, 4])[0]
                if kind == 'trig':
                    trig(c, **fields(c))
                elif kind == 'pw':
                    W[c].append(isa.pulse_cmd(**fields(c)))
                    q[c] += 3
                else:
                    op = rng.randrange(8)
                    if rng.random() < 0.5:
                        W[c].append(raw(1, 0, op, imm=rng.choice([rng.randint(-40, 40), rng.getrandbits(32)]),
                                        rs1=rng.randint(0, 15), rd=rng.randint(0, 7)))
                    else:
                        W[c].append(raw(1, 1, op, rs0=rng.randint(0, 15), rs1=rng.randint(0, 15), rd=rng.randint(0, 7)))
                    q[c] += 4

        def readout(c, t_lo=None):
            """a readout strobe at t_lo + [0, 10] (without a drive strobe: + [0, 4]); -> its cmd_time"""
            if t_lo is not None:
                assert q[c] <= t_lo
                q[c] = t_lo
            if drv_elem is not None:
                trig(c, 0, 3, freq_word=rng.randint(0, 511), phase_word=rng.randint(0, 2 ** 17 - 1),
                     amp_word=rng.randint(0, 2 ** 16 - 1), env_word=rng.randint(0, 4095) | (ro_words << 12),
                     cfg_word=(rng.randint(0, 3) << 2) | drv_elem)
            t = trig(c, 0, 4, freq_word=rng.randint(0, 511), phase_word=rng.randint(0, 2 ** 17 - 1),
                     amp_word=rng.randint(0, 2 ** 16 - 1), env_word=rng.randint(0, 4095) | (ro_words << 12),
                     cfg_word=(rng.randint(0, 3) << 2) | meas_elem)
            n_strobed[c] += 1
            return t

        def read(c, k, rd, m, cost):
            """the read, and what it switches; m: the target's measurement the read sees (None: not planned)"""
            op, imm = rng.choice(WIDE_OPS[rd['kind']])
            rec = dict(rd, core=c, round=k, op=op, imm=imm, m=m, group=grp)
            if rd['kind'] == 'jump':
                n = 1 if short else 2
                W[c].append(raw(5, 0, op, imm=imm, target=len(W[c]) + 1 + n, fproc_id=rd['fid']))
                q[c] = cost(q[c] + 8)
                for _ in range(n):      # (base_events counts the pulses a taken jump skips)
                    trig(c, 0, 6, **fields(c))
                rec['skips'] = n
            else:
                reg = 8 + n_alu[c] % 8
                n_alu[c] += 1
                assert n_alu[c] <= 8
                W[c].append(raw(4, 0, op, imm=imm, rd=reg, fproc_id=rd['fid']))
                q[c] = cost(q[c] + 6)
                f = {k_: v for k_, v in fields(c).items() if not k_.endswith('_regaddr')}
                f.pop('amp_word', None)
                trig(c, 0, 6, amp_regaddr=reg, **f)
                rec['rd'] = reg
            info[c].append(rec)

        for k in range(R + 1):
            if short and k == 0:
                continue
            if k == 0:
                for c in range(C):
                    W[c].append(isa.pulse_reset())
                    q[c], ev[c] = 3, 1
                    blk(c, rng.randint(0, block))
            else:
                # arrival: every core at a time of its own, the planned core past all others
                for c in range(C):
                    if c in outside and k > 1:
                        continue
                    if c != last[k] and not short:
                        t = q[c] + rng.randint(0, 40)
                        W[c].append(isa.idle(t))
                        q[c] = t + 3
                t = max(q) + rng.randint(8, 30)
                W[last[k]].append(isa.idle(t))
                lt.append(t)
                for c in range(C):
                    if c in outside and k > 1:
                        continue
                    if skip.get(c) == k:
                        continue        # no sync: the core's qclk runs on
                    W[c].append(isa.sync(rng.randint(0, 255)))
                    q[c] = 1
            act = [c for c in range(C) if not (c in outside and k > 0)]
            if short and k == 2:
                break
            off = {c: skip[c] <= k for c in skip}      # a core that has left out a sync runs at a time of its own
            if mode == 'meas':
                # a strobe at qclk t is valid at t + 2 + ro_clocks; the command after idle(T) decodes at T + 3
                tmax = max([readout(c) for c in act if c in strobes[k]], default=0)
                T = max(max(q[c] for c in act), tmax + ro_clocks)
                for c in act:
                    W[c].append(isa.idle(T))
                    q[c] = T + 3
                    for rd in readplan[k][c]:
                        read(c, k, rd, None if off.get(c) else n_strobed[rd['target']] - 1, lambda x: x)
                    if not short:
                        blk(c, rng.randint(0, block))
            else:
                # strobes of the other cores in [A + 3, A + 13], valid by A + 15 + ro_clocks; of the masked cores in
                # [A + 16, A + 26], the fire at the last of their meas_valid in [A + 18, A + 28] + ro_clocks; a
                # masked core's own read decodes by A + 29 (A + 23 without a drive strobe), before the fire
                A = max(q[c] for c in act) + 8
                for c in act:
                    W[c].append(isa.idle(A))
                    q[c] = A + 3
                fire_by = A + 28 + ro_clocks
                for c in act:
                    if c in strobes[k]:
                        readout(c, A + 16 if c in masked else A + 3)
                    for rd in readplan[k][c]:
                        if rd['fid'] == 0:
                            read(c, k, rd, n_strobed[c] - 1, lambda x, c=c: q[c] + 2 + ro_clocks + 6)
                        else:
                            read(c, k, dict(rd, fire=k), None, lambda x: fire_by + 6)
                for c in act:
                    q[c] = max(q[c], fire_by + 8)
                    blk(c, rng.randint(0, block))
        for c in range(C):
            W[c].append(isa.done_cmd())
        progs += W
        base_events.append(ev)
        reads_out += [r for c in range(C) for r in info[c]]
        last_T.append(lt)
    table = np.arange(n_groups * C, dtype=np.uint32)
    plan = dict(strobes=strobes, last=last, last_T=last_T, reads=reads_out, base_events=base_events, part=part,
                outside=outside, skip=skip, masked=masked, rounds=R)
    return dict(ncores=C, mode=mode, n_groups=n_groups, progs=progs, table=table, rng=rng, plan=plan)
