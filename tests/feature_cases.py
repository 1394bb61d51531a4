"""Program sets with an exact feature set, one per instantiation of
branch_kernel<FEAT, CT> and interp_kernel<F> (csrc/branch_kernel.h,
csrc/interp.hip), and the helpers the tests of those kernels share.

The kernel choice (csrc/launch_plan.h plan_run) reads five facts of the loaded
programs (csrc/program_image.h): has_fproc, has_sync, reg_writes, straight and
linear.  progfuzz.random_case nearly always writes a register and mixes fproc
reads and syncs as its seed falls, so a fuzz corpus asks for the instantiations
it happens to ask for.  Here a case is rewritten, command for command (jump
targets stay valid), until its facts are exactly the requested ones:

* no register writes: without_register_writes;
* no fproc: without_fproc (alu_fproc -> reg_alu, jump_fproc -> jump_cond);
* no sync: without_sync (sync -> the inc_qclk that leaves qclk as the release would);
* a feature that must be present comes with the seed; nothing is inserted.

INSTANTIATIONS is the one table of rows.  tests/test_feature_cases.py checks
on the CPU that every row plans exactly the kernel it claims
(tests/instantiation_plan_test.cpp), that the rows are exactly the kernels
libdpemu.so holds, and that every row reaches the code its feature bits switch;
tests/test_gpu_instantiations.py runs every row against oracle_fast.

Out of scope: straight_kernel and the macro kernels.  tests/test_gpu_staging.py
and tests/test_gpu_macro_paths.py assert their names case by case, and their
large-grid fb1 variants need grids of more than a thousand workgroups, which a
row of a few hundred lanes cannot ask for."""

import collections
import functools
import random
import re

import numpy as np

from distributed_processor_amd import _abi, isa
from distributed_processor_amd.emulator import ProgramSet, alloc_device_outputs
from tests import qsim_meas_ref as mref
from tests.progfuzz import random_case, raw

FEAT_FPROC, FEAT_SYNC, FEAT_LUT, FEAT_PROG_LDS, FEAT_STRAIGHT, FEAT_REGS, FEAT_DEMOD, FEAT_STATES = \
    1, 2, 4, 8, 16, 32, 64, 128
MODEL_BIT = {'state': 0, 'demod': FEAT_DEMOD, 'states': FEAT_STATES}
CM, SM = _abi.LANES_CORE_MAJOR, _abi.LANES_SHOT_MAJOR
SEED_A, SEED_B = 0xA11CE5EED, 0xB0B5EED00F
ALL_OUT = ('summary', 'events', 'trace', 'meas', 'regs', 'hist')


# ---- rewriting commands ----

def without_register_writes(progs):
    """the programs with every reg_alu a pulse_reset and every alu_fproc a jump_fproc to the next command:
    no command writes the reg_file (FEAT_REGS off), the fproc reads and their waits stay"""
    out = []
    for p in progs:
        q = []
        for i, w in enumerate(p):
            d = isa.decode(w)
            if d['op'] == 'reg_alu':
                w = isa.pulse_reset()
            elif d['op'] == 'alu_fproc':
                w = raw(5, d['in0_reg'], isa.ALU_OPS[d['alu_op']], imm=d['imm'], rs0=d['rs0'], target=i + 1,
                        fproc_id=d['fproc_id'])
            q.append(w)
        out.append(q)
    return out


def without_fproc(progs):
    """the programs with every alu_fproc a reg_alu (same op, in0 and rd; in1 is reg[rs1] in place of the fproc
    data) and every jump_fproc a jump_cond (same op, in0 and target): nothing reads the fproc interface"""
    out = []
    for p in progs:
        q = []
        for w in p:
            d = isa.decode(w)
            if d['op'] == 'alu_fproc':
                w = raw(1, d['in0_reg'], isa.ALU_OPS[d['alu_op']], imm=d['imm'], rs0=d['rs0'], rs1=d['rs1'], rd=d['rd'])
            elif d['op'] == 'jump_fproc':
                w = raw(3, d['in0_reg'], isa.ALU_OPS[d['alu_op']], imm=d['imm'], rs0=d['rs0'], rs1=d['rs1'],
                        target=d['target'])
            q.append(w)
        out.append(q)
    return out


def without_sync(progs):
    """the programs with every sync the inc_qclk `qclk = -3` (id0): qclk is 0 three cycles after its decode and 1 at
    the next decode, as after a barrier release (qclk(S + 2) = 0, decode at S + 3).  Gen.program continues its
    qclk estimate from 1 there, so the triggers that follow stay in the future"""
    return [[raw(6, 0, 0, imm=-3) if isa.decode(w)['op'] == 'sync' else w for w in p] for p in progs]


# ---- the five facts of csrc/program_image.h, restated ----

Facts = collections.namedtuple('Facts', 'has_fproc has_sync reg_writes straight linear')


def program_facts(progs):
    ops = {isa.decode(w)['op4'] for p in progs for w in p}
    return Facts(has_fproc=bool(ops & {4, 5}), has_sync=7 in ops, reg_writes=bool(ops & {1, 4}),
                 straight=not ops & set(range(1, 8)), linear=not ops & {2, 3, 4, 5, 7})


def has_jump(progs):
    return any(isa.decode(w)['op4'] in (2, 3, 5) for p in progs for w in p)


def names_source_register(progs):
    """some command reads the reg_file: a jump_cond (in1 = reg[rs1]), a register-sourced pulse field, or the
    register form of in0 (in0_reg) of an ALU-class command whose op reads in0"""
    for p in progs:
        for w in p:
            d = isa.decode(w)
            if d['op'] == 'jump_cond':
                return True
            if d['op'] in ('pulse_write', 'pulse_write_trig') and any(
                    d[k + '_we'] and d[k + '_sel'] for k in ('env_word', 'phase', 'freq', 'amp')):
                return True
            if d['op'] in ('jump_fproc', 'inc_qclk') and d['in0_reg'] and d['alu_op'] not in ('id1', 'zero'):
                return True
    return False


# ---- the table ----

# family: 'branch' | 'interp'; model: 'state' | 'demod' | 'states'; feat: the FEAT_* bits of the instantiation
# without the model's bit; c8: the compile-time C = 8 instantiation (branch_kernel only); seed, C, n_groups, body:
# random_case's arguments (body None: its own draw); shots_per_group, n_shots, order, exec_flags: the run's; ro_seed:
# the seed of a DEMOD row's model parameters and frequency tables (demod_setup)
Row = collections.namedtuple('Row', 'family model feat c8 seed C n_groups shots_per_group n_shots order exec_flags body '
                             'ro_seed', defaults=(None,))

XG, XL, XM = _abi.X_GENERAL, _abi.X_PROG_LDS, _abi.X_PROG_MAJOR

# Shapes: n_shots * C in [257, 511] and no multiple of 64 (two workgroups, a partly filled last wave, invalid tail
# lanes); shots_per_group below the 256 / C shots of a workgroup.  The rows without FEAT_PROG_LDS alternate between
# DPEMU_X_PROG_MAJOR and programs too long to stage (long blocks; under the LUT back end, whose reads wait hundreds
# of cycles each, many groups of short programs instead, so that lanes still finish within max_cycles).
# Seeds: the first from the row's own range that has the features the row needs and meets the reach conditions of
# tests/test_feature_cases.py, found on the CPU with oracle_fast alone.  DEMOD rows that read fproc_meas need a
# readout whose window ends before a later read, so their ro_seed is one that draws cpw = 1, a delay below 40 and
# sigma = 200 (outcomes that differ between run seeds within a few hundred cycles); the other DEMOD rows take
# 70000 + seed.
INSTANTIATIONS = [
    Row('branch', 'state', 0x08, True, 1000, 8, 2, 20, 37, CM, 0, (3, 6)),
    Row('branch', 'state', 0x08, False, 1400, 1, 3, 100, 301, SM, 0, None),
    Row('branch', 'state', 0x09, True, 1802, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'state', 0x09, False, 2203, 2, 3, 50, 150, CM, 0, (3, 6)),
    Row('branch', 'state', 0x0a, True, 2600, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'state', 0x0a, False, 3001, 2, 3, 50, 150, SM, 0, None),
    Row('branch', 'state', 0x0b, True, 3404, 8, 2, 20, 37, SM, 0, (2, 4)),
    Row('branch', 'state', 0x0b, False, 3800, 4, 2, 25, 77, CM, 0, None),
    Row('branch', 'state', 0x0c, True, 4200, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'state', 0x0c, False, 4615, 4, 2, 25, 77, SM, 0, None),
    Row('branch', 'state', 0x0e, True, 5065, 8, 2, 20, 37, SM, 0, None),
    Row('branch', 'state', 0x0e, False, 5513, 16, 2, 10, 19, CM, 0, (2, 4)),
    Row('branch', 'state', 0x00, True, 5800, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'state', 0x00, False, 6200, 16, 2, 10, 19, SM, XM, None),
    Row('branch', 'state', 0x01, True, 6600, 8, 2, 20, 37, SM, 0, (15, 25)),
    Row('branch', 'state', 0x01, False, 7003, 1, 3, 100, 301, CM, 0, (100, 120)),
    Row('branch', 'state', 0x02, True, 7401, 8, 2, 20, 37, CM, XM, (3, 6)),
    Row('branch', 'state', 0x02, False, 7804, 2, 3, 50, 150, SM, XM, None),
    Row('branch', 'state', 0x03, True, 8206, 8, 2, 20, 37, SM, 0, (30, 45)),
    Row('branch', 'state', 0x03, False, 8614, 4, 2, 25, 77, CM, 0, (15, 25)),
    Row('branch', 'state', 0x04, True, 9001, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'state', 0x04, False, 9405, 2, 3, 50, 150, SM, XM, (3, 6)),
    Row('branch', 'state', 0x06, True, 9816, 8, 8, 4, 37, SM, 0, (3, 6)),
    Row('branch', 'state', 0x06, False, 10290, 16, 4, 4, 19, CM, 0, (2, 4)),
    Row('branch', 'state', 0x28, True, 10600, 8, 2, 20, 37, CM, 0, (3, 6)),
    Row('branch', 'state', 0x28, False, 11000, 4, 2, 25, 77, SM, 0, None),
    Row('branch', 'state', 0x29, True, 11403, 8, 2, 20, 37, SM, 0, None),
    Row('branch', 'state', 0x29, False, 11805, 16, 2, 10, 19, CM, 0, (3, 6)),
    Row('branch', 'state', 0x2a, True, 12201, 8, 2, 20, 37, CM, 0, (2, 4)),
    Row('branch', 'state', 0x2a, False, 12600, 2, 3, 50, 150, SM, 0, None),
    Row('branch', 'state', 0x2b, True, 13003, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'state', 0x2b, False, 13417, 4, 2, 25, 77, CM, 0, None),
    Row('branch', 'state', 0x2c, True, 13801, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'state', 0x2c, False, 14200, 1, 3, 100, 301, SM, 0, 2),
    Row('branch', 'state', 0x2e, True, 14644, 8, 2, 20, 37, SM, 0, 2),
    Row('branch', 'state', 0x2e, False, 15162, 16, 2, 10, 19, CM, 0, 2),
    Row('branch', 'state', 0x20, True, 15400, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'state', 0x20, False, 15800, 2, 3, 50, 150, SM, XM, None),
    Row('branch', 'state', 0x21, True, 16200, 8, 2, 20, 37, SM, 0, (30, 45)),
    Row('branch', 'state', 0x21, False, 16600, 4, 2, 25, 77, CM, 0, (15, 25)),
    Row('branch', 'state', 0x22, True, 17000, 8, 2, 20, 37, CM, XM, (3, 6)),
    Row('branch', 'state', 0x22, False, 17400, 2, 3, 50, 150, SM, XM, None),
    Row('branch', 'state', 0x23, True, 17801, 8, 2, 20, 37, SM, 0, (15, 25)),
    Row('branch', 'state', 0x23, False, 18215, 4, 2, 25, 77, CM, 0, (15, 25)),
    Row('branch', 'state', 0x24, True, 18601, 8, 2, 20, 37, CM, XM, (3, 6)),
    Row('branch', 'state', 0x24, False, 19001, 16, 2, 10, 19, SM, XM, (3, 6)),
    Row('branch', 'state', 0x26, True, 19407, 8, 8, 4, 37, SM, 0, (3, 6)),
    Row('branch', 'state', 0x26, False, 19909, 16, 4, 4, 19, CM, 0, (2, 4)),
    Row('branch', 'demod', 0x08, True, 20200, 8, 2, 20, 37, CM, 0, None, 90200),
    Row('branch', 'demod', 0x08, False, 20600, 1, 3, 100, 301, SM, 0, None, 90600),
    Row('branch', 'demod', 0x09, True, 21277, 8, 2, 20, 37, SM, 0, None, 72884),
    Row('branch', 'demod', 0x09, False, 21406, 2, 3, 50, 150, CM, 0, (3, 6), 70292),
    Row('branch', 'demod', 0x0a, True, 21800, 8, 2, 20, 37, CM, 0, (2, 4), 91800),
    Row('branch', 'demod', 0x0a, False, 22200, 2, 3, 50, 150, SM, 0, None, 92200),
    Row('branch', 'demod', 0x0b, True, 22600, 8, 2, 20, 37, SM, 0, (2, 4), 70004),
    Row('branch', 'demod', 0x0b, False, 23371, 4, 2, 25, 77, CM, 0, (2, 4), 70853),
    Row('branch', 'demod', 0x0c, True, 23405, 8, 2, 20, 37, CM, 0, (2, 4), 93405),
    Row('branch', 'demod', 0x0c, False, 23833, 4, 2, 25, 77, SM, 0, None, 93833),
    Row('branch', 'demod', 0x0e, True, 24395, 8, 2, 20, 37, SM, 0, (2, 4), 94395),
    Row('branch', 'demod', 0x0e, False, 24886, 16, 2, 10, 19, CM, 0, (2, 4), 94886),
    Row('branch', 'demod', 0x00, True, 25000, 8, 2, 20, 37, CM, XM, None, 95000),
    Row('branch', 'demod', 0x00, False, 25400, 16, 2, 10, 19, SM, XM, None, 95400),
    Row('branch', 'demod', 0x01, True, 25822, 8, 2, 20, 37, SM, 0, (15, 25), 95822),
    Row('branch', 'demod', 0x01, False, 26412, 1, 3, 100, 301, CM, 0, (100, 120), 96412),
    Row('branch', 'demod', 0x02, True, 26601, 8, 2, 20, 37, CM, XM, (3, 6), 96601),
    Row('branch', 'demod', 0x02, False, 27001, 2, 3, 50, 150, SM, XM, None, 97001),
    Row('branch', 'demod', 0x03, True, 27593, 8, 2, 20, 37, SM, 0, (60, 80), 71640),
    Row('branch', 'demod', 0x03, False, 27886, 4, 2, 25, 77, CM, 0, (60, 80), 71175),
    Row('branch', 'demod', 0x04, True, 28206, 8, 2, 20, 37, CM, XM, None, 98206),
    Row('branch', 'demod', 0x04, False, 28613, 2, 3, 50, 150, SM, XM, (3, 6), 98613),
    Row('branch', 'demod', 0x06, True, 29134, 8, 8, 4, 37, SM, 0, (3, 6), 99134),
    Row('branch', 'demod', 0x06, False, 29675, 16, 4, 4, 19, CM, 0, (2, 4), 99675),
    Row('branch', 'demod', 0x28, True, 29800, 8, 2, 20, 37, CM, 0, (3, 6), 99800),
    Row('branch', 'demod', 0x28, False, 30200, 4, 2, 25, 77, SM, 0, None, 100200),
    Row('branch', 'demod', 0x29, True, 30665, 8, 2, 20, 37, SM, 0, (2, 4), 100665),
    Row('branch', 'demod', 0x29, False, 32134, 1, 3, 100, 301, CM, 0, (2, 4), 72740),
    Row('branch', 'demod', 0x2a, True, 31401, 8, 2, 20, 37, CM, 0, (3, 6), 101401),
    Row('branch', 'demod', 0x2a, False, 31802, 2, 3, 50, 150, SM, 0, None, 101802),
    Row('branch', 'demod', 0x2b, True, 32238, 8, 2, 20, 37, SM, 0, (3, 6), 72128),
    Row('branch', 'demod', 0x2b, False, 33310, 4, 2, 25, 77, CM, 0, None, 70407),
    Row('branch', 'demod', 0x2c, True, 33008, 8, 2, 20, 37, CM, 0, None, 103008),
    Row('branch', 'demod', 0x2c, False, 33445, 2, 3, 50, 150, SM, 0, None, 103445),
    Row('branch', 'demod', 0x2e, True, 34170, 8, 2, 20, 37, SM, 0, 2, 104170),
    Row('branch', 'demod', 0x2e, False, 34428, 16, 2, 10, 19, CM, 0, 2, 104428),
    Row('branch', 'demod', 0x20, True, 34600, 8, 2, 20, 37, CM, XM, None, 104600),
    Row('branch', 'demod', 0x20, False, 35000, 4, 2, 25, 77, SM, XM, None, 105000),
    Row('branch', 'demod', 0x21, True, 35409, 8, 2, 20, 37, SM, 0, (60, 80), 105409),
    Row('branch', 'demod', 0x21, False, 35800, 16, 2, 10, 19, CM, 0, (60, 80), 105800),
    Row('branch', 'demod', 0x22, True, 36201, 8, 2, 20, 37, CM, XM, None, 106201),
    Row('branch', 'demod', 0x22, False, 36604, 2, 3, 50, 150, SM, XM, None, 106604),
    Row('branch', 'demod', 0x23, True, 37043, 8, 2, 20, 37, SM, 0, (30, 45), 72498),
    Row('branch', 'demod', 0x23, False, 37404, 4, 2, 25, 77, CM, 0, (100, 120), 70075),
    Row('branch', 'demod', 0x24, True, 37826, 8, 2, 20, 37, CM, XM, (3, 6), 107826),
    Row('branch', 'demod', 0x24, False, 38396, 1, 3, 100, 301, SM, XM, None, 108396),
    Row('branch', 'demod', 0x26, True, 38690, 8, 8, 4, 37, SM, 0, (3, 6), 108690),
    Row('branch', 'demod', 0x26, False, 39271, 16, 4, 4, 19, CM, 0, (2, 4), 109271),
    Row('branch', 'states', 0x08, True, 39400, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'states', 0x08, False, 39800, 2, 3, 50, 150, SM, 0, None),
    Row('branch', 'states', 0x09, True, 40200, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x09, False, 40601, 4, 2, 25, 77, CM, 0, None),
    Row('branch', 'states', 0x0a, True, 41000, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'states', 0x0a, False, 41400, 2, 3, 50, 150, SM, 0, None),
    Row('branch', 'states', 0x0b, True, 41815, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x0b, False, 42228, 4, 2, 25, 77, CM, 0, (2, 4)),
    Row('branch', 'states', 0x0c, True, 42602, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'states', 0x0c, False, 43000, 16, 2, 10, 19, SM, 0, 2),
    Row('branch', 'states', 0x0e, True, 43488, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x0e, False, 43941, 16, 2, 10, 19, CM, 0, (2, 4)),
    Row('branch', 'states', 0x00, True, 44200, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'states', 0x00, False, 44600, 1, 3, 100, 301, SM, XM, None),
    Row('branch', 'states', 0x01, True, 45000, 8, 2, 20, 37, SM, 0, (15, 25)),
    Row('branch', 'states', 0x01, False, 45400, 2, 3, 50, 150, CM, 0, (30, 45)),
    Row('branch', 'states', 0x02, True, 45802, 8, 2, 20, 37, CM, XM, (3, 6)),
    Row('branch', 'states', 0x02, False, 46200, 2, 3, 50, 150, SM, XM, None),
    Row('branch', 'states', 0x03, True, 46664, 8, 2, 20, 37, SM, 0, (30, 45)),
    Row('branch', 'states', 0x03, False, 47001, 4, 2, 25, 77, CM, 0, (15, 25)),
    Row('branch', 'states', 0x04, True, 47402, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'states', 0x04, False, 47801, 4, 2, 25, 77, SM, XM, None),
    Row('branch', 'states', 0x06, True, 48272, 8, 8, 4, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x06, False, 48659, 16, 4, 4, 19, CM, 0, (2, 4)),
    Row('branch', 'states', 0x28, True, 49000, 8, 2, 20, 37, CM, 0, None),
    Row('branch', 'states', 0x28, False, 49400, 16, 2, 10, 19, SM, 0, (2, 4)),
    Row('branch', 'states', 0x29, True, 49801, 8, 2, 20, 37, SM, 0, None),
    Row('branch', 'states', 0x29, False, 50205, 1, 3, 100, 301, CM, 0, None),
    Row('branch', 'states', 0x2a, True, 50601, 8, 2, 20, 37, CM, 0, (2, 4)),
    Row('branch', 'states', 0x2a, False, 51001, 2, 3, 50, 150, SM, 0, None),
    Row('branch', 'states', 0x2b, True, 51405, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x2b, False, 51804, 4, 2, 25, 77, CM, 0, None),
    Row('branch', 'states', 0x2c, True, 52201, 8, 2, 20, 37, CM, 0, 2),
    Row('branch', 'states', 0x2c, False, 52626, 2, 3, 50, 150, SM, 0, (2, 4)),
    Row('branch', 'states', 0x2e, True, 53230, 8, 2, 20, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x2e, False, 53511, 16, 2, 10, 19, CM, 0, 2),
    Row('branch', 'states', 0x20, True, 53800, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'states', 0x20, False, 54200, 4, 2, 25, 77, SM, XM, (3, 6)),
    Row('branch', 'states', 0x21, True, 54600, 8, 2, 20, 37, SM, 0, (15, 25)),
    Row('branch', 'states', 0x21, False, 55000, 16, 2, 10, 19, CM, 0, (15, 25)),
    Row('branch', 'states', 0x22, True, 55400, 8, 2, 20, 37, CM, XM, (3, 6)),
    Row('branch', 'states', 0x22, False, 55800, 2, 3, 50, 150, SM, XM, None),
    Row('branch', 'states', 0x23, True, 56208, 8, 2, 20, 37, SM, 0, (15, 25)),
    Row('branch', 'states', 0x23, False, 56610, 4, 2, 25, 77, CM, 0, (15, 25)),
    Row('branch', 'states', 0x24, True, 57002, 8, 2, 20, 37, CM, XM, None),
    Row('branch', 'states', 0x24, False, 57401, 1, 3, 100, 301, SM, XM, (3, 6)),
    Row('branch', 'states', 0x26, True, 57817, 8, 8, 4, 37, SM, 0, (3, 6)),
    Row('branch', 'states', 0x26, False, 58221, 16, 4, 4, 19, CM, 0, (2, 4)),
    Row('interp', 'state', 0x10, False, 58600, 2, 3, 50, 150, CM, XG, None),
    Row('interp', 'state', 0x00, False, 59000, 8, 2, 20, 37, SM, XG, None),
    Row('interp', 'state', 0x01, False, 59400, 4, 2, 25, 77, SM, XG, None),
    Row('interp', 'state', 0x02, False, 59804, 16, 2, 10, 19, CM, XG, None),
    Row('interp', 'state', 0x03, False, 60203, 2, 3, 50, 150, CM, XG, (30, 45)),
    Row('interp', 'state', 0x04, False, 60604, 8, 2, 20, 37, SM, XG, (30, 45)),
    Row('interp', 'state', 0x06, False, 61371, 4, 2, 25, 77, SM, XG, None),
    Row('interp', 'state', 0x18, False, 61400, 16, 2, 10, 19, CM, XG | XL, None),
    Row('interp', 'state', 0x08, False, 61800, 1, 3, 100, 301, CM, XG | XL, None),
    Row('interp', 'state', 0x09, False, 62200, 2, 3, 50, 150, SM, XG | XL, None),
    Row('interp', 'state', 0x0a, False, 62600, 8, 2, 20, 37, SM, XG | XL, (3, 6)),
    Row('interp', 'state', 0x0b, False, 63004, 4, 2, 25, 77, CM, XG | XL, None),
    Row('interp', 'state', 0x0c, False, 63400, 16, 2, 10, 19, CM, XG | XL, None),
    Row('interp', 'state', 0x0e, False, 63805, 2, 3, 50, 150, SM, XG | XL, (3, 6)),
]


def row_id(r):
    return '{}-{}-0x{:x}{}'.format(r.family, r.model, r.feat | MODEL_BIT[r.model], '-c8' if r.c8 else '')


def kernel_name(r):
    """dpemu_last_kernel's name of the instantiation the row claims"""
    f = r.feat | MODEL_BIT[r.model]
    if r.family == 'interp':
        return 'interp_kernel<feat=0x{:x}>'.format(f)
    return 'branch_kernel<feat=0x{:x}{}>'.format(f, ',c8' if r.c8 else '')


def instantiation(r):
    """the template arguments of the row's kernel: ('branch', FEAT, CT) or ('interp', F)"""
    f = r.feat | MODEL_BIT[r.model]
    return ('interp', f) if r.family == 'interp' else ('branch', f, 8 if r.c8 else 0)


def requested(r):
    """(xmeas, sync, reg_writes) the row's programs must have; reg_writes None: as the seed has them (interp_kernel
    has no instantiation per register use)"""
    xmeas = 'lut' if r.feat & FEAT_LUT else 'fproc' if r.feat & FEAT_FPROC else 'none'
    return xmeas, bool(r.feat & FEAT_SYNC), None if r.family == 'interp' else bool(r.feat & FEAT_REGS)


@functools.lru_cache(maxsize=None)
def programs_of_row(r):
    """the row's ProgramSet, its facts asserted to be exactly the requested ones"""
    xmeas, sync, regs = requested(r)
    straight = bool(r.feat & FEAT_STRAIGHT)
    case = random_case(r.seed, ncores=r.C, mode='lut' if xmeas == 'lut' else 'meas', allow_late=True, allow_hang=True,
                       n_groups=r.n_groups, straight=straight, body=r.body)
    progs = case['progs']
    if regs is False:
        progs = without_register_writes(progs)
    if xmeas == 'none':
        progs = without_fproc(progs)
    if not sync:
        progs = without_sync(progs)
    f = program_facts(progs)
    assert f.has_fproc == (xmeas != 'none') and f.has_sync == sync and f.straight == straight, (row_id(r), f)
    assert regs is None or f.reg_writes == regs, (row_id(r), f)
    assert f.linear == (not has_jump(progs) and not f.has_fproc and not f.has_sync), (row_id(r), f)
    if r.family == 'branch' and r.model == 'state':
        # the plan sends a STATE-model program set without a jump, fproc read or sync to the straight / macro kernels
        assert has_jump(progs) and not f.linear, row_id(r)
    groups = [[progs[case['table'][g * r.C + c]] for c in range(r.C)] for g in range(r.n_groups)]
    return ProgramSet(groups, cores_per_shot=r.C)


def shot0_of(r):
    return (r.seed * 37) % 100000


def demod_setup(r, ps):
    """the DEMOD rows' model parameters and frequency tables, drawn as tests/test_gpu_demod.py draws them"""
    from tests.test_fast_vs_rtl import demod_params
    from tests.test_gpu_demod import random_tables
    rng = random.Random(r.ro_seed)
    meas_elem = r.ro_seed % 4
    return meas_elem, demod_params(rng, r.C, meas_elem), random_tables(rng, ps.n_programs)


def config_of_row(r, ps, seed=SEED_A):
    """-> (config, DEMOD frequency tables or None)"""
    p1 = [(0.5, 0.3, 0.8, 0.05, 0.95, 0.6, 1.0, 0.0)[c % 8] for c in range(r.C)]
    kw, tables = {}, None
    if r.model == 'demod':
        kw['meas_elem'], kw['demod'], tables = demod_setup(r, ps)
    cfg = _abi.make_config(r.C, n_groups=ps.n_groups, shots_per_group=r.shots_per_group, max_cycles=6000, event_cap=32,
                           trace_cap=16, meas_cap=8,
                           fproc_mode=_abi.FPROC_LUT if r.feat & FEAT_LUT else _abi.FPROC_MEAS,
                           meas_latency=1 + r.seed % 23, sync_latency=1 + r.seed % 3, seed=seed, p1=p1,
                           lane_order=r.order, exec_flags=r.exec_flags, **kw)
    return cfg, tables


def outs_of(cfg):
    return tuple(k for k in ALL_OUT + ('acc',) if (k != 'hist' or cfg.cores_per_shot <= 12) and
                 (k != 'acc' or cfg.meas_model == _abi.MEAS_DEMOD))


def oracle_of_row(r, seed=SEED_A):
    import oracle
    ps = programs_of_row(r)
    cfg, tables = config_of_row(r, ps, seed)
    return oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, shot0_of(r), r.n_shots, want=outs_of(cfg),
                           ro=tables)


# ---- the census of built kernels ----

def built_instantiations(symbols):
    """the branch_kernel<FEAT, CT> / interp_kernel<F> template arguments among mangled kernel symbol names, as
    instantiation() writes them"""
    out = set()
    for s in symbols:
        m = re.search(r'13branch_kernelILi(\d+)ELi(\d+)EE', s)
        if m:
            out.add(('branch', int(m.group(1)), int(m.group(2))))
        m = re.search(r'13interp_kernelILi(\d+)EE', s)
        if m:
            out.add(('interp', int(m.group(1))))
    return out


def census(symbols, rows):
    """-> (instantiations built without a row, rows whose kernel is not built), both sorted lists"""
    built, claimed = built_instantiations(symbols), {instantiation(r) for r in rows}
    return sorted(built - claimed), sorted(claimed - built)


# ---- shared with tests/test_gpu_run_states.py ----

def lane_shots_cores(cfg, n_shots, shot0):
    L = np.arange(n_shots * cfg.cores_per_shot)
    if cfg.lane_order == SM:
        return shot0 + L // cfg.cores_per_shot, L % cfg.cores_per_shot
    return shot0 + L % n_shots, L // n_shots


def drawn_states(cfg, n_shots, shot0, n_bits=32):
    """the words whose bit m is cfg's own state draw of (shot, core, m), in the run's lane order"""
    shot, core = lane_shots_cores(cfg, n_shots, shot0)
    return mref.draw_words(cfg, shot, core, n_bits)


def device_run(emu, ps, cfg, n_shots, shot0, states, outs, entry=None):
    """a device run into zeroed buffers, copied back as the oracle's unsigned arrays; states: uint32 words or None"""
    import torch
    if emu.programs is not ps:
        emu.load(ps)
    dev = alloc_device_outputs(cfg, n_shots, want=outs)
    for t in dev.values():
        t.zero_()
    st = None if states is None else torch.from_numpy(np.ascontiguousarray(states).view(np.int32).copy()).cuda()
    if entry is None:
        emu.run_device(cfg, n_shots, shot0, dev, states=st)
    else:
        entry(dev, st)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().view(np.int32 if k == 'acc' else np.uint64 if k == 'hist' else np.uint32)
            for k, v in dev.items()}


def compare(got, want, ctx):
    for k in want:
        assert k in got, (ctx, k)
        a, b = np.asarray(got[k]).reshape(-1), np.asarray(want[k]).reshape(-1)
        assert a.shape == b.shape, (ctx, k, a.shape, b.shape)
        if not np.array_equal(a, b):
            bad = np.flatnonzero(a != b)
            raise AssertionError('{} {}: {} mismatches, first at {}: gpu {} ref {}'.format(
                ctx, k, len(bad), bad[0], a[bad[0]], b[bad[0]]))


def paths_differ(fa, fb):
    """lanes whose control flow differs: the stop cycle, the final ip or the instructions decoded"""
    a, b = fa['summary'].reshape(-1, 8), fb['summary'].reshape(-1, 8)
    return (a[:, 0] != b[:, 0]) | ((a[:, 1] & 0xFFFF) != (b[:, 1] & 0xFFFF)) | (a[:, 3] != b[:, 3])
