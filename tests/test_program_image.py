"""The load-time program image (csrc/program_image.h) on the CPU: the decoded
commands in both orders, the macro image of branch-free register programs
(round trip back to the commands, MACRO_SIMPLE, lean chunks, register
renumbering) and the facts the kernel choice reads.  The checks themselves are
in tests/program_image_test.cpp; this file supplies the program sets and
asserts the per-case facts the binary prints."""

import os
import random
import re
import shutil
import subprocess

import numpy as np
import pytest

from distributed_processor_amd import isa, workloads
from tests.progfuzz import dead_tail_program, pack_programs, random_case

HERE = os.path.dirname(os.path.abspath(__file__))


def case_words(C, n_groups, words, offsets, n_instr, table):
    """one case of the binary's input: header, offsets, n_instr, prog_table, words (all u32)"""
    words = np.ascontiguousarray(words, np.uint32).reshape(-1, 4)
    head = np.array([C, n_groups, len(offsets), len(words)], np.uint32)
    return [head, np.asarray(offsets, np.uint32), np.asarray(n_instr, np.uint32), np.asarray(table, np.uint32),
            words.ravel()]


def from_programs(C, n_groups, progs, table=None):
    words, offsets, n_instr = pack_programs(progs)
    return case_words(C, n_groups, words, offsets, n_instr,
                      np.arange(n_groups * C, dtype=np.uint32) if table is None else table)


def lean_chunk_core(w, step):
    """the program of test_gpu_rb.py::test_lean_chunk_after_qclk_wrap"""
    words = [isa.pulse_reset(), isa.reg_alu_i(0, 'id0', 0, 1), isa.inc_qclk_i(-w)]
    for k in range(40):
        words.append(isa.reg_alu_i(5, 'add', 1, 1))
        words.append(isa.pulse_i(freq_word=3, phase_word=0, amp_word=100, env_word=1 | (4 << 12),
                                 cfg_word=0, cmd_time=10 + step * k))
    words.append(isa.done_cmd())
    return words


def build_cases():
    cases, names, n_regs = [], [], {}
    for seed in range(12):                          # the samples of test_gpu_parity.py::test_fuzz_linear_few_registers
        regs = random.Random(seed).sample(range(16), 1 + seed % 4)
        for C in (1, 2, 4):
            case = random_case(17000 + seed, ncores=C, mode='meas', allow_late=seed % 2 == 1, allow_hang=True,
                               n_groups=9 + seed, linear=True, regs=regs)
            n_regs[len(cases)] = len(regs)
            names.append('fuzz seed {} C {}'.format(seed, C))
            cases.append(from_programs(C, case['n_groups'], case['progs'], case['table']))
    ps = workloads.config4_rb_set(96, 40)
    names.append('rb')
    cases.append(case_words(ps.cores_per_shot, ps.n_groups, ps.words, ps.offsets, ps.n_instr, ps.table))
    names.append('lean chunk')
    cases.append(from_programs(1, 1, [lean_chunk_core(1000, 20)]))
    names.append('dead tail')
    cases.append(from_programs(1, 1, [dead_tail_program()]))
    # one long pulse-only program among a hundred short ones: the command-major copy would be
    # mostly padding (5001 rows x 101 programs against 5201 commands), so the padding rule declines it
    pulse = isa.pulse_i(freq_word=1, phase_word=0, amp_word=1, env_word=1, cfg_word=0, cmd_time=5)
    names.append('padding')
    cases.append(from_programs(1, 101, [[pulse] * 4999 + [isa.done_cmd()]] + [[isa.done_cmd()]] * 100))
    return cases, names, n_regs


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_program_image(tmp_path):
    exe = str(tmp_path / 'program_image_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'program_image_test.cpp')],
                   check=True)
    cases, names, n_regs = build_cases()
    path = str(tmp_path / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(np.array([len(cases)], np.uint32).tobytes())
        for parts in cases:
            for a in parts:
                fh.write(np.ascontiguousarray(a, np.uint32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'OK'
    facts = [dict((k, int(v, 0)) for k, v in re.findall(r'(\w+)=(\S+)', ln)) for ln in lines[:-1]]
    assert len(facts) == len(cases)
    by_name = dict(zip(names, facts))
    for i, f in enumerate(facts):
        if i in n_regs:
            assert f['linear'] and f['macros'] and f['cm'], names[i]
            assert bin(f['used']).count('1') <= n_regs[i] or f['nr'] == 16, names[i]
            if n_regs[i] <= 2:
                assert f['nr'] == 2 and f['w3'] == 1, names[i]
    assert {f['w3'] for i, f in enumerate(facts) if i in n_regs} == {0, 1}      # both layouts were checked
    rb = by_name['rb']
    assert (rb['nr'], rb['w3'], rb['addid']) == (2, 1, 1) and rb['simple'] > 0 and rb['lean'] > 0
    lean = by_name['lean chunk']
    assert (lean['nr'], lean['addid']) == (2, 1) and lean['lean'] >= 1          # whole chunks after the qclk wrap
    # the unreachable tail names r3..r5: only the commands up to `done` decide the layout
    dead = by_name['dead tail']
    assert (dead['macros'], dead['nr'], dead['w3'], dead['used']) == (1, 2, 1, 0b110)
    pad = by_name['padding']
    assert (pad['straight'], pad['macros'], pad['cm']) == (1, 0, 0)
