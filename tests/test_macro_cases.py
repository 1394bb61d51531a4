"""The case table of tests/macro_cases.py on the CPU: what
tests/test_gpu_macro_paths.py relies on, asserted without a GPU so that no case
passes vacuously -- the macro image of every case (tests/program_image_test.cpp:
macro counts, lean chunks, MACRO_SIMPLE macros with a third ALU slot, with no
pulse slot, with every ALU op, with the register form of in0, the
register-sourced pulse fields), the kernel csrc/launch_plan.h names for it, a
timing model of branch-free programs held to oracle_fast's event and trace
times, with it macro.hip's lean_chunk_ok / lean_ok / simple_ok restated per
(program, chunk or macro, max_cycles) and the sweeps of family H placed across
their flips, the lane endings the cases were chosen for (oracle_fast), and
oracle_fast against the per-clock oracle_rtl on one program set per family."""

import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import oracle
from distributed_processor_amd import _abi, isa
from tests import macro_cases as mc
from tests.progfuzz import pack_programs
from tests.test_fast_vs_rtl import EV_CAP, HORIZON, MEAS_CAP, TR_CAP, compare
from tests.test_launch_plan import plan, run_line        # noqa: F401  (plan: the fixture)
from tests.test_program_image import from_programs
from tests.test_staging_cases import facts as plan_facts

HERE = os.path.dirname(os.path.abspath(__file__))
SINGLE, FUZZ = mc.FAMILY_G_SINGLE, mc.FAMILY_G_FUZZ


def ids(cases):
    return [c.name for c in cases]


@pytest.fixture(scope='module')
def image(tmp_path_factory):
    """the image tool's facts of every case, by name"""
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    d = tmp_path_factory.mktemp('image')
    exe = str(d / 'program_image_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'program_image_test.cpp')],
                   check=True)
    path = str(d / 'cases.bin')
    with open(path, 'wb') as fh:
        fh.write(np.array([len(mc.ALL)], np.uint32).tobytes())
        for c in mc.ALL:
            fz = mc.fuzz_case(c)
            for a in from_programs(c.C, c.n_groups, fz['progs'], fz['table']):
                fh.write(np.ascontiguousarray(a, np.uint32).tobytes())
    r = subprocess.run([exe, path], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == 'OK' and len(lines) == len(mc.ALL) + 1
    return {c.name: dict((k, int(v, 0)) for k, v in re.findall(r'(\w+)=(\S+)', ln)) for c, ln in zip(mc.ALL, lines)}


def chunk_kinds(c, words, w3):
    """per chunk of the program: True lean candidate, False MIXED (macro_cases.is_simple over macros_of)"""
    mac = mc.macros_of(words, 3 if w3 else 2)
    return [mc.lean_candidate(words, mac, ch) for ch in range(-(-len(mac) // mc.CHUNK))]


# ---------------------------------------------------------------- the images
@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
@pytest.mark.skipif(shutil.which('g++') is None, reason='g++ not available')
def test_images_reach_the_paths(image):
    rs = 0
    for c in mc.ALL:
        f = image[c.name]
        assert f['linear'] and f['macros'] and not f['straight'], c.name
        assert (f['nr'], f['w3']) == ((2, 1) if c.n_regs <= 2 else (16, 0)), (c.name, f)
        assert bin(f['used']).count('1') == c.n_regs or f['nr'] == 16, (c.name, f)
        assert f['addid'] == int(c.addid), (c.name, f)
        assert ('<{}'.format(f['nr']) in c.kernel or c.kernel == 'macro_kernel') and \
            (',addid' in c.kernel) == bool(f['addid'] and c.kernel != 'macro_kernel'), (c.name, c.kernel)
        # the Python restatement of the macro image (the timing checks below build on it) against the tool's
        progs = mc.fuzz_case(c)['progs']
        kinds = [chunk_kinds(c, w, f['w3']) for w in progs]
        nm = [len(mc.macros_of(w, 3 if f['w3'] else 2)) for w in progs]
        assert (min(nm), max(nm)) == (f['nm_min'], f['nm_max']), c.name
        assert sum(map(sum, kinds)) == f['lean'] and min(map(sum, kinds)) == f['lean_min'], c.name
        if c.family in 'FH' or c in SINGLE:
            assert f['nm_min'] == f['nm_max'] == c.M, (c.name, f)
        if c.family in 'FH':
            # every macro but the first and the terminal one is simple: all chunks but 0 and those that
            # reach the terminal macro are lean candidates
            assert f['simple'] == (c.M - 2) * c.n_groups * c.C, (c.name, f)
            assert f['lean_min'] == (c.M - 1) // 16 - 1 >= 1 and f['lean'] == f['lean_min'] * c.n_groups * c.C, (c.name, f)
            assert f['ops'] == (0x3 if c.addid else 0xff), (c.name, hex(f['ops']))
            assert f['absent'] > 0 and f['in0reg'] > 0 and (f['third'] > 0) == bool(f['w3']), (c.name, f)
            rs |= f['rs'] >> 16
            if c.addid:
                assert f['rs'] >> 16 == 0xf, (c.name, hex(f['rs']))      # all four fields in one addid image
    assert rs == 0xf                        # UOP_RS_ENV | PH | FR | AMP over the family
    for c in SINGLE:
        # exactly the one MIXED chunk between lean ones: chunks 0 (macro 0) and 4 (terminal) are MIXED
        # by construction
        (kinds,) = [chunk_kinds(c, w, image[c.name]['w3']) for w in mc.fuzz_case(c)['progs']]
        assert kinds == [False, True, False, True, False], (c.name, kinds)
        assert image[c.name]['lean'] == 2 and image[c.name]['simple'] == c.M - 3
    # g_fuzz: a lean chunk and a MIXED one at the same chunk index in consecutive groups' programs of one
    # core (spg <= 32: every wave of 64 shots holds two groups and more); both with 2 and with 3+ registers
    seen = set()
    for c in FUZZ:
        f = image[c.name]
        progs = mc.fuzz_case(c)['progs']
        kinds = [chunk_kinds(c, w, f['w3']) for w in progs]
        assert c.spg <= 32 and len(set(len(k) for k in kinds)) > 1
        for g in range(c.n_groups):
            for k in range(c.C):
                a, b = kinds[g * c.C + k], kinds[(g + 1) % c.n_groups * c.C + k]
                if any(x != y for x, y in zip(a[1:], b[1:len(b) - 1])):
                    seen.add(f['nr'])
    assert seen == {2, 16}


@pytest.mark.fresh_process
def test_kernel_names(plan, image):
    lines = []
    for c in mc.ALL:
        pf, f = plan_facts(mc.program_set(c)), image[c.name]
        for flags in (0, _abi.X_MACRO_DIRECT):
            lines.append(run_line(C=c.C, n_groups=c.n_groups, n_programs=pf['n_programs'], straight=0, linear=1,
                                  reg_writes=1, macros=1, cmd_major=pf['cmd_major'], nr=f['nr'], addid=f['addid'],
                                  max_len=pf['max_len'], group_len=max(pf['group_len']), spg=c.spg, order=c.order,
                                  flags=flags, n_shots=c.n_shots))
    _, got = plan(lines)
    for i, c in enumerate(mc.ALL):
        assert got[2 * i]['name'] == c.kernel, (c.name, got[2 * i])
        assert got[2 * i + 1]['name'] == 'macro_kernel', (c.name, got[2 * i + 1])
    names = {c.kernel for c in mc.FAMILY_F}
    assert names == {'macro_staged_kernel<2>', 'macro_staged_kernel<2,12>', 'macro_staged_kernel<16>', 'macro_kernel',
                     'macro_staged_kernel<2,addid>', 'macro_staged_kernel<2,addid,12>'}
    assert mc.BY_NAME['f_spg4'].kernel == 'macro_kernel' and mc.BY_NAME['f_lds'].kernel == 'macro_staged_kernel<16>'


def test_trace_is_off():
    """both routes, and the two twins with the trace on"""
    off = [c for c in mc.ALL if not c.trace_on]
    assert {c.name for c in mc.ALL if c.trace_on} == set(mc.TRACE_TWINS)
    assert any(c.caps['trace_cap'] == 0 for c in off) and any(c.caps['trace_cap'] > 0 for c in off)
    for c in off:
        assert 'trace' not in c.outputs
    for c in mc.ALL:
        assert 256 <= c.n_shots <= 1300 and (c.n_groups == 1 or (6 <= c.n_groups <= 13 and 4 <= c.spg <= 32)), c.name


# ---------------------------------------------------------------- the timing model
@pytest.mark.parametrize('c', mc.ALL, ids=ids(mc.ALL))
def test_timing_model(c):
    """macro_cases.timing against oracle_fast on one period of the case's groups, max_cycles loose: event
    times (pulse reset at its decode, strobes at fire + 2), trace times (decode + 3) and t_end"""
    fz, ps = mc.fuzz_case(c), mc.program_set(c)
    cfg = mc.config(c, max_cycles=100000, event_cap=128, trace_cap=512, lane_order=_abi.LANES_CORE_MAJOR)
    n = c.spg * c.n_groups
    f = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, 0, n, want=('summary', 'events', 'trace'))
    s = _abi.unpack_summary(f['summary'])
    for g in range(c.n_groups):
        for k in range(c.C):
            L, w = k * n + g * c.spg, fz['progs'][g * c.C + k]
            tm = mc.timing(w)
            ev, tr = [], []
            for (D, _, tT, late), wd in zip(tm, w):
                if not late:
                    ev += [D] if mc.op4(wd) == 0xB else [tT + 2] if mc.op4(wd) == 0x9 else []
                    tr += [D + 3] if mc.op4(wd) in (1, 6) else []
            assert f['events'][:int(s['n_events'][L]), L, 0].tolist() == ev, (c.name, g, k)
            assert f['trace'][:int(s['n_trace'][L]), L, 0].tolist() == tr, (c.name, g, k)
            assert int(s['t_end'][L]) == tm[-1][0] and bool(s['flags'][L] & _abi.F_LATE) == tm[-1][3], (c.name, g, k)


@pytest.mark.parametrize('c', mc.FAMILY_F + SINGLE, ids=ids(mc.FAMILY_F + SINGLE))
def test_loose_max_cycles_passes_the_tests(c):
    """at the case's max_cycles every lean-candidate chunk of every program passes lean_chunk_ok (2
    registers), every simple macro simple_ok (3): the wave ballots then pass whatever programs a wave
    holds.  After inc_qclk by a negative value (g_single_incq_neg) no chunk passes: the no_wrap term"""
    for w in mc.fuzz_case(c)['progs']:
        slots = 3 if c.n_regs <= 2 else 2
        mac = mc.macros_of(w, slots)
        n_ok = 0
        if c.n_regs <= 2:
            bounds, v = mc.lean_bounds(w), mc.lean_chunk_verdicts(w, c.caps['max_cycles'])
            for ch, (_, _, b) in enumerate(bounds):
                wrapped = 'incq_neg' in c.name and ch > 2
                assert v[ch] == (b is not None and not wrapped), (c.name, ch)
                n_ok += v[ch]
            # (a late trigger's chunk passes too: pulse_lean stops the lane)
            assert n_ok == (1 if 'incq_neg' in c.name else 2 if c in SINGLE else (c.M - 1) // 16 - 1), c.name
        n_cmds = len(mc.timing(w))
        for j in range(1, len(mac) - 1):
            first = (mac[j][0] + [mac[j][1]])[0]
            if first < n_cmds:
                assert mc.macro_verdict(w, j, c.caps['max_cycles'], slots) == mc.is_simple(w, mac, j), (c.name, j)


@pytest.fixture(scope='module')
def summary():
    cache = {}

    def get(c, max_cycles=None):
        key = (c.name, max_cycles)
        if key not in cache:
            ps = mc.program_set(c)
            cfg = mc.config(c) if max_cycles is None else mc.config(c, max_cycles=max_cycles)
            out = oracle.fast_run(cfg, ps.words, ps.offsets, ps.n_instr, ps.table, c.shot0, c.n_shots,
                                  want=('summary',))
            cache[key] = _abi.unpack_summary(out['summary'])
        return cache[key]
    return get


def lane_programs(c):
    """per output lane: the index of the lane's program"""
    grp = np.array([((c.shot0 + s) // c.spg) % c.n_groups for s in range(c.n_shots)])
    idx = grp[None, :] * c.C + np.arange(c.C)[:, None]                 # [core, shot]
    return (idx.T if c.order == _abi.LANES_SHOT_MAJOR else idx).reshape(-1)


def chunk_of_ip(c, words, ip):
    """the chunk of the macro that holds command ip"""
    for j, (alus, slot) in enumerate(mc.macros_of(words, 3 if c.n_regs <= 2 else 2)):
        if ip in alus or ip == slot:
            return j // mc.CHUNK
    raise AssertionError(ip)


@pytest.mark.parametrize('c', mc.FAMILY_H, ids=ids(mc.FAMILY_H))
def test_sweep_windows_hold_the_flips(c, summary):
    progs = mc.fuzz_case(c)['progs']
    slots = 3 if c.n_regs <= 2 else 2
    # the per-macro window: t + SPAN of two macros and more of each program strictly inside, the verdict
    # False below and True from it on; lanes stopped by max_cycles at both ends of the window
    lo, n = mc.h_macro_window(c)
    for w in progs:
        mac, tm = mc.macros_of(w, slots), mc.timing(w)
        inside = [j for j in range(1, c.M - 1) if lo < tm[(mac[j][0] + [mac[j][1]])[0]][0] + 4 * slots < lo + n - 1]
        assert len(inside) >= 2, (c.name, inside)
        for j in inside:
            v = tm[(mac[j][0] + [mac[j][1]])[0]][0] + 4 * slots
            assert not mc.macro_verdict(w, j, v - 1, slots) and mc.macro_verdict(w, j, v, slots)
    for v in (lo, lo + n - 1):
        assert (summary(c, v)['status'] == _abi.ST_MAX_CYCLES).all(), c.name
    if c.n_regs > 2:
        return
    # the lean-chunk window: every bound strictly inside, the verdict flips there; below the earliest
    # bound no chunk passes, at the last value every candidate does
    lo, n = mc.h_window(c)
    assert n >= mc.H_WINDOW and (n == mc.H_WINDOW or c.M > 50)
    lanes = lane_programs(c)
    cut_chunks = set()
    for p, w in enumerate(progs):
        bounds = [(ch, b) for ch, (_, _, b) in enumerate(mc.lean_bounds(w)) if b is not None]
        assert len(bounds) == (c.M - 1) // 16 - 1 >= 2
        for ch, b in bounds:
            assert lo < b - 1 and b < lo + n - 1, (c.name, ch, b)
            assert mc.lean_chunk_verdicts(w, b - 1)[ch] is False and mc.lean_chunk_verdicts(w, b)[ch] is True
            # one below the bound: the lanes of a longer program stop in a later chunk
            s = summary(c, b - 1)
            for L in np.flatnonzero(s['status'] == _abi.ST_MAX_CYCLES)[:4]:
                cut_chunks.add((ch, chunk_of_ip(c, progs[lanes[L]], int(s['ip'][L]))))
        assert not any(mc.lean_chunk_verdicts(w, lo).values())
        assert sum(mc.lean_chunk_verdicts(w, lo + n - 1).values()) == len(bounds)
    assert cut_chunks, c.name
    if c.M > 50:
        # 80 macros: at the bounds of chunks 1 and 2 lanes stop inside a later lean-candidate chunk
        assert {(1, 2), (2, 3)} & cut_chunks or {(1, 3)} & cut_chunks, cut_chunks
        assert any(a in (1, 2) and b in (2, 3) for a, b in cut_chunks), cut_chunks


# ---------------------------------------------------------------- the lanes end as the cases need
@pytest.mark.parametrize('c', mc.FAMILY_F, ids=ids(mc.FAMILY_F))
def test_family_f_runs_long(c, summary):
    """90 % of the lanes and more end DONE having retired 100 commands and more (the cases of 33 macros,
    whose programs hold 66 to 126 commands: 66; f_late: of the lanes whose program has no late trigger)"""
    s = summary(c)
    keep = np.ones(len(s['status']), bool)
    if 'late' in c.reach:
        late = np.array([any(t[3] for t in mc.timing(w)) for w in mc.fuzz_case(c)['progs']])
        keep = ~late[lane_programs(c)]
        assert 0.3 < keep.mean() < 0.7
    need = 100 if c.M >= 47 else 2 * c.M
    assert ((s['status'] == _abi.ST_DONE) & (s['n_instr'] >= need))[keep].mean() >= 0.9, c.name


def test_family_f_endings(summary):
    c = mc.BY_NAME['f_meas']
    s = summary(c)
    both = _abi.F_MEAS_OVF | _abi.F_EVENT_OVF
    assert ((s['n_meas'] > 32) & (s['flags'] & both == both)).mean() >= 0.9
    assert c.caps['event_cap'] == 5 and c.caps['meas_cap'] == 4 and c.meas_elem == c.gen['elem']
    c = mc.BY_NAME['f_late']
    s = summary(c)
    late = (s['flags'] & _abi.F_LATE != 0) & (s['status'] == _abi.ST_MAX_CYCLES)
    done = s['status'] == _abi.ST_DONE
    assert (late | done).all() and late.any() and done.any()
    progs = mc.fuzz_case(c)['progs']
    for L in np.flatnonzero(late)[:50]:
        assert chunk_of_ip(c, progs[lane_programs(c)[L]], int(s['ip'][L])) == 2        # stopped inside chunk 2
    # shot-major lanes, C = 2: neighbouring lanes are the two cores of a shot, an even and an odd program
    assert c.order == _abi.LANES_SHOT_MAJOR and (late[0::2] != late[1::2]).all()
    # f_partial: block_core_major gives a workgroup BLOCK / C consecutive shots, a wave 64 of one core
    c = mc.BY_NAME['f_partial']
    S = mc.BLOCK // c.C
    rest = c.n_shots % S
    assert c.order == _abi.LANES_CORE_MAJOR and 0 < rest < 64 and S // 64 >= 2       # one partial wave, empty ones
    assert c.shot0 % c.spg != 0 and (c.shot0 // c.spg) % c.n_groups != 0
    t = mc.BY_NAME[mc.TRACE_TWINS['f_trace_on_vgpr']]
    assert mc.BY_NAME['f_partial'].gen == t.gen


# ---------------------------------------------------------------- oracle_fast against oracle_rtl
RTL_CASES = ['f_vgpr_47', 'f_lds', 'f_addid_wide', 'f_meas', 'g_single_incq_neg', 'g_fuzz_0', 'g_fuzz_6', 'h_vgpr']


@pytest.mark.parametrize('name', RTL_CASES)
def test_fast_vs_rtl_on_the_programs(name):
    """64 shots of the case (every group, the case's shots_per_group and first shot) through both oracles:
    all 8 ALU ops on 32-bit immediates and the register form of in0, register-sourced pulse fields,
    inc_qclk breakers, late triggers"""
    c = mc.BY_NAME[name]
    fz = mc.fuzz_case(c)
    cfg = mc.config(c, max_cycles=HORIZON, event_cap=EV_CAP, trace_cap=TR_CAP, meas_cap=MEAS_CAP,
                    lane_order=_abi.LANES_CORE_MAJOR)
    n_shots = 64
    words, offs, ni = pack_programs(fz['progs'])
    fast = oracle.fast_run(cfg, words, offs, ni, fz['table'], c.shot0, n_shots)
    scfg = oracle.shot_cfg_from_config(cfg)
    rtl = []
    for s in range(n_shots):
        g = ((c.shot0 + s) // c.spg) % c.n_groups
        progs = [np.asarray(isa.words_to_u32(fz['progs'][int(fz['table'][g * c.C + k])])) for k in range(c.C)]
        rtl.append(oracle.rtl_run_shot(scfg, progs, c.shot0 + s, HORIZON + 16, EV_CAP, TR_CAP, MEAS_CAP)[1])
    st = compare(cfg, fast, rtl, n_shots)
    assert st['done'] + st['other'] == n_shots * c.C and st['done'] > 0
