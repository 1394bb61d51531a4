"""The per-call choices of the entry points (csrc/launch_plan.h) on the CPU:
which kernel a run launches (the names the GPU tests pin through
dpemu_last_kernel), its LDS words, the histogram plan, the DDS record-LDS plan
and the iq_stats grid.  tests/launch_plan_test.cpp prints the plan of every
request line; the assertions are here."""

import os
import re
import shutil
import subprocess

import pytest

from distributed_processor_amd import _abi

HERE = os.path.dirname(os.path.abspath(__file__))


def run_line(C=2, n_groups=1, n_programs=None, straight=0, linear=1, fproc=0, sync=0, reg_writes=1, macros=1,
             cmd_major=1, nr=2, addid=0, max_len=100, group_len=None, spg=1, order=0, flags=0, model=0, fproc_mode=0,
             n_shots=1000, hist=0):
    n_programs = n_groups * C if n_programs is None else n_programs
    group_len = C * (max_len + 1) if group_len is None else group_len
    return 'run {} {} {} {} {} {} {} {} {} {} {} {} {} {} | {} {} {} {} {} {} {}'.format(
        C, n_groups, n_programs, straight, linear, fproc, sync, reg_writes, macros, cmd_major, nr, addid, max_len,
        group_len, spg, order, flags, model, fproc_mode, n_shots, hist)


@pytest.fixture(scope='module')
def plan(tmp_path_factory):
    if shutil.which('g++') is None:
        pytest.skip('g++ not available')
    d = tmp_path_factory.mktemp('plan')
    exe = str(d / 'launch_plan_test')
    subprocess.run(['g++', '-std=c++17', '-O1', '-Wall', '-o', exe, os.path.join(HERE, 'launch_plan_test.cpp')],
                   check=True)

    def ask(lines):
        path = str(d / 'requests.txt')
        with open(path, 'w') as fh:
            fh.write('\n'.join(lines) + '\n')
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr
        out = []
        for ln in r.stdout.strip().splitlines():
            out.append({k: (v if k == 'name' else int(v)) for k, v in re.findall(r'(\w+)=(\S+)', ln)})
        assert len(out) == len(lines) + 1, r.stdout[-2000:]
        return out[0], out[1:]
    return ask


@pytest.mark.fresh_process        # runs g++ and a binary: before any test touches the GPU (tests/conftest.py)
def test_macro_kernel_names(plan):
    """the `need` formula of test_gpu_parity.py::test_fuzz_linear_few_registers over its grid, and
    the names test_gpu_rb.py pins for the RB tables"""
    lines, want = [], []
    for C in (1, 2, 4):
        for order in (0, 1):
            for spg in (10, 16, 32, 5):
                for nr in (2, 16):              # 1-2 named registers: the VGPR file; 3-4: the LDS file
                    shots_run = 64 // C if order else min(256 // C, 64)
                    cores_w = C if order else 64 // shots_run
                    need = (-(-(shots_run - 1) // spg) + 1) * cores_w
                    lines.append(run_line(C=C, n_groups=32, spg=spg, order=order, nr=nr, n_shots=64 * 9))
                    want.append('macro_kernel' if need > 12 or (need > 8 and nr != 2) else
                                'macro_staged_kernel<2,12>' if need > 8 else 'macro_staged_kernel<{}>'.format(nr))
    # test_rb_lean_path_edges: 96 sequences x 10 shots, both lane orders
    for order, name in ((0, 'macro_staged_kernel<2,addid>'), (1, 'macro_staged_kernel<2,addid,12>')):
        lines.append(run_line(C=2, n_groups=96, spg=10, order=order, addid=1, n_shots=960))
        want.append(name)
    # test_fewer_shots_per_sequence: 3000 sequences with 8 / 6 / 4 shots each
    for spg, name in ((8, 'macro_staged_kernel<2,addid,12>'), (6, 'macro_staged_kernel<2,addid,12>'),
                      (4, 'macro_kernel')):
        lines.append(run_line(C=2, n_groups=3000, spg=spg, addid=1, n_shots=3000 * spg))
        want.append(name)
    lines.append(run_line(C=2, n_groups=96, spg=10, addid=1, flags=_abi.X_MACRO_DIRECT))
    want.append('macro_kernel')
    _, got = plan(lines)
    for ln, g, w in zip(lines, got, want):
        assert g['name'] == w, (ln, g)
        assert g['lds'] == 0, (ln, g)           # the macro kernels stage their own chunks


@pytest.mark.fresh_process
def test_other_kernel_names_and_lds_words(plan):
    lines = [
        run_line(model=2),                                               # 0 DEMOD: branch_kernel with FEAT_DEMOD
        run_line(model=2, straight=1, reg_writes=0, macros=0),           # 1 ... pulse-only programs too
        run_line(straight=1, reg_writes=0, macros=0, max_len=20),        # 2 pulse-only, short: rows
        run_line(straight=1, reg_writes=0, macros=0, max_len=200),       # 3 pulse-only, long: LDS
        run_line(straight=1, reg_writes=0, macros=0, max_len=200, cmd_major=0),   # 4
        run_line(straight=1, reg_writes=0, macros=0, max_len=5000, n_shots=10 ** 6),   # 5 too long for the LDS share
        run_line(straight=1, reg_writes=0, macros=0, max_len=65536),     # 6 ip could wrap: not the straight kernel
        run_line(flags=_abi.X_GENERAL),                                  # 7
        run_line(flags=_abi.X_GENERAL | _abi.X_PROG_LDS, max_len=30),    # 8 the interpreter stages on request
        run_line(flags=_abi.X_PROG_LDS, max_len=3000),                   # 9 ... within 16 KiB
        run_line(linear=0, macros=0, fproc=1, sync=1, max_len=30, C=8),        # 10 branch, staged: 8 x 31 commands
        run_line(linear=0, macros=0, fproc=1, fproc_mode=1, max_len=2000),                        # 11 branch, too long
        run_line(linear=0, macros=0, max_len=30, flags=_abi.X_PROG_MAJOR),                        # 12
    ]
    caps, got = plan(lines)
    assert got[0]['name'].startswith('branch_kernel<') and got[0]['bfeat'] & 0x40
    assert got[1]['name'].startswith('branch_kernel<') and got[1]['bfeat'] & 0x40
    assert got[2]['name'] == 'straight_kernel<rows,fb4>' and got[2]['lds'] == 0
    assert got[3]['name'] == 'straight_kernel<lds,fb4>' and got[3]['lds'] > 0
    assert got[4]['name'] == 'straight_kernel<lds,fb4>'
    assert got[5]['name'] == 'straight_kernel<rows,fb1>' and got[5]['lds'] == 0
    assert got[6]['name'].startswith('branch_kernel<')
    assert got[7]['name'].startswith('interp_kernel<') and got[7]['lds'] == 0
    assert got[8]['name'] == 'interp_kernel<feat=0x8>' and got[8]['lds'] > 0
    assert got[9]['name'] == 'interp_kernel<feat=0x0>' and got[9]['lds'] == 0
    assert got[10]['name'] == 'branch_kernel<feat=0x2b,c8>' and got[10]['lds'] > 0     # fproc | sync | prog_lds | regs
    assert got[11]['name'] == 'branch_kernel<feat=0x24>' and got[11]['lds'] == 0       # lut | regs
    assert got[12]['name'] == 'branch_kernel<feat=0x20>' and got[12]['lds'] == 0 and got[12]['cm'] == 0
    cap = {0: caps['straight'], 2: caps['branch'], 3: caps['interp']}                  # by RunPlan::family
    for ln, g in zip(lines, got):
        if g['lds']:
            assert g['lds'] % 16 == 0 and 16 <= g['lds'] <= cap[g['family']], (ln, g)


@pytest.mark.fresh_process
def test_histogram_plan(plan):
    lines = []
    for C in (1, 2, 8, 12):
        for ng in (1, 100, 100000):
            for n_shots in (1, 300, 10 ** 6):
                for flags in (0, _abi.X_HIST_REPL, _abi.X_HIST_DIRECT):
                    lines.append(run_line(C=C, n_groups=ng, spg=10, linear=0, macros=0, hist=1, flags=flags,
                                          n_shots=n_shots))
    lines.append(run_line(hist=0))
    _, got = plan(lines)
    assert got[-1]['repl'] == 0 and got[-1]['bins'] == 0
    some_repl = some_direct = False
    for ln, g in zip(lines[:-1], got):
        flags = int(ln.split('|')[1].split()[2])
        C, ng = int(ln.split()[1]), int(ln.split()[2])
        assert g['bins'] == ng << C, (ln, g)
        if flags & _abi.X_HIST_DIRECT:
            assert g['repl'] == 0, (ln, g)
        if flags & _abi.X_HIST_REPL:
            assert g['repl'] == 1, (ln, g)
        if g['repl']:
            assert g['stride'] % 32 == 0 and g['stride'] >= g['bins'] and g['R'] >= 1, (ln, g)
            assert g['R'] * g['stride'] * 4 <= 2 << 20 or g['R'] == 1, (ln, g)
            assert g['R'] <= 64
        some_repl |= flags == 0 and g['repl'] == 1
        some_direct |= flags == 0 and g['repl'] == 0
    assert some_repl and some_direct            # the default takes both ways over this grid


@pytest.mark.fresh_process
def test_dds_and_iq_plans(plan):
    lines, kinds = [], []
    for cap in (8, 200, 700, 1024):
        for n_samples in (4096, 40000, 100000):
            lines.append('dds {} {} 4 1 64 8'.format(cap, n_samples))
            kinds.append('small')
    lines.append('dds 700 40000 4 1 4000 8')    # a 32-KiB envelope leaves the records neither budget
    kinds.append('big')
    iq = [(1, 1, 1), (10 ** 6, 2, 1), (10 ** 6, 64, 32), (10 ** 7, 1, 1)]
    lines += ['iq {} {} {} 4 256'.format(n, C, S) for n, C, S in iq]
    caps, got = plan(lines)
    for ln, kind, g in zip(lines, kinds, got):
        cap = int(ln.split()[1])
        assert g['ev_lds'] % 8 == 0 and g['ev_lds'] >= max(cap, 8), (ln, g)
        assert g['stripes'] * g['wg_tiles'] >= g['tiles'] >= 1, (ln, g)
        assert g['rec_lds'] <= g['ev_lds']
        if g['dense']:
            assert g['rec_lds'] == g['ev_lds'] and g['bytes'] <= caps['dds_dense'], (ln, g)
        else:
            assert g['bytes'] <= caps['dds_budget'] or g['rec_lds'] == caps['rec_min'], (ln, g)
        # every record staged exactly when that fits the 20-KiB budget or the dense branch was taken
        assert (g['rec_lds'] == g['ev_lds']) == bool(g['dense'] or g['all_bytes'] <= caps['dds_budget']), (ln, g)
        if kind == 'small':
            assert bool(g['dense']) == (cap >= 700), (ln, g)
        else:
            assert not g['dense'] and g['rec_lds'] == caps['rec_min'] < g['ev_lds'], (ln, g)
    for (n, C, S), g in zip(iq, got[len(kinds):]):
        per_wg = max(256, 128 * C)
        assert g['gx'] == max(1, min(-(-n // per_wg), max(1, 4 * 256 // S))), (n, C, S, g)
