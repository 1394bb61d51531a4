"""Resource guard of the branch_kernel variants that take supplied states
(FEAT_STATES = 128, csrc/branch_states.hip; dpemu_run_states), on the CPU.
tests/test_kernel_resources.py already holds every _ZN5dpemu kernel, these
included, to no scratch and no flat_* instruction; its occupancy floors are
keyed by mangled-name substrings that the new variants' names do not contain,
so theirs are here: each variant keeps the floor of its base (the same FEAT
without bit 128), whose Philox state draw it trades for one loaded word.

* all 48 instantiations exist: the six fproc / sync / LUT cases x {none,
  FEAT_REGS, FEAT_PROG_LDS, both} x CT in {0, 8};
* branch_kernel<11 | 128, 8> (config 3's shape) allows 6 waves per SIMD, the
  floor of <11, 8>; <14 | 128, 8> (config 3 through the LUT) 7, the floor of <14, 8>."""

from tests.test_kernel_resources import (code_objects, memory_instrs, product_kernels,  # noqa: F401 (the fixture,
                                         pytestmark, waves_per_simd)                  # the module's marks)

FEAT_FPROC, FEAT_SYNC, FEAT_LUT, FEAT_PROG_LDS, FEAT_REGS, FEAT_STATES = 1, 2, 4, 8, 32, 128
CASES = (0, FEAT_FPROC, FEAT_SYNC, FEAT_FPROC | FEAT_SYNC, FEAT_LUT, FEAT_LUT | FEAT_SYNC)
EXTRAS = (0, FEAT_REGS, FEAT_PROG_LDS, FEAT_REGS | FEAT_PROG_LDS)
FLOORS = {'branch_kernelILi139ELi8E': 6,       # config 3 under co-simulation (base <11,8>: 6)
          'branch_kernelILi142ELi8E': 7}       # ... through the LUT (base <14,8>: 7)


def symbol(feat, ct):
    return '_ZN5dpemu13branch_kernelILi{}ELi{}EEEvNS_7KParamsE'.format(feat, ct)


def test_all_48_states_variants_exist(code_objects):
    ks = product_kernels(code_objects)
    want = [symbol(FEAT_STATES | c | x, ct) for c in CASES for x in EXTRAS for ct in (0, 8)]
    assert len(set(want)) == 48
    missing = [s for s in want if s not in ks]
    assert not missing, missing
    # and no others carry the bit (DEMOD with supplied states is refused, not instantiated)
    extra = [k for k in ks if 'branch_kernelILi' in k and int(k.split('branch_kernelILi')[1].split('E')[0]) & FEAT_STATES
             and k not in want]
    assert not extra, extra


def test_states_variants_keep_their_bases_floors(code_objects):
    ks = product_kernels(code_objects)
    for sub, floor in FLOORS.items():
        names = [k for k in ks if sub in k]
        assert len(names) == 1, (sub, names)
        m = ks[names[0]]
        w = waves_per_simd(m['vgpr_count'], m.get('agpr_count', 0))
        assert w >= floor, (names[0], 'VGPRs {} -> {} waves / SIMD < {}'.format(m['vgpr_count'], w, floor))


def test_states_variants_use_no_scratch_and_no_flat(code_objects):
    """(test_kernel_resources.py covers these too; here by name, so a renamed unit cannot drop out unseen)"""
    ks = product_kernels(code_objects)
    mine = {k: m for k, m in ks.items() if 'branch_kernelILi' in k
            and int(k.split('branch_kernelILi')[1].split('E')[0]) & FEAT_STATES}
    assert len(mine) == 48
    for k, m in mine.items():
        assert m.get('private_segment_fixed_size', 0) == 0 and m.get('vgpr_spill_count', 0) == 0, (k, m)
    seen = 0
    for co in code_objects:
        for name, (n_scratch, n_flat) in memory_instrs(co).items():
            if name in mine:
                seen += 1
                assert n_scratch == 0 and n_flat == 0, (name, n_scratch, n_flat)
    assert seen == 48
