"""Every branch_kernel<FEAT, CT> and interp_kernel<F> instantiation of
libdpemu.so, launched once and compared bit for bit with oracle_fast.

The rows are tests/feature_cases.py's INSTANTIATIONS: one program set per
instantiation, its facts rewritten to exactly the instantiation's feature bits.
tests/test_feature_cases.py checks on the CPU that the rows are all the
instantiations that are built, that each plans the kernel it claims and reaches
the code its bits switch; here each row runs, dpemu_last_kernel must be that
kernel, and every output array must equal the oracle's:

* state: dpemu_run with the plain config;
* demod: the DEMOD model with random parameters and frequency tables, the
  accumulated {I, Q} included;
* states: dpemu_run_states by draw equivalence, as
  tests/test_gpu_run_states.py does it: under seed A with the words of seed B's
  draws, against the oracle under seed B.

straight_kernel and the macro kernels are out of scope here:
tests/test_gpu_staging.py and tests/test_gpu_macro_paths.py assert their names
case by case, and their large-grid fb1 variants need grids far beyond a few
hundred lanes."""

import pytest

from distributed_processor_amd.emulator import Emulator
from tests import feature_cases as fc
from tests.feature_cases import INSTANTIATIONS, SEED_A, SEED_B

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def emu():
    e = Emulator(0)
    yield e
    e.close()


@pytest.mark.parametrize('r', INSTANTIATIONS, ids=[fc.row_id(r) for r in INSTANTIATIONS])
def test_instantiation_equals_the_oracle(emu, r):
    ps = fc.programs_of_row(r)
    cfg, tables = fc.config_of_row(r, ps, SEED_A)
    outs, shot0 = fc.outs_of(cfg), fc.shot0_of(r)
    states = None
    if r.model == 'states':
        want = fc.oracle_of_row(r, SEED_B)
        cfg_b, _ = fc.config_of_row(r, ps, SEED_B)
        n_meas = want['summary'].reshape(-1, 8)[:, 5]
        assert n_meas.max() <= 32, n_meas.max()         # every readout's state is a bit of the lane's word
        states = fc.drawn_states(cfg_b, r.n_shots, shot0, max(1, int(n_meas.max())))
    else:
        want = fc.oracle_of_row(r, SEED_A)
    assert set(want) == set(outs), (sorted(want), outs)
    if emu.programs is not ps:
        emu.load(ps)
    if tables is not None:
        emu.load_readout_freqs(cfg.ro_drv_elem, cfg.meas_elem, tables=tables)
    got = fc.device_run(emu, ps, cfg, r.n_shots, shot0, states, outs)
    assert emu.last_kernel() == fc.kernel_name(r)
    fc.compare(got, want, fc.row_id(r))
