// CPU driver of dpemu_qsim_meas's host part (csrc/launch_plan.h plan_qsim with
// meas set), built and run by tests/test_qsim_meas.py with g++: the two
// refusals the measuring call adds, that dpemu_qsim's plan does not make them,
// and that both calls build the same device table.  Prints "ok <checks>" and
// returns 0, or the first failed check.
#include <cstdio>
#include <vector>

#include "../distributed_processor_amd/csrc/launch_plan.h"

using namespace dpemu;

static int n_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        n_checks++;                                                        \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

int main()
{
    dpemu_config cfg{};
    cfg.cores_per_shot = 4;
    cfg.meas_elem = 2;
    std::vector<uint32_t> reg = {0, 1, 2, 0xFFFFFFFFu};
    dpemu_qsim_gate g{};
    g.core = 2; g.freq = 1; g.env = 0x040000; g.amp = 100; g.m[0][0] = 1 << 30; g.m[0][6] = 1 << 30;
    dpemu_qsim_args qs{};
    qs.n_regs = 2; qs.reg_core = reg.data(); qs.n_gates = 1; qs.gates = &g;
    qs.drv_elem = 0; qs.event_cap = 16; qs.n_shots = 70; qs.n_lanes = 280;

    const QsimPlan base = plan_qsim(&cfg, &qs), meas = plan_qsim(&cfg, &qs, true);
    CHECK(base.err.empty() && meas.err.empty());
    CHECK(base.tab == meas.tab && base.lds_bytes == meas.lds_bytes);          // one uploaded table serves both calls
    CHECK(base.off_reg == meas.off_reg && base.off_slot == meas.off_slot && base.off_det == meas.off_det &&
          base.off_dict == meas.off_dict);

    for (uint32_t e : {4u, 0xFFu, 0xFFFFFFFFu}) {                             // meas_elem > 3 (0xFF: "none" of dpemu_run)
        cfg.meas_elem = e;
        CHECK(plan_qsim(&cfg, &qs, true).err.find("meas_elem") != std::string::npos);
        CHECK(plan_qsim(&cfg, &qs).err.empty());                              // dpemu_qsim does not read it
    }
    for (uint32_t e = 0; e < 4; e++) {                                        // meas_elem == drv_elem
        cfg.meas_elem = e;
        for (uint32_t d = 0; d < 4; d++) {
            qs.drv_elem = d;
            const QsimPlan pl = plan_qsim(&cfg, &qs, true);
            CHECK(pl.err.empty() == (d != e));
            CHECK(d != e || pl.err.find("drive element") != std::string::npos);
            CHECK(plan_qsim(&cfg, &qs).err.empty());
        }
    }
    cfg.meas_elem = 2; qs.drv_elem = 4;                                       // dpemu_qsim's own refusals still come first
    CHECK(plan_qsim(&cfg, &qs, true).err.find("drv_elem") != std::string::npos);
    qs.drv_elem = 0; qs.n_shots = 0; qs.n_lanes = 0;
    CHECK(plan_qsim(&cfg, &qs, true).err.empty());                            // no shots: still checked, accepted
    cfg.meas_elem = 0;
    CHECK(!plan_qsim(&cfg, &qs, true).err.empty());
    std::printf("ok %d\n", n_checks);
    return 0;
}
