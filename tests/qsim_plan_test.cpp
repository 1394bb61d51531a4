// CPU driver of dpemu_qsim's host part (csrc/launch_plan.h plan_qsim,
// qsim_phase_lut), built and run by tests/test_qsim_plan.py with g++: the
// device table of an accepted request, and every refusal include/dpemu.h
// lists.  Prints "ok <checks>" and returns 0, or the first failed check.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../distributed_processor_amd/csrc/launch_plan.h"

using namespace dpemu;

static int n_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        n_checks++;                                                        \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

struct Request {
    dpemu_config cfg{};
    std::vector<uint32_t> reg = {0, 1, 3, 0xFFFFFFFFu, 5, 2};   // (0, 1), 3 alone, (5, 2)
    std::vector<dpemu_qsim_gate> gates;
    std::vector<uint32_t> detune = std::vector<uint32_t>(8, 0u);
    dpemu_qsim_args qs{};
    Request()
    {
        cfg.cores_per_shot = 8;
        for (uint32_t core : {0u, 1u, 2u, 3u, 5u})
            for (uint32_t k = 0; k < 3; k++) {
                dpemu_qsim_gate g{};
                g.core = core; g.freq = k; g.env = 0x040000; g.amp = 100 + core;
                g.kind = (k == 1 && (core == 0 || core == 5)) ? 1 : 0;
                g.err_thr = k;
                for (int i = 0; i < 2; i++) { g.m[i][0] = 1 << 30; g.m[i][6] = -(1 << 30); g.m[i][3] = 7 + (int)core; }
                gates.push_back(g);
            }
        detune[3] = 0xDEADBEEFu;
        qs.drv_elem = 0; qs.event_cap = 24; qs.shot_begin = 5; qs.n_shots = 70;
        sync();
    }
    void sync()
    {
        qs.n_regs = (uint32_t)(reg.size() / 2); qs.reg_core = reg.data();
        qs.n_gates = (uint32_t)gates.size(); qs.gates = gates.data();
        qs.detune = detune.data();
        qs.n_lanes = (uint32_t)(qs.n_shots * cfg.cores_per_shot);
    }
};

static bool refused(const std::function<void(Request &)> &edit, const char *word)
{
    Request r;
    edit(r);
    const QsimPlan pl = plan_qsim(&r.cfg, &r.qs);
    const bool found = pl.err.find(word) != std::string::npos;
    if (!found) std::printf("expected '%s' in '%s'\n", word, pl.err.c_str());
    return found;
}

int main()
{
    // ---- the phase table ----
    std::vector<int32_t> lut(QSIM_LUT_WORDS);
    qsim_phase_lut(lut.data());
    CHECK(lut[0] == 1 << 30 && lut[1] == 0 && lut[2 * 128] == 0 && lut[2 * 128 + 1] == 1 << 30);
    CHECK(lut[2 * 256] == -(1 << 30) && lut[2 * 256 + 1] == 0 && lut[2 * 384] == 0 && lut[2 * 384 + 1] == -(1 << 30));
    CHECK(lut[2 * 512] == 1 << 30 && lut[2 * 512 + 1] == 0);
    CHECK(lut[2 * 64] == lut[2 * 64 + 1] && lut[2 * 64] == 759250125);          // 2^30 / sqrt(2), rounded

    // ---- an accepted request: the table ----
    {
        Request r;
        const QsimPlan pl = plan_qsim(&r.cfg, &r.qs);
        CHECK(pl.err.empty());
        CHECK(pl.off_reg == QSIM_LUT_WORDS && pl.off_slot == pl.off_reg + 6 && pl.off_det == pl.off_slot + 4);
        CHECK(pl.off_dict == pl.off_det + 64 && pl.tab.size() == pl.off_dict + 5 * QSIM_SLOT_WORDS);
        CHECK(!memcmp(pl.tab.data(), lut.data(), QSIM_LUT_WORDS * 4));
        const uint32_t want_slots[4] = {0, 2, 3, 5};
        CHECK(!memcmp(&pl.tab[pl.off_slot], want_slots, sizeof want_slots));
        CHECK(!memcmp(&pl.tab[pl.off_reg], r.reg.data(), 6 * 4));
        CHECK(pl.tab[pl.off_det + 3] == 0xDEADBEEFu && pl.tab[pl.off_det + 2] == 0 && pl.tab[pl.off_det + 8] == 0);
        // slots in register order: cores 0, 1, 3, 5, 2; three entries each, then unused ones
        const uint32_t cores[5] = {0, 1, 3, 5, 2};
        for (uint32_t s = 0; s < 5; s++)
            for (uint32_t k = 0; k < DPEMU_QSIM_GATES_MAX; k++) {
                const uint32_t *e = &pl.tab[pl.off_dict + s * QSIM_SLOT_WORDS + k * QSIM_GATE_WORDS];
                if (k < 3)
                    CHECK(e[0] == cores[s] && e[1] == k && e[2] == 0x040000 && e[3] == 100 + cores[s] && e[5] == k &&
                          (int32_t)e[6] == 1 << 30 && (int32_t)e[6 + 3] == 7 + (int32_t)cores[s] &&
                          (int32_t)e[6 + 8 + 6] == -(1 << 30));
                else
                    CHECK(e[1] == QSIM_NO_GATE);
            }
        // 70 shots: 256 rows span at most 255 / 70 + 2 = 5 > 3 registers: all 5 slots
        CHECK(pl.lds_bytes == (QSIM_LUT_WORDS + 5 * QSIM_SLOT_WORDS) * 4);
        r.qs.n_shots = 1000; r.sync();
        CHECK(plan_qsim(&r.cfg, &r.qs).lds_bytes == (QSIM_LUT_WORDS + 3 * QSIM_SLOT_WORDS) * 4);   // 2 registers: (0, 1), 3
        r.qs.detune = nullptr;
        const QsimPlan p2 = plan_qsim(&r.cfg, &r.qs);
        CHECK(p2.err.empty() && p2.tab[p2.off_det + 3] == 0);
        r.qs.n_shots = 0; r.sync();
        CHECK(plan_qsim(&r.cfg, &r.qs).err.empty());                               // no shots: still checked, accepted
    }

    // ---- 64 cores: the dictionary slots a workgroup's 256 rows can touch, up to all 64 (51,200 B) ----
    for (uint32_t two = 0; two < 2; two++) {
        Request r;
        r.cfg.cores_per_shot = 64;
        r.reg.clear();
        r.gates.clear();
        r.detune.assign(64, 0u);
        for (uint32_t k = 0; k < 64; k++) {               // the cores in a shuffled order: 37 k + 5 mod 64
            const uint32_t core = (37 * k + 5) % 64;
            r.reg.push_back(core);
            if (!two) r.reg.push_back(0xFFFFFFFFu);
            dpemu_qsim_gate g{};
            g.core = core; g.freq = 1; g.env = 0x040000; g.amp = 100 + core;
            g.kind = (two && k % 2 == 0) ? 1 : 0;           // the first core of a two-qubit register
            r.gates.push_back(g);
        }
        const uint32_t shots[3] = {1, 5, 37};
        const uint32_t slots[2][3] = {{64, 53, 8}, {64, 64, 16}};   // min(n_regs, 255 / n_shots + 2) registers' worth
        for (uint32_t i = 0; i < 3; i++) {
            r.qs.n_shots = shots[i];
            r.sync();
            const QsimPlan pl = plan_qsim(&r.cfg, &r.qs);
            CHECK(pl.err.empty());
            CHECK(pl.lds_bytes == (QSIM_LUT_WORDS + slots[two][i] * QSIM_SLOT_WORDS) * 4);
            if (slots[two][i] == 64) CHECK(pl.lds_bytes == 51200);
            CHECK(pl.tab[pl.off_slot + r.qs.n_regs] == 64 && pl.tab.size() == pl.off_dict + 64 * QSIM_SLOT_WORDS);
            CHECK(pl.tab[pl.off_slot + 1] == (two ? 2u : 1u));
        }
        CHECK(QSIM_LUT_WORDS == 1536 && QSIM_SLOT_WORDS == 176);
    }

    // ---- the refusals ----
    CHECK(refused([](Request &r) { r.qs.n_regs = 0; }, "n_regs"));
    CHECK(refused([](Request &r) { r.qs.reg_core = nullptr; }, "reg_core"));
    CHECK(refused([](Request &r) { r.qs.gates = nullptr; }, "gates"));
    CHECK(refused([](Request &r) { r.reg[4] = 8; }, "core 8"));
    CHECK(refused([](Request &r) { r.reg[3] = 0; }, "two registers"));
    CHECK(refused([](Request &r) { r.reg[5] = 5; }, "two registers"));
    CHECK(refused([](Request &r) { r.reg[0] = 0xFFFFFFFFu; }, ">= cores_per_shot"));   // only the second may be absent
    CHECK(refused([](Request &r) {
        for (uint32_t k = 3; k < 9; k++) { dpemu_qsim_gate g = r.gates[0]; g.freq = k; r.gates.push_back(g); }
        r.sync();
    }, "more than 8 entries for core 0"));
    CHECK(refused([](Request &r) { r.gates.push_back(r.gates[4]); r.sync(); }, "key"));
    CHECK(refused([](Request &r) { r.gates[2].kind = 2; }, "kind 2"));
    CHECK(refused([](Request &r) { r.gates[3].kind = 1; }, "kind 1"));       // core 1: the second of (0, 1)
    CHECK(refused([](Request &r) { r.gates[6].kind = 1; }, "kind 1"));       // core 2: the second of (5, 2)
    CHECK(refused([](Request &r) { r.gates[9].kind = 1; }, "kind 1"));       // core 3: a one-qubit register
    CHECK(refused([](Request &r) { r.gates[0].core = 4; }, "no register"));
    CHECK(refused([](Request &r) { r.gates[0].core = 64; }, "no register"));
    CHECK(refused([](Request &r) { r.gates[5].m[1][7] = (1 << 30) + 1; }, "2^30"));
    CHECK(refused([](Request &r) { r.gates[5].m[0][0] = -(1 << 30) - 1; }, "2^30"));
    CHECK(refused([](Request &r) { r.qs.drv_elem = 4; }, "drv_elem"));
    CHECK(refused([](Request &r) { r.qs.event_cap = DPEMU_MAX_EVENT_CAP + 1; }, "event_cap"));
    CHECK(refused([](Request &r) { r.qs.n_lanes += 1; }, "n_lanes"));
    CHECK(refused([](Request &r) { r.cfg.cores_per_shot = 6; }, "cores_per_shot"));
    CHECK(refused([](Request &r) { r.cfg.lane_order = 2; }, "lane_order"));
    CHECK(refused([](Request &r) {             // five one-qubit registers x (2^29 - 1) shots: the lanes fit, the rows do not
        const uint32_t none = 0xFFFFFFFFu;
        r.reg = {0, none, 1, none, 2, none, 3, none, 4, none};
        r.qs.n_shots = (1ull << 29) - 1;
        r.sync();
    }, "2^31"));
    {   // the bounds themselves are accepted
        Request r;
        r.gates[5].m[1][7] = 1 << 30; r.gates[5].m[0][0] = -(1 << 30); r.qs.drv_elem = 3;
        r.qs.event_cap = DPEMU_MAX_EVENT_CAP;
        for (uint32_t k = 3; k < 8; k++) { dpemu_qsim_gate g = r.gates[0]; g.freq = k; r.gates.push_back(g); }
        r.sync();
        CHECK(plan_qsim(&r.cfg, &r.qs).err.empty());
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
