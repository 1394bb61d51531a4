// CPU driver of dpemu_qsim_decay's host part (csrc/launch_plan.h
// plan_qsim_decay), built and run by tests/test_qsim_decay_plan.py with g++,
// beside tests/qsim_plan_test.cpp: the device table of an accepted request and
// the refusals include/dpemu.h lists for the decay argument.  plan_qsim is
// untouched: its table and LDS bytes are what they are without a decay.
// Prints "ok <checks>" and returns 0, or the first failed check.
#include <cstdio>
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
    std::vector<uint32_t> damp, deph;
    dpemu_qsim_decay_args dec{};
    explicit Request(uint32_t C = 8)
    {
        cfg.cores_per_shot = C;
        for (uint32_t c = 0; c < C; c++)
            for (uint32_t i = 0; i < 32; i++) {
                damp.push_back((1u << 30) - (1000u * c + i));       // every entry differs; core 0 entry 0 is 2^30
                deph.push_back((1u << 30) >> ((c + i) % 31));
            }
        dec.t_final = 12345;
        sync();
    }
    void sync() { dec.damp = damp.data(); dec.deph = deph.data(); }
};

static bool refused(const std::function<void(Request &)> &edit, const char *word)
{
    Request r;
    edit(r);
    const QsimDecayPlan pl = plan_qsim_decay(&r.cfg, &r.dec);
    const bool found = pl.err.find(word) != std::string::npos && pl.tab.empty();
    if (!found) std::printf("expected '%s' in '%s'\n", word, pl.err.c_str());
    return found;
}

int main()
{
    CHECK(QSIM_DECAY_WORDS == 64);
    // ---- accepted: per core damp[32], then deph[32] ----
    for (uint32_t C : {1u, 8u, 64u}) {
        Request r(C);
        const QsimDecayPlan pl = plan_qsim_decay(&r.cfg, &r.dec);
        CHECK(pl.err.empty() && pl.tab.size() == (size_t)C * 64);
        if (C == 64) CHECK(pl.tab.size() * 4 == 16384);               // 16 KB at 64 cores
        for (uint32_t c = 0; c < C; c++)
            for (uint32_t i = 0; i < 32; i++) {
                CHECK(pl.tab[64 * c + i] == r.damp[32 * c + i]);
                CHECK(pl.tab[64 * c + 32 + i] == r.deph[32 * c + i]);
            }
    }
    {   // the bounds themselves: 0 and 2^30
        Request r;
        r.damp[5] = 0; r.deph[255] = 1u << 30; r.damp[0] = 1u << 30; r.dec.t_final = 0;
        CHECK(plan_qsim_decay(&r.cfg, &r.dec).err.empty());
        r.dec.t_final = 0xFFFFFFFFu;
        CHECK(plan_qsim_decay(&r.cfg, &r.dec).err.empty());
    }
    // ---- the refusals ----
    {
        Request r;
        const QsimDecayPlan pl = plan_qsim_decay(&r.cfg, nullptr);
        CHECK(pl.err.find("dec is NULL") != std::string::npos && pl.tab.empty());
    }
    CHECK(refused([](Request &r) { r.dec.damp = nullptr; }, "damp is NULL"));
    CHECK(refused([](Request &r) { r.dec.deph = nullptr; }, "deph is NULL"));
    CHECK(refused([](Request &r) { r.damp[0] = (1u << 30) + 1; }, "damp: entry 0 of core 0"));
    CHECK(refused([](Request &r) { r.damp[32 * 7 + 31] = 0xFFFFFFFFu; }, "damp: entry 31 of core 7"));
    CHECK(refused([](Request &r) { r.deph[32 * 3 + 9] = (1u << 30) + 1; }, "deph: entry 9 of core 3"));
    CHECK(refused([](Request &r) { r.deph[32 * 3 + 9] = 0x80000000u; }, "2^30"));
    CHECK(refused([](Request &r) { r.cfg.cores_per_shot = 0; }, "cores_per_shot"));
    CHECK(refused([](Request &r) { r.cfg.cores_per_shot = 65; }, "cores_per_shot"));
    {   // entries of cores past cores_per_shot are not read
        Request r(8);
        r.cfg.cores_per_shot = 4;
        r.damp[32 * 4] = 0xFFFFFFFFu;
        const QsimDecayPlan pl = plan_qsim_decay(&r.cfg, &r.dec);
        CHECK(pl.err.empty() && pl.tab.size() == 4 * 64);
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
