// CPU driver of the entry points' host half (csrc/stage_plan.h), built and run
// by tests/test_stage_plan.py with g++: every refusal of dpemu_run's config,
// dpemu_dds, dpemu_demod_iq, the feedline stages and dpemu_iq_stats that needs
// no device pointer, which of two violated rules wins, the tables of accepted
// requests (written out here from the layouts in uop.h and kernels.h), and the
// boundary values that are still accepted.  Prints "ok <checks>" and returns 0,
// or the first failed check.
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "../distributed_processor_amd/csrc/stage_plan.h"

using namespace dpemu;

static int n_checks = 0;
#define CHECK(...)                                                         \
    do {                                                                   \
        n_checks++;                                                        \
        if (!(__VA_ARGS__)) { std::printf("line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } \
    } while (0)

static bool says(const Refusal &r, int code, const char *word)
{
    const bool found = r.code == code && r.err.find(word) != std::string::npos;
    if (!found) std::printf("expected %d '%s', got %d '%s'\n", code, word, r.code, r.err.c_str());
    return found;
}
static bool invalid(const Refusal &r, const char *word) { return says(r, DPEMU_E_INVALID, word); }
static bool accepted(const Refusal &r)
{
    if (r.refused() || !r.err.empty()) std::printf("refused: %d '%s'\n", r.code, r.err.c_str());
    return !r.refused() && r.err.empty();
}
template <class T> static bool same(const std::vector<T> &got, const std::vector<T> &want)
{
    if (got != want) {
        std::printf("table of %zu words, expected %zu:", got.size(), want.size());
        for (const T &v : got) std::printf(" %lld", (long long)v);
        std::printf("\n");
    }
    return got == want;
}

constexpr uint32_t NONE = 0xFFFFFFFFu;
typedef std::vector<std::vector<uint32_t>> LineSet;

// The pair table of tests/test_gpu_feedline.py's refusal test: 3 pairs on lanes 0, 3, 1 of 4 and cores 0, 1, 1 of
// 2, spc 16 : 4, lines {(0, 1), (2)}.  grow(n): n pairs of the same kind, pair i on lane i % 4 and core i % 2.
struct Stage {
    dpemu_config cfg{};
    std::vector<uint32_t> lane = {0, 3, 1}, core = {0, 1, 1}, drv_row = {0, 1, 2}, lo_row = {0, 1, 2};
    std::vector<uint32_t> spc_drv = {16, 16, 16}, spc_lo = {4, 4, 4};
    std::vector<uint64_t> shot = {5, 6, 0x100000006ull};
    std::vector<uint32_t> first, member;
    dpemu_demod_pairs pairs{};
    dpemu_feedlines lines{};
    dpemu_trace_bins bins{8, 1, 1};
    Stage()
    {
        cfg.cores_per_shot = 2;
        cfg.ro_cpw = 4;
        cfg.ro_gain[0] = cfg.ro_gain[1] = 65536;
        cfg.p1_threshold[0] = 0x11111111u; cfg.p1_threshold[1] = 0x22222222u; cfg.p1_threshold[2] = 0x33333333u;
        cfg.ro_axis[0] = 0xA0A0u; cfg.ro_axis[1] = 0xB0B0u; cfg.ro_axis[2] = 0xC0C0u;
        pairs.n_pairs = 3; pairs.n_lanes = 4; pairs.event_cap = 16; pairs.meas_cap = 4;
        pairs.n_samples_drv = 64; pairs.n_samples_lo = 16;
        set_lines({{0, 1}, {2}});
    }
    void grow(uint32_t n)
    {
        lane.resize(n); core.resize(n); drv_row.resize(n); lo_row.resize(n);
        spc_drv.assign(n, 16); spc_lo.assign(n, 4); shot.assign(n, 9);
        for (uint32_t i = 0; i < n; i++) { lane[i] = i % 4; core[i] = i % 2; drv_row[i] = lo_row[i] = i; }
        pairs.n_pairs = n;
        sync();
    }
    void set_lines(const LineSet &ls)
    {
        first.assign(1, 0u);
        member.clear();
        for (const auto &l : ls) {
            member.insert(member.end(), l.begin(), l.end());
            first.push_back((uint32_t)member.size());
        }
        lines.n_lines = (uint32_t)ls.size();
        sync();
    }
    void sync()
    {
        pairs.lane = lane.data(); pairs.core = core.data(); pairs.shot = shot.data();
        pairs.drv_row = drv_row.data(); pairs.lo_row = lo_row.data();
        pairs.spc_drv = spc_drv.data(); pairs.spc_lo = spc_lo.data();
        lines.line_first = first.data(); lines.member = member.data();
    }
};
typedef std::function<void(Stage &)> Edit;

enum { ADC, ADC_RES, DEMOD, TRACES, N_STAGES };     // the feedline entry points by their planner
static FeedlinePlan plan_stage(int stage, const Stage &s)
{
    if (stage == TRACES) return plan_trace_feedlines(&s.cfg, &s.pairs, &s.lines, &s.bins, "dpemu_feedline_traces");
    return plan_feedlines(&s.cfg, &s.pairs, &s.lines, "stage",
                          stage == ADC ? FEEDLINE_ADC : stage == ADC_RES ? FEEDLINE_ADC_RES : FEEDLINE_DEMOD);
}
static FeedlinePlan edited(int stage, const Edit &edit)
{
    Stage s;
    edit(s);
    return plan_stage(stage, s);
}
// dpemu_demod_iq's two steps, as the entry point takes them
static PairPlan plan_iq_pairs(const Stage &s)
{
    PairPlan pl = check_pairs(&s.cfg, &s.pairs, "dpemu_demod_iq", true);
    if (!pl.refused() && s.pairs.n_pairs) describe_pairs(pl, &s.cfg, &s.pairs);
    return pl;
}

static dpemu_config run_config()
{
    dpemu_config c{};
    c.cores_per_shot = 2; c.n_groups = 1; c.shots_per_group = 1; c.max_cycles = 1000;
    c.meas_latency = 1; c.sync_latency = 1; c.lut_mask = 1;
    c.meas_elem = 0; c.ro_drv_elem = 1; c.ro_cpw = 4; c.ro_gain[0] = c.ro_gain[1] = 65536;
    return c;
}
static ProgramFacts run_facts(uint32_t C = 2, uint32_t n_groups = 1)
{
    ProgramFacts f;
    f.n_programs = 1; f.C = C; f.n_groups = n_groups;
    return f;
}
typedef std::function<void(dpemu_config &)> CfgEdit;
static Refusal run_with(uint32_t model, const CfgEdit &edit, bool freqs = true, uint64_t n_shots = 10, bool hist = false)
{
    dpemu_config c = run_config();
    c.meas_model = model;
    edit(c);
    return check_run(run_facts(c.cores_per_shot == 16 ? 16 : 2, c.n_groups > 1 ? c.n_groups : 1), freqs, &c, n_shots, hist);
}

struct Columns {
    dpemu_config cfg{};
    std::vector<uint32_t> core = {1, 7, 2};
    std::vector<uint64_t> shot = {5, 0x100000006ull, 7};
    dpemu_iq_columns cols{};
    Columns()
    {
        cfg.cores_per_shot = 8;
        cfg.ro_thr = -77;
        for (uint32_t c = 0; c < DPEMU_MAX_CORES; c++) { cfg.p1_threshold[c] = 1000 + c; cfg.ro_axis[c] = 2000 + c; }
        cols.n_cols = 16; cols.meas_cap = 3; cols.by_slot = 0; cols.count_stride = 8;
    }
};
static IqColumnsPlan columns_with(const std::function<void(Columns &)> &edit)
{
    Columns k;
    edit(k);
    return plan_iq_columns(&k.cfg, &k.cols);
}

struct Channels {
    std::vector<uint32_t> lane = {1, 1}, elem = {5, 2}, spc = {16, 4}, interp = {1, 4};
    std::vector<uint32_t> env_off = {10, 20}, env_len = {30, 40}, freq_off = {50, 60}, freq_len = {70, 80};
    dpemu_dds_channels ch{};
    Channels() { ch.n_channels = 2; ch.n_lanes = 4; ch.n_samples = 1024; ch.event_cap = 16; }
    ChannelPlan plan()
    {
        ch.ch_lane = lane.data(); ch.ch_elem = elem.data(); ch.spc = spc.data(); ch.interp = interp.data();
        ch.env_off = env_off.data(); ch.env_len = env_len.data(); ch.freq_off = freq_off.data();
        ch.freq_len = freq_len.data();
        return plan_channels(&ch);
    }
};
static ChannelPlan channels_with(const std::function<void(Channels &)> &edit)
{
    Channels c;
    edit(c);
    return c.plan();
}

// resonator coefficients [3][2][4] of tests/test_gpu_resonator.py: pole (lim, 0), coupling (2^30, 0), then `edit`
constexpr int32_t LIM = (1 << 30) - (1 << 18);
static ResonatorPlan resonators_with(const std::function<void(int32_t (*)[2][4])> &edit)
{
    int32_t k[3][2][4] = {};
    for (auto &p : k) for (auto &st : p) { st[0] = LIM; st[2] = 1 << 30; }
    edit(k);
    const dpemu_resonators res = {&k[0][0][0], 5};
    return plan_resonators(&res, 3);
}

int main()
{
    // ================= dpemu_run's config (check_run) =================
    {
        dpemu_config c = run_config();
        CHECK(accepted(check_run(run_facts(), false, &c, 10, true)));
        CHECK(invalid(check_run(run_facts(), true, nullptr, 10, false), "null config"));
        CHECK(says(check_run(ProgramFacts(), true, &c, 10, false), DPEMU_E_NOPROG, "run before load_programs"));
        CHECK(says(check_run(ProgramFacts(), true, &c, 0, false), DPEMU_E_NOPROG, "load_programs"));
        CHECK(invalid(check_run(run_facts(4), true, &c, 10, false), "cores_per_shot 2 != loaded 4"));
        CHECK(invalid(check_run(run_facts(2, 3), true, &c, 10, false), "n_groups 1 != loaded 3"));
    }
    for (uint32_t model : {DPEMU_MEAS_STATE, DPEMU_MEAS_READOUT, DPEMU_MEAS_DEMOD}) {     // whatever the model
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.shots_per_group = 0; }), "shots_per_group"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.n_groups = 0x80000001u; }), "n_groups > 2^31"));
        CHECK(accepted(run_with(model, [](dpemu_config &c) { c.n_groups = 0x80000000u; })));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.max_cycles = 0; }), "max_cycles must be in"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.max_cycles = 0x7FFFFFC1u; }), "max_cycles must be in"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.meas_latency = 0; }), "meas_latency / sync_latency"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.meas_latency = (1u << 20) + 1; }), "meas_latency"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.sync_latency = 0; }), "sync_latency"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.sync_latency = (1u << 20) + 1; }), "sync_latency"));
        CHECK(accepted(run_with(model, [](dpemu_config &c) { c.meas_latency = c.sync_latency = 1u << 20; })));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.hist_assign = 2; }), "hist_assign"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.lane_order = 2; }), "lane_order 2"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.ro_win = 4096; }), "ro_win 4096"));
        CHECK(accepted(run_with(model, [](dpemu_config &c) { c.ro_win = 4095; c.hist_assign = 1; c.lane_order = 1; })));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.meas_cap = 33; }), "meas_cap > 32"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.event_cap = DPEMU_MAX_EVENT_CAP + 1; }), "event_cap / trace_cap"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.trace_cap = DPEMU_MAX_EVENT_CAP + 1; }), "event_cap / trace_cap"));
        CHECK(accepted(run_with(model, [](dpemu_config &c) { c.meas_cap = 32; c.event_cap = c.trace_cap = DPEMU_MAX_EVENT_CAP; })));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.fproc_mode = 2; }), "fproc_mode 2"));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.lut_mask = 0; }), "lut_mask"));
        CHECK(invalid(run_with(model, [](dpemu_config &) {}, true, 1ull << 30), "n_shots * cores_per_shot"));
        CHECK(accepted(run_with(model, [](dpemu_config &) {}, true, (1ull << 30) - 1)));
        CHECK(invalid(run_with(model, [](dpemu_config &c) { c.cores_per_shot = 16; }, true, 10, true), "histogram needs"));
        CHECK(accepted(run_with(model, [](dpemu_config &c) { c.cores_per_shot = 16; }, true, 10, false)));
    }
    CHECK(invalid(run_with(3, [](dpemu_config &) {}), "meas_model must be"));
    // max_cycles + meas_latency + 16 reaches 2^31 at latency 48 under the largest max_cycles
    CHECK(invalid(run_with(DPEMU_MEAS_STATE, [](dpemu_config &c) { c.max_cycles = 0x7FFFFFC0u; c.meas_latency = 48; }),
                  "max_cycles + meas_latency must stay below 2^31"));
    CHECK(accepted(run_with(DPEMU_MEAS_STATE, [](dpemu_config &c) { c.max_cycles = 0x7FFFFFC0u; c.meas_latency = 47; })));
    {   // the DEMOD-only conditions: refused under DEMOD, accepted under STATE with the same fields
        const struct { CfgEdit edit; bool freqs; const char *word; } demod_only[] = {
            {[](dpemu_config &c) { c.ro_drv_elem = 4; }, true, "ro_drv_elem 4"},
            {[](dpemu_config &c) { c.ro_drv_elem = 2; c.meas_elem = 2; }, true, "ro_drv_elem 2 must be an element 0..3 other"},
            {[](dpemu_config &c) { c.ro_cpw = 0; }, true, "ro_cpw 0 not in [1, 8]"},
            {[](dpemu_config &c) { c.ro_cpw = 9; }, true, "ro_cpw 9"},
            {[](dpemu_config &c) { c.ro_delay = 1u << 20; }, true, "ro_delay"},
            {[](dpemu_config &c) { c.ro_gain[0] = 65537; }, true, "ro_gain must be <= 65536 (1.0 in Q16)"},
            {[](dpemu_config &c) { c.ro_gain[1] = 65537; }, true, "ro_gain"},
            {[](dpemu_config &c) { c.ro_sigma = 1u << 24; }, true, "DEMOD: ro_sigma"},
            // 2^31 - 64 - 4096 * 8 clocks + latency 1 + the window 4096 * 8 + 64 = 2^31 + 1
            {[](dpemu_config &c) { c.max_cycles = 0x7FFFFFC0u - 32768u; }, true, "the readout window"},
            {[](dpemu_config &) {}, false, "without readout frequency tables"},
        };
        for (const auto &d : demod_only) {
            CHECK(invalid(run_with(DPEMU_MEAS_DEMOD, d.edit, d.freqs), d.word));
            CHECK(accepted(run_with(DPEMU_MEAS_STATE, d.edit, d.freqs)));
            CHECK(accepted(run_with(DPEMU_MEAS_READOUT, d.edit, d.freqs)));
        }
        CHECK(accepted(run_with(DPEMU_MEAS_DEMOD, [](dpemu_config &c) {       // the DEMOD bounds themselves
            c.ro_drv_elem = 3; c.ro_cpw = 8; c.ro_delay = (1u << 20) - 1; c.ro_sigma = (1u << 24) - 1;
            c.max_cycles = 0x7FFFFFC0u - 32768u - 2;
        })));
    }
    // two rules at once: the first in the order above wins
    CHECK(invalid(check_run(ProgramFacts(), true, nullptr, 10, false), "null config"));
    CHECK(invalid(run_with(DPEMU_MEAS_STATE, [](dpemu_config &c) { c.cores_per_shot = 4; c.shots_per_group = 0; }),
                  "cores_per_shot 4 != loaded 2"));
    CHECK(invalid(run_with(DPEMU_MEAS_DEMOD, [](dpemu_config &c) { c.ro_cpw = 0; c.hist_assign = 2; }), "ro_cpw"));
    CHECK(invalid(run_with(DPEMU_MEAS_DEMOD, [](dpemu_config &c) { c.max_cycles = 0; c.ro_cpw = 0; }), "max_cycles"));

    // ================= dpemu_dds (plan_channels) =================
    {
        const ChannelPlan pl = channels_with([](Channels &) {});
        CHECK(accepted(pl));
        // lane, elem & 3, spc, interp, env_off, env_len, freq_off, freq_len
        CHECK(same(pl.desc, {1, 1, 16, 1, 10, 30, 50, 70, 1, 2, 4, 4, 20, 40, 60, 80}));
        CHECK(pl.pair_lanes);
        CHECK(!channels_with([](Channels &c) { c.lane[1] = 2; }).pair_lanes);
        const ChannelPlan odd = channels_with([](Channels &c) { c.ch.n_channels = 1; });
        CHECK(accepted(odd) && !odd.pair_lanes && same(odd.desc, {1, 1, 16, 1, 10, 30, 50, 70}));
        // nothing to do: accepted, with no descriptors (and no array read)
        const ChannelPlan none = channels_with([](Channels &c) { c.ch.n_channels = 0; });
        CHECK(accepted(none) && none.desc.empty());
        const ChannelPlan empty = channels_with([](Channels &c) { c.ch.n_samples = 0; c.lane[0] = 9; });
        CHECK(accepted(empty) && empty.desc.empty());
        CHECK(accepted(channels_with([](Channels &c) { c.ch.event_cap = 1024; c.spc = {1, 16}; c.lane = {3, 3}; })));
    }
    CHECK(invalid(channels_with([](Channels &c) { c.ch.n_samples = 1002; }), "n_samples must be a multiple of 4"));
    CHECK(invalid(channels_with([](Channels &c) { c.ch.event_cap = 1025; }), "event_cap > 1024"));
    CHECK(invalid(channels_with([](Channels &c) { c.ch.n_channels = 65536; }), "n_channels > 65535"));
    CHECK(invalid(channels_with([](Channels &c) { c.lane[1] = 4; }), "channel 1: lane 4 >= n_lanes"));
    CHECK(invalid(channels_with([](Channels &c) { c.spc[0] = 0; }), "channel 0: spc 0 not in [1, 16]"));
    CHECK(invalid(channels_with([](Channels &c) { c.spc[1] = 17; }), "channel 1: spc 17"));
    CHECK(invalid(channels_with([](Channels &c) { c.interp[1] = 0; }), "channel 1: interp must be >= 1"));
    // two at once: the sample count before the cap, the cap before "nothing to do", a channel's lane before its spc
    CHECK(invalid(channels_with([](Channels &c) { c.ch.n_samples = 1002; c.ch.event_cap = 1025; }), "n_samples"));
    CHECK(invalid(channels_with([](Channels &c) { c.ch.n_channels = 0; c.ch.event_cap = 1025; }), "event_cap"));
    CHECK(invalid(channels_with([](Channels &c) { c.lane[0] = 4; c.spc[0] = 17; }), "lane"));
    CHECK(invalid(channels_with([](Channels &c) { c.interp[0] = 0; c.lane[1] = 4; }), "channel 0: interp"));

    // ================= the pair table (check_pairs / describe_pairs) =================
    const std::vector<uint32_t> want_desc = {
        // lane, core, shot low, shot high, drv_row, lo_row, spc_drv, spc_lo, p1_threshold[core], ro_axis[core]
        0, 0, 5, 0, 0, 0, 16, 4, 0x11111111u, 0xA0A0u,
        3, 1, 6, 0, 1, 1, 16, 4, 0x22222222u, 0xB0B0u,
        1, 1, 6, 1, 2, 2, 16, 4, 0x22222222u, 0xB0B0u};
    {
        Stage s;
        const PairPlan pl = plan_iq_pairs(s);
        CHECK(accepted(pl) && pl.desc.size() == 3 * DEMOD_PAIR_WORDS);
        CHECK(same(pl.desc, want_desc));
        s.pairs.n_pairs = 0;                    // no pairs: accepted with nothing else looked at
        s.pairs.lane = nullptr; s.pairs.n_samples_lo = 0;
        CHECK(accepted(plan_iq_pairs(s)) && plan_iq_pairs(s).desc.empty());
        s.pairs.meas_cap = 0;                   // ... but the scalars before n_pairs are
        CHECK(invalid(plan_iq_pairs(s), "meas_cap"));
    }
    {   // tests/test_gpu_demod_iq.py's refusals, on its two pairs
        auto two = [](const Edit &edit) { Stage s; s.pairs.n_pairs = 2; edit(s); return plan_iq_pairs(s); };
        CHECK(accepted(two([](Stage &) {})));
        CHECK(invalid(two([](Stage &s) { s.spc_drv = {16, 6, 16}; }), "pair 1: spc_drv 6 is not a multiple of spc_lo 4"));
        CHECK(invalid(two([](Stage &s) { s.spc_drv = {3, 3, 3}; s.spc_lo = {3, 3, 3}; }), "pair 0: spc_lo 3 is not a power of two"));
        CHECK(invalid(two([](Stage &s) { s.lane = {0, 4, 1}; }), "pair 1: lane 4 >= n_lanes"));
        CHECK(invalid(two([](Stage &s) { s.pairs.meas_cap = 0; }), "meas_cap 0 not in [1, 32]"));
        CHECK(invalid(two([](Stage &s) { s.core = {0, 2, 1}; }), "pair 1: core 2 >= cores_per_shot"));
        CHECK(invalid(two([](Stage &s) { s.spc_drv = {16, 17, 16}; }), "spc_drv 17"));
        CHECK(invalid(two([](Stage &s) { s.spc_drv = {0, 16, 16}; }), "spc_drv 0"));
        CHECK(invalid(two([](Stage &s) { s.spc_lo = {0, 4, 4}; }), "spc_lo 0"));
        CHECK(invalid(two([](Stage &s) { s.spc_drv = {32, 16, 16}; s.spc_lo = {32, 4, 4}; }), "spc_lo 32"));
        CHECK(invalid(two([](Stage &s) { s.pairs.n_samples_drv = 0; }), "n_samples_drv must be nonzero"));
        CHECK(accepted(two([](Stage &s) { s.spc_drv = {16, 1, 16}; s.spc_lo = {16, 1, 4}; s.pairs.meas_cap = 32; })));
    }

    // ================= the feedline stages (plan_feedlines, plan_trace_feedlines) =================
    for (int stage = 0; stage < N_STAGES; stage++) {
        // ---- accepted: the tables ----
        const FeedlinePlan pl = edited(stage, [](Stage &) {});
        CHECK(accepted(pl));
        CHECK(same(pl.desc, want_desc));
        // line_first | member | line_of | wg_first: both lines in one workgroup
        CHECK(same(pl.tab, {0, 2, 3, /**/ 0, 1, 2, /**/ 0, 0, 1, /**/ 0, 2}));
        CHECK(pl.n_pairs == 3 && pl.n_lines == 2 && pl.member == 3 && pl.line_of == 6 && pl.wg_first == 9 && pl.n_wgs == 1);

        // ---- every stage's refusals (tests/test_gpu_feedline.py, _resonator.py, _traces.py) ----
        const struct { Edit edit; const char *word; } common[] = {
            {[](Stage &s) { s.lines.n_lines = 0; }, "n_lines is 0"},
            {[](Stage &s) { s.set_lines({{0, 1}, {}}); }, "line 1 is empty"},
            {[](Stage &s) { s.first = {0, 2, 1}; s.sync(); }, "line 1 is empty"},
            {[](Stage &s) { s.set_lines({std::vector<uint32_t>(17, 0u)}); }, "line 0 has 17 members (> 16)"},
            {[](Stage &s) { s.grow(17); s.set_lines({{0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15, 16}}); }, "17 members"},
            {[](Stage &s) { s.set_lines({{0, 3}, {1, 2}}); }, "line 0: member 3 >= n_pairs"},
            {[](Stage &s) { s.set_lines({{0, 3}}); }, "member 3"},
            {[](Stage &s) { s.set_lines({{0, 1}, {1, 2}}); }, "pair 1 is in two lines (0 and 1)"},
            {[](Stage &s) { s.set_lines({{0, 0, 1}, {2}}); }, "pair 0 is in two lines (0 and 0)"},
            {[](Stage &s) { s.spc_drv = {16, 8, 16}; }, "line 0: pairs 0 and 1 differ in spc_drv / spc_lo"},
            {[](Stage &s) { s.spc_drv = {4, 2, 4}; s.spc_lo = {4, 2, 4}; }, "differ in spc_"},
            {[](Stage &s) { s.pairs.n_samples_lo = 0; }, "n_samples_lo must be a nonzero multiple of 4"},
            {[](Stage &s) { s.pairs.n_samples_lo = 18; }, "n_samples_lo"},
            {[](Stage &s) { s.pairs.event_cap = 1025; }, "event_cap > 1024"},
            {[](Stage &s) { s.pairs.meas_cap = 0; }, "meas_cap 0"},
            {[](Stage &s) { s.pairs.meas_cap = 33; }, "meas_cap 33"},
            {[](Stage &s) { s.lane = {0, 4, 1}; }, "pair 1: lane 4"},
            {[](Stage &s) { s.core = {0, 2, 1}; }, "pair 1: core 2"},
            {[](Stage &s) { s.first = {1, 2, 3}; s.sync(); }, "line_first[0] must be 0"},
            // what no GPU test reaches
            {[](Stage &s) { s.cfg.ro_cpw = 0; }, "ro_cpw 0 not in [1, 8]"},
            {[](Stage &s) { s.cfg.ro_cpw = 9; }, "ro_cpw 9"},
            {[](Stage &s) { s.cfg.cores_per_shot = 0; }, "cores_per_shot 0 not in [1, 64]"},
            {[](Stage &s) { s.cfg.cores_per_shot = 65; }, "cores_per_shot 65"},
            {[](Stage &s) { s.pairs.n_pairs = 65536; }, "n_pairs > 65535"},
            {[](Stage &s) { s.pairs.lane = nullptr; }, ": pairs->lane is NULL"},
            {[](Stage &s) { s.pairs.core = nullptr; }, "pairs->core is NULL"},
            {[](Stage &s) { s.pairs.shot = nullptr; }, "pairs->shot is NULL"},
            {[](Stage &s) { s.pairs.drv_row = nullptr; }, "pairs->drv_row is NULL"},
            {[](Stage &s) { s.pairs.lo_row = nullptr; }, "pairs->lo_row is NULL"},
            {[](Stage &s) { s.pairs.spc_drv = nullptr; }, "pairs->spc_drv is NULL"},
            {[](Stage &s) { s.pairs.spc_lo = nullptr; }, "pairs->spc_lo is NULL"},
            {[](Stage &s) { s.lines.line_first = nullptr; }, ": lines->line_first is NULL"},
            {[](Stage &s) { s.lines.member = nullptr; }, ": lines->member is NULL"},
            {[](Stage &s) { s.pairs.n_pairs = 0; }, "member 0 >= n_pairs"},       // no pairs: no line can hold one
            {[](Stage &s) { s.spc_lo = {4, 4, 3}; }, "pair 2: spc_lo 3"},
            {[](Stage &s) { s.spc_drv = {16, 16, 6}; }, "pair 2: spc_drv 6"},
        };
        for (const auto &c : common) CHECK(invalid(edited(stage, c.edit), c.word));

        // ---- what the stages differ in ----
        const Edit gain = [](Stage &s) { s.cfg.ro_gain[1] = 65537; }, gain0 = [](Stage &s) { s.cfg.ro_gain[0] = 65537; };
        const Edit unlisted = [](Stage &s) { s.set_lines({{2, 0}}); }, no_drv = [](Stage &s) { s.pairs.n_samples_drv = 0; };
        if (stage == ADC) {
            CHECK(invalid(edited(stage, gain), "ro_gain must be <= 65536"));
            CHECK(invalid(edited(stage, gain0), "ro_gain"));
        } else {
            CHECK(accepted(edited(stage, gain)) && accepted(edited(stage, gain0)));
        }
        if (stage == ADC || stage == ADC_RES) {
            CHECK(invalid(edited(stage, no_drv), "n_samples_drv must be nonzero"));
            // a table with an unlisted pair: line_of[1] stays ~0
            const FeedlinePlan un = edited(stage, unlisted);
            CHECK(accepted(un) && same(un.desc, want_desc));
            CHECK(same(un.tab, {0, 2, /**/ 2, 0, /**/ 0, NONE, 0, /**/ 0, 1}));
            CHECK(un.tab[un.line_of + 1] == 0xFFFFFFFFu);
            CHECK(un.n_lines == 1 && un.member == 2 && un.line_of == 4 && un.wg_first == 7 && un.n_wgs == 1);
        } else {
            CHECK(accepted(edited(stage, no_drv)));
            CHECK(invalid(edited(stage, unlisted), "pair 1 is in no line"));
            CHECK(invalid(edited(stage, [](Stage &s) { s.set_lines({{0, 1}}); }), "pair 2 is in no line"));
            // ... while with every pair listed, {(2, 0), (1)} is this stage's table too
            const FeedlinePlan all = edited(stage, [](Stage &s) { s.set_lines({{2, 0}, {1}}); });
            CHECK(accepted(all) && same(all.tab, {0, 2, 3, /**/ 2, 0, 1, /**/ 0, 1, 0, /**/ 0, 2}));
        }

        // ---- two rules at once ----
        // the lines' own arguments come before the pair descriptors, those before the line table
        CHECK(invalid(edited(stage, [](Stage &s) { s.lines.n_lines = 0; s.lane = {0, 4, 1}; }), "n_lines is 0"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.lane = {0, 4, 1}; s.first = {1, 2, 3}; s.sync(); }), "lane 4"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.pairs.event_cap = 1025; s.pairs.meas_cap = 0; }), "event_cap"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.pairs.n_samples_lo = 18; s.lines.n_lines = 0; }), "n_samples_lo"));
        // a line's size before any member; a member's range before its being listed twice, that before its spc
        CHECK(invalid(edited(stage, [](Stage &s) { s.set_lines({{0, 3}, {}}); }), "line 1 is empty"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.set_lines({{0, 0}, {2, 3}}); }), "two lines"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.set_lines({{0, 1}, {1, 2}}); s.spc_drv = {16, 8, 16}; }), "differ in spc_drv"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.set_lines({{0}, {1, 1}}); s.spc_drv = {16, 8, 8}; }), "two lines"));
        // the gain and the unlisted pair come last
        CHECK(invalid(edited(stage, [](Stage &s) { s.cfg.ro_gain[1] = 65537; s.set_lines({{0, 1}, {1, 2}}); }), "two lines"));
        CHECK(invalid(edited(stage, [](Stage &s) { s.set_lines({{0, 3}}); }), "member 3"));    // (pairs 1, 2 are in no line)

        // ---- a 16-member line; the workgroups of feedline_res_kernel ----
        const FeedlinePlan full = edited(stage, [](Stage &s) {
            s.grow(16);
            s.set_lines({{15, 14, 13, 12, 11, 10, 9, 8, 7, 6, 5, 4, 3, 2, 1, 0}});
        });
        CHECK(accepted(full) && full.n_wgs == 1 && full.tab.size() == 2 + 16 + 16 + 2 && full.tab[1] == 16);
        CHECK(full.tab[full.member] == 15 && full.tab[full.line_of + 15] == 0 && full.tab[full.wg_first + 1] == 1);
        // 33 lines of one member: 16, 16 and 1 lines
        const FeedlinePlan many = edited(stage, [](Stage &s) {
            s.grow(33);
            LineSet ls;
            for (uint32_t i = 0; i < 33; i++) ls.push_back({32 - i});
            s.set_lines(ls);
        });
        CHECK(accepted(many) && many.n_wgs == 3 && many.member == 34 && many.line_of == 67 && many.wg_first == 100);
        CHECK((std::vector<uint32_t>(many.tab.begin() + many.wg_first, many.tab.end()) == std::vector<uint32_t>{0, 16, 32, 33}));
        CHECK(many.tab[33] == 33 && many.tab[many.member] == 32 && many.tab[many.line_of] == 32 && many.tab[many.line_of + 32] == 0);
        // lines of 7, 7, 7, 16 and 1 members: (7, 7), (7), (16), (1)
        const FeedlinePlan mixed = edited(stage, [](Stage &s) {
            s.grow(38);
            LineSet ls(5);
            const uint32_t sizes[5] = {7, 7, 7, 16, 1};
            for (uint32_t l = 0, m = 0; l < 5; l++)
                for (uint32_t k = 0; k < sizes[l]; k++) ls[l].push_back(m++);
            s.set_lines(ls);
        });
        CHECK(accepted(mixed) && mixed.n_wgs == 4 && mixed.member == 6 && mixed.line_of == 44 && mixed.wg_first == 82);
        CHECK((std::vector<uint32_t>(mixed.tab.begin(), mixed.tab.begin() + 6) == std::vector<uint32_t>{0, 7, 14, 21, 37, 38}));
        CHECK((std::vector<uint32_t>(mixed.tab.begin() + mixed.wg_first, mixed.tab.end()) == std::vector<uint32_t>{0, 2, 3, 4, 5}));
        CHECK(mixed.tab[mixed.line_of + 20] == 2 && mixed.tab[mixed.line_of + 21] == 3 && mixed.tab[mixed.line_of + 37] == 4);
    }
    CHECK(accepted(edited(ADC, [](Stage &s) { s.cfg.ro_gain[0] = s.cfg.ro_gain[1] = 65536; })));
    CHECK(accepted(edited(ADC, [](Stage &s) { s.cfg.ro_gain[0] = 0; s.pairs.event_cap = 1024; s.pairs.meas_cap = 32; })));
    CHECK(says(edited(ADC, [](Stage &s) { s.pairs.lane = nullptr; }), DPEMU_E_INVALID, "stage: pairs->lane is NULL"));

    // ---- the bins of dpemu_feedline_traces ----
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.n_bins = 0; }), "n_bins 0 not in [1, 4096]"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.n_bins = 4097; }), "n_bins 4097"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.bin_clocks = 0; }), "bin_clocks must be >= 1"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.by_slot = 2; }), "by_slot 2 must be 0 or 1"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.bin_clocks = (1u << 31) / (3 * 4 * 16) + 1; }),
                  "n_pairs * meas_cap * bin_clocks * 16 = 192 * 11184811 exceeds 2^31"));
    CHECK(accepted(edited(TRACES, [](Stage &s) { s.bins.bin_clocks = (1u << 31) / (3 * 4 * 16); s.bins.by_slot = 0; })));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.bin_clocks = 0xFFFFFFFFu; s.pairs.n_pairs = 65535; s.pairs.meas_cap = 32; }),
                  "bin_clocks"));
    // 2 pairs x 4 slots x 2^24 clocks x 16 = 2^31 exactly
    const Edit two_pairs = [](Stage &s) { s.pairs.n_pairs = 2; s.set_lines({{0, 1}}); s.bins.n_bins = 4096; };
    CHECK(accepted(edited(TRACES, [&](Stage &s) { two_pairs(s); s.bins.bin_clocks = 1u << 24; })));
    CHECK(invalid(edited(TRACES, [&](Stage &s) { two_pairs(s); s.bins.bin_clocks = (1u << 24) + 1; }), "exceeds 2^31"));
    // the bins come before the pairs and the lines
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.n_bins = 0; s.lines.n_lines = 0; }), "n_bins"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.by_slot = 2; s.set_lines({{0, 1}, {1, 2}}); }), "by_slot"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.bin_clocks = 0; s.pairs.event_cap = 1025; }), "bin_clocks"));
    CHECK(invalid(edited(TRACES, [](Stage &s) { s.bins.n_bins = 0; s.bins.bin_clocks = 0; s.bins.by_slot = 2; }), "n_bins"));

    // ================= the resonators (plan_resonators) =================
    {
        const int32_t k[8] = {1, -2, 3, -4, 5, 6, -(1 << 30), 1 << 30};
        const dpemu_resonators res = {k, 0};
        const ResonatorPlan pl = plan_resonators(&res, 1);
        CHECK(accepted(pl) && same(pl.coef, {1, -2, 3, -4, 5, 6, -(1 << 30), 1 << 30, 0, 0, 0, 0}));
        CHECK(accepted(resonators_with([](int32_t (*)[2][4]) {})));
        CHECK(resonators_with([](int32_t (*)[2][4]) {}).coef.size() == 3 * 8 + 4);
        // the bounds themselves: |a| = 2^30 - 2^18 on either axis, couplings of +-2^30
        CHECK(accepted(resonators_with([](int32_t (*k)[2][4]) {
            k[0][0][0] = 0; k[0][0][1] = -LIM; k[1][1][2] = -(1 << 30); k[1][1][3] = 1 << 30; k[2][0][0] = -LIM;
        })));
    }
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[2][1][0] = LIM + 1; }), "pair 2 state 1: pole (1073479681, 0) outside"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[0][0][1] = 1 << 18; }), "pair 0 state 0: pole"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[0][0][1] = 1; }), "pole"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[1][0][0] = INT32_MIN; }), "pair 1 state 0: pole (-2147483648, 0)"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[1][0][2] = (1 << 30) + 1; }), "pair 1 state 0: coupling (1073741825, 0)"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[0][1][3] = -(1 << 30) - 1; }), "pair 0 state 1: coupling (1073741824, -1073741825) outside +-2^30"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[0][1][2] = -(1 << 30) - 1; }), "coupling"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[0][1][3] = (1 << 30) + 1; }), "coupling"));
    // in table order, and a pair's pole before its coupling
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[1][0][0] = LIM + 1; k[0][1][2] = INT32_MAX; }), "pair 0 state 1: coupling"));
    CHECK(invalid(resonators_with([](int32_t (*k)[2][4]) { k[1][1][0] = LIM + 1; k[1][1][2] = INT32_MAX; }), "pair 1 state 1: pole"));

    // ================= dpemu_iq_stats (plan_iq_columns) =================
    {
        const IqColumnsPlan run = columns_with([](Columns &) {});
        CHECK(accepted(run) && !run.expl && run.tab.empty());
        for (uint32_t c = 0; c < DPEMU_MAX_CORES; c++) CHECK(run.p1[c] == 1000 + c && run.axis[c] == 2000 + c && run.thr[c] == -77);
        Columns k;
        k.cols.n_cols = 3; k.cols.core = k.core.data(); k.cols.shot = k.shot.data();
        const uint32_t axis[8] = {10, 11, 12, 13, 14, 15, 16, 17};
        const int32_t thr[8] = {-1, -2, -3, -4, 5, 6, 7, 8};
        k.cols.axis = axis; k.cols.thr = thr;
        const IqColumnsPlan ex = plan_iq_columns(&k.cfg, &k.cols);
        CHECK(accepted(ex) && ex.expl);
        // [3] u64 shots then [3] u32 cores, little-endian
        CHECK(same(ex.tab, {5, 0, 0, 0, 0, 0, 0, 0, /**/ 6, 0, 0, 0, 1, 0, 0, 0, /**/ 7, 0, 0, 0, 0, 0, 0, 0,
                            /**/ 1, 0, 0, 0, /**/ 7, 0, 0, 0, /**/ 2, 0, 0, 0}));
        // the caller's axes and thresholds for the C cores, cfg's beyond
        for (uint32_t c = 0; c < DPEMU_MAX_CORES; c++) {
            CHECK(ex.p1[c] == 1000 + c);
            CHECK(ex.axis[c] == (c < 8 ? axis[c] : 2000 + c) && ex.thr[c] == (c < 8 ? thr[c] : -77));
        }
        k.cols.n_cols = 0;                      // no columns: accepted, nothing to upload
        const IqColumnsPlan none = plan_iq_columns(&k.cfg, &k.cols);
        CHECK(accepted(none) && none.expl && none.tab.empty());
        // n_cols * meas_cap = 2^31 exactly (the run layout: no table is built)
        CHECK(accepted(columns_with([](Columns &k) { k.cols.n_cols = 1u << 30; k.cols.meas_cap = 2; })));
        CHECK(accepted(columns_with([](Columns &k) { k.cols.n_cols = 1u << 26; k.cols.meas_cap = 32; k.cols.by_slot = 1; })));
    }
    CHECK(invalid(columns_with([](Columns &k) { k.cfg.cores_per_shot = 6; }), "cores_per_shot 6 is not a power of two"));
    CHECK(invalid(columns_with([](Columns &k) { k.cfg.cores_per_shot = 0; }), "cores_per_shot 0"));
    CHECK(invalid(columns_with([](Columns &k) { k.cfg.cores_per_shot = 128; }), "cores_per_shot 128"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.meas_cap = 0; }), "meas_cap 0 not in [1, 32]"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.meas_cap = 33; }), "meas_cap 33"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.by_slot = 2; }), "by_slot 2"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.count_stride = 0; }), "count_stride must be >= 1"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = 1u << 31; k.cols.meas_cap = 2; }), "n_cols * meas_cap = 4294967296 exceeds 2^31"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = (1u << 30) + 8; k.cols.meas_cap = 2; }), "2^31"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = 3; k.cols.core = k.core.data(); }), "need both core and shot (shot is NULL)"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = 3; k.cols.shot = k.shot.data(); }), "(core is NULL)"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = 3; k.core[1] = 8; k.cols.core = k.core.data(); k.cols.shot = k.shot.data(); }),
                  "column 1: core 8 >= cores_per_shot"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = 12; }), "n_cols 12 is not a multiple of cores_per_shot 8"));
    CHECK(invalid(columns_with([](Columns &k) { k.cfg.lane_order = 2; }), "lane_order 2"));
    // explicit columns read no lane order and need no multiple of C
    CHECK(accepted(columns_with([](Columns &k) { k.cfg.lane_order = 2; k.cols.n_cols = 3; k.cols.core = k.core.data(); k.cols.shot = k.shot.data(); })));
    // two at once
    CHECK(invalid(columns_with([](Columns &k) { k.cols.meas_cap = 0; k.cols.by_slot = 2; }), "meas_cap"));
    CHECK(invalid(columns_with([](Columns &k) { k.cfg.cores_per_shot = 6; k.cols.count_stride = 0; }), "cores_per_shot"));
    CHECK(invalid(columns_with([](Columns &k) { k.cfg.lane_order = 2; k.cols.n_cols = 12; }), "lane_order"));
    CHECK(invalid(columns_with([](Columns &k) { k.cols.n_cols = 12; k.cols.core = k.core.data(); }), "need both"));

    std::printf("ok %d\n", n_checks);
    return 0;
}
