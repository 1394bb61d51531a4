// CPU driver of the kernel choice over whole program sets, built and run by
// tests/test_feature_cases.py with g++.  Reads cases from the file named by
// argv[1] (u32 little-endian: n_cases, then per case C, n_groups, n_programs,
// n_cmds, shots_per_group, lane_order, exec_flags, meas_model, fproc_mode,
// n_shots, offsets[], n_instr[], prog_table[], words[]), builds each image and
// its facts (csrc/program_image.h) and prints the facts and two plans
// (csrc/launch_plan.h plan_run) per case as key=value pairs: dpemu_run's
// ("off") and dpemu_run_states' ("on").  The assertions are in the Python test.
#include <cstdio>
#include <vector>

#include "../distributed_processor_amd/csrc/launch_plan.h"

using namespace dpemu;

static void show(const char *tag, int i, const RunPlan &p)
{
    std::printf("%s case=%d name=%s family=%d feat=%d bfeat=%d lds=%u cm=%d\n", tag, i, p.name.c_str(), (int)p.family, p.feat,
                p.bfeat, p.prog_lds_words, p.cmd_major);
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s cases.bin\n", argv[0]); return 2; }
    std::FILE *fh = std::fopen(argv[1], "rb");
    if (!fh) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::vector<uint32_t> buf;
    uint32_t tmp[4096];
    for (size_t n; (n = std::fread(tmp, 4, 4096, fh)) > 0;) buf.insert(buf.end(), tmp, tmp + n);
    std::fclose(fh);
    if (buf.empty()) { std::printf("empty input\n"); return 2; }
    const uint32_t *in = buf.data(), *end = buf.data() + buf.size();
    const uint32_t n_cases = *in++;
    std::printf("caps branch=%u prog=%u k_branch=%d k_interp=%d\n", BRANCH_LDS_MAX, PROG_LDS_MAX, (int)K_BRANCH, (int)K_INTERP);
    for (uint32_t i = 0; i < n_cases; i++) {
        if (end - in < 10) { std::printf("truncated input at case %u\n", i); return 2; }
        const uint32_t C = in[0], n_groups = in[1], n_programs = in[2], n_cmds = in[3];
        dpemu_config cfg{};
        cfg.cores_per_shot = C; cfg.n_groups = n_groups;
        cfg.shots_per_group = in[4]; cfg.lane_order = in[5]; cfg.exec_flags = in[6]; cfg.meas_model = in[7];
        cfg.fproc_mode = in[8];
        const uint64_t n_shots = in[9];
        in += 10;
        const uint64_t need = 2ull * n_programs + (uint64_t)n_groups * C + 4ull * n_cmds;
        if ((uint64_t)(end - in) < need) { std::printf("truncated input in case %u\n", i); return 2; }
        const uint32_t *offsets = in, *n_instr = in + n_programs, *table = in + 2 * n_programs;
        const uint32_t *words = table + (size_t)n_groups * C;
        in = words + 4ull * n_cmds;
        const ProgramImage im = build_program_image(words, offsets, n_instr, n_programs, table, n_groups, C);
        if (!im.err.empty()) { std::printf("case %u refused: %s\n", i, im.err.c_str()); return 1; }
        const ProgramFacts &f = im.facts;
        uint64_t tot = 0;
        for (uint64_t x : f.group_len) tot += x;
        std::printf("facts case=%u has_fproc=%d has_sync=%d reg_writes=%d straight=%d linear=%d macros=%d group_cmds=%llu\n", i,
                    f.has_fproc, f.has_sync, f.reg_writes, f.straight, f.linear, f.has_macros, (unsigned long long)tot);
        show("off", (int)i, plan_run(f, &cfg, n_shots, C <= 12, false));
        show("on", (int)i, plan_run(f, &cfg, n_shots, C <= 12, true));
    }
    if (in != end) { std::printf("trailing input\n"); return 2; }
    std::printf("OK\n");
    return 0;
}
