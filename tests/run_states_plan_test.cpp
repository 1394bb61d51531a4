// CPU driver of plan_run's `states` argument (csrc/launch_plan.h), built and
// run by tests/test_run_states_plan.py with g++.  Reads launch_plan_test.cpp's
// `run` request lines from the file named by argv[1] and prints three plans per
// line as key=value pairs: the four-argument call's, the five-argument call's
// with states = false, and the one with states = true.  The assertions are in
// the Python test.
//   run C n_groups n_programs straight linear has_fproc has_sync reg_writes has_macros has_cmd_major
//       macro_nr macro_addid max_len group_len | spg lane_order exec_flags meas_model fproc_mode n_shots want_hist
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../distributed_processor_amd/csrc/launch_plan.h"

using namespace dpemu;

static void show(const char *tag, const RunPlan &p)
{
    std::printf("%s name=%s family=%d cm=%d src=%d fb=%d slots=%u feat=%d bfeat=%d lds=%u repl=%d R=%u stride=%" PRIu64
                " hist_lds=%u bins=%" PRIu64 " fold=%d rep_words=%" PRIu64 "\n",
                tag, p.name.c_str(), (int)p.family, p.cmd_major, p.src, p.fetch_batch, p.slots, p.feat, p.bfeat,
                p.prog_lds_words, p.hist_repl, p.R, p.hist_stride, p.hist_lds, p.bins, p.hist_fold, p.hist_rep_words());
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s requests.txt\n", argv[0]); return 2; }
    std::FILE *fh = std::fopen(argv[1], "r");
    if (!fh) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::printf("caps branch=%u k_branch=%d feat_states=%d feat_prog_lds=%d\n", BRANCH_LDS_MAX, (int)K_BRANCH, FEAT_STATES,
                FEAT_PROG_LDS);
    char line[512];
    while (std::fgets(line, sizeof line, fh)) {
        unsigned v[20];
        unsigned long long n_shots;
        if (strncmp(line, "run ", 4)) continue;
        if (std::sscanf(line + 4, "%u %u %u %u %u %u %u %u %u %u %u %u %u %u | %u %u %u %u %u %llu %u", &v[0], &v[1],
                        &v[2], &v[3], &v[4], &v[5], &v[6], &v[7], &v[8], &v[9], &v[10], &v[11], &v[12], &v[13],
                        &v[14], &v[15], &v[16], &v[17], &v[18], &n_shots, &v[19]) != 21) {
            std::printf("bad line: %s", line);
            return 2;
        }
        ProgramFacts f;
        f.C = v[0]; f.n_groups = v[1]; f.n_programs = v[2];
        f.straight = v[3]; f.linear = v[4]; f.has_fproc = v[5]; f.has_sync = v[6]; f.reg_writes = v[7];
        f.has_macros = v[8]; f.has_cmd_major = v[9];
        f.macro_nr = (int)v[10]; f.macro_addid = v[11]; f.max_len = v[12];
        f.group_len.assign(f.n_groups, v[13]);
        dpemu_config cfg{};
        cfg.cores_per_shot = f.C; cfg.n_groups = f.n_groups;
        cfg.shots_per_group = v[14]; cfg.lane_order = v[15]; cfg.exec_flags = v[16]; cfg.meas_model = v[17];
        cfg.fproc_mode = v[18];
        show("four", plan_run(f, &cfg, n_shots, v[19] != 0));
        show("off", plan_run(f, &cfg, n_shots, v[19] != 0, false));
        show("on", plan_run(f, &cfg, n_shots, v[19] != 0, true));
    }
    std::fclose(fh);
    return 0;
}
