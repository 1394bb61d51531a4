// CPU driver of the per-call planners (csrc/launch_plan.h), built and run by
// tests/test_launch_plan.py with g++.  Reads one request per line from the
// file named by argv[1] and prints the plan as key=value pairs; the
// assertions are in the Python test.
//   run C n_groups n_programs straight linear has_fproc has_sync reg_writes has_macros has_cmd_major
//       macro_nr macro_addid max_len group_len | spg lane_order exec_flags meas_model fproc_mode n_shots want_hist
//   dds event_cap n_samples n_channels interp env_len freq_len
//   iq  n_cols C S wgs_per_cu n_cu
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../distributed_processor_amd/csrc/launch_plan.h"

using namespace dpemu;

int main(int argc, char **argv)
{
    if (argc != 2) { std::printf("usage: %s requests.txt\n", argv[0]); return 2; }
    std::FILE *fh = std::fopen(argv[1], "r");
    if (!fh) { std::printf("cannot open %s\n", argv[1]); return 2; }
    std::printf("caps straight=%u branch=%u interp=%u dds_budget=%u dds_dense=%u rec_min=%u\n", STRAIGHT_LDS_MAX,
                BRANCH_LDS_MAX, PROG_LDS_MAX, DDS_WG_LDS_BUDGET, (uint32_t)DDS_WG_LDS_DENSE, DDS_REC_LDS_MIN);
    char line[512];
    while (std::fgets(line, sizeof line, fh)) {
        unsigned v[22];
        unsigned long long n_shots;
        if (!strncmp(line, "run ", 4)) {
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
            const RunPlan p = plan_run(f, &cfg, n_shots, v[19] != 0);
            std::printf("name=%s family=%d cm=%d src=%d fb=%d slots=%u feat=%d bfeat=%d lds=%u repl=%d R=%u stride=%" PRIu64
                        " hist_lds=%u bins=%" PRIu64 "\n",
                        p.name.c_str(), (int)p.family, p.cmd_major, p.src, p.fetch_batch, p.slots, p.feat, p.bfeat,
                        p.prog_lds_words, p.hist_repl, p.R, p.hist_stride, p.hist_lds, p.bins);
        } else if (!strncmp(line, "dds ", 4)) {
            if (std::sscanf(line + 4, "%u %u %u %u %u %u", &v[0], &v[1], &v[2], &v[3], &v[4], &v[5]) != 6) return 2;
            std::vector<uint32_t> desc((size_t)v[2] * DDS_CH_WORDS, 0u);
            for (uint32_t i = 0; i < v[2]; i++) {
                uint32_t *d = &desc[(size_t)i * DDS_CH_WORDS];
                d[2] = 1; d[3] = v[3]; d[5] = v[4]; d[7] = v[5];
            }
            const DdsPlan p = plan_dds(desc.data(), v[2], v[1], v[0]);
            std::printf("ev_lds=%u rec_lds=%u env_lds=%u freq_lds=%u tiles=%u stripes=%u wg_tiles=%u dense=%d bytes=%u "
                        "all_bytes=%u\n",
                        p.ev_lds, p.rec_lds, p.env_lds, p.freq_lds, p.tiles, p.stripes, p.wg_tiles, p.dense,
                        dds_lds_bytes(p.rec_lds, p.wg_tiles, p.env_lds, p.freq_lds),
                        dds_lds_bytes(p.ev_lds, p.wg_tiles, p.env_lds, p.freq_lds));
        } else if (!strncmp(line, "iq ", 3)) {
            if (std::sscanf(line + 3, "%u %u %u %u %u", &v[0], &v[1], &v[2], &v[3], &v[4]) != 5) return 2;
            std::printf("gx=%u\n", iq_stats_grid(v[0], v[1], v[2], v[3], v[4]));
        }
    }
    std::fclose(fh);
    return 0;
}
