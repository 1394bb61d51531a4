// launch_plan.h -- the per-call choices of the entry points, made on the host
// from the loaded programs' facts (program_image.h) and the caller's config:
// which interpreter kernel a run launches and with which template choices,
// the histogram strategy, the DDS stripe / record-LDS plan, the iq_stats
// grid width, the trace chunks and dpemu_qsim's checks and device table.
// The other entry points' argument checks and the tables they upload (the
// channel descriptors plan_dds reads, the pair table plan_traces sorts) are
// stage_plan.h's.  Nothing here touches the device (tests/launch_plan_test.cpp
// builds it with a plain C++ compiler).  The choice depends only on the
// programs, the grid size and the caller's exec_flags -- never on the
// environment.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dpemu.h"
#include "program_image.h"

namespace dpemu {

enum KernelFamily { K_STRAIGHT, K_MACRO, K_BRANCH, K_INTERP };

struct RunPlan {
    KernelFamily family = K_INTERP;
    bool cmd_major = false;                 // fetch from the command-major copy (KParams::fetch)
    int src = STRAIGHT_PROG, fetch_batch = 1;   // straight_kernel
    uint32_t slots = 0;                     // program slots per wave of the staged macro kernel (0: macro_kernel)
    int feat = 0, bfeat = 0;                // interp_kernel / branch_kernel FEAT_* bits
    uint32_t prog_lds_words = 0;            // KParams::prog_lds_words
    // outcome histogram: replicas (hist_repl) or direct atomics into out->hist
    bool hist_repl = false;
    uint32_t R = 0;
    uint64_t bins = 0, hist_stride = 0;
    uint32_t hist_lds = 0;
    bool hist_fold = false;                 // straight_kernel reduces the replicas itself: no reduce launch
    std::string name;                       // dpemu_last_kernel

    // u32 words of the replica allocation: the rows, then the folded reduce's tickets
    uint64_t hist_rep_words() const { return R * hist_stride + (hist_fold ? (R + 1ull) * HIST_TICKET_PITCH : 0); }
};

// states: dpemu_run_states' plan -- every program on branch_kernel<FEAT_STATES>,
// whatever its facts and the exec_flags that pick other kernel families (the
// route DEMOD runs take already); LDS staging and the histogram as for any
// K_BRANCH run
inline RunPlan plan_run(const ProgramFacts &f, const dpemu_config *cfg, uint64_t n_shots, bool want_hist,
                        bool states = false)
{
    RunPlan pl;
    const uint32_t C = cfg->cores_per_shot;
    const uint32_t n_lanes = (uint32_t)(n_shots * C);
    const bool cmd_major = pl.cmd_major = f.has_cmd_major && !(cfg->exec_flags & DPEMU_X_PROG_MAJOR);
    // LDS program staging: a workgroup of S = BLOCK / C shots spans at most w
    // consecutive program groups; stage their programs if they fit
    const uint32_t S = BLOCK / C, ng = cfg->n_groups;
    const uint64_t w = (ng == 1) ? 1 : (S - 1) / cfg->shots_per_group + 2;
    uint64_t footprint = ~0ull;
    if (w * C <= BLOCK) {
        const std::vector<uint64_t> &gl = f.group_len;
        uint64_t tot = 0;
        for (uint64_t x : gl) tot += x;
        footprint = (w / ng) * tot;
        const uint64_t r = w % ng;
        if (r) {
            uint64_t win = 0, best = 0;
            for (uint64_t i = 0; i < r; i++) win += gl[i % ng];
            best = win;
            for (uint64_t g = 1; g < ng; g++) {
                win += gl[(g + r - 1) % ng];
                win -= gl[g - 1];
                best = std::max(best, win);
            }
            footprint += best;
        }
    }
    int feat = 0;
    // Pulse-only programs run on the wave-uniform-ip kernel (straight.hip)
    // unless ip could wrap (a 2^16-command program) or the general
    // interpreter is asked for (DPEMU_X_GENERAL).  Small grids (latency-bound)
    // fetch commands in batches of 4.  The kernel stages the workgroup's
    // programs in LDS when they fit the share of a CU's LDS that the grid's
    // co-resident workgroups leave and the programs are long (a dependent
    // global fetch per command is then the bottleneck); else it fetches the
    // command-major image.  The general interpreter stages only on request
    // (DPEMU_X_PROG_LDS), within 16 KiB.
    const uint64_t blocks = ((uint64_t)n_lanes + BLOCK - 1) / BLOCK;
    const bool small = blocks <= 4 * 256;
    pl.fetch_batch = small ? 4 : 1;
    // the DEMOD readout model runs on branch_kernel<FEAT_DEMOD> (or the
    // general interpreter): the straight / macro kernels do not carry it
    const bool demod = cfg->meas_model == DPEMU_MEAS_DEMOD;
    const bool uniform = !states && !demod && f.straight && f.max_len < 65536u && !(cfg->exec_flags & DPEMU_X_GENERAL);
    const bool macro = !states && !demod && !uniform && f.has_macros && !(cfg->exec_flags & (DPEMU_X_GENERAL | DPEMU_X_PROG_LDS));
    // the staged macro kernel needs at most MACRO_SLOTS distinct programs per
    // wave: (program groups a wave's run of consecutive shots can span) x
    // (cores in the wave), for the thread mapping of block_core_major
    if (macro && !(cfg->exec_flags & DPEMU_X_MACRO_DIRECT)) {
        uint64_t shots_run, cores_w;
        if (cfg->lane_order == DPEMU_LANES_SHOT_MAJOR) {
            shots_run = std::max<uint64_t>(1, 64 / C);
            cores_w = std::min<uint64_t>(C, 64);
        } else {
            const uint64_t Sb = BLOCK / C;
            shots_run = std::min<uint64_t>(Sb, 64);
            cores_w = 64 / shots_run;
        }
        const uint64_t spg = cfg->shots_per_group;
        const uint64_t groups = ng == 1 ? 1 : std::min<uint64_t>(ng, (shots_run - 1 + spg - 1) / spg + 1);
        const uint64_t need = groups * cores_w;
        pl.slots = need <= MACRO_SLOTS ? MACRO_SLOTS : (need <= MACRO_SLOTS_WIDE && f.macro_nr == 2) ? MACRO_SLOTS_WIDE : 0u;
    }
    pl.src = cmd_major ? STRAIGHT_ROWS : STRAIGHT_PROG;
    if (uniform) {
        const uint64_t per_cu = std::min<uint64_t>(8, std::max<uint64_t>(1, (blocks + 255) / 256));
        const uint64_t budget = std::min<uint64_t>(STRAIGHT_LDS_MAX, (150ull * 1024 / per_cu) / 16);
        if (footprint <= budget && f.max_len >= 64) {
            pl.src = STRAIGHT_LDS;
            pl.prog_lds_words = (uint32_t)std::max<uint64_t>(16, (footprint + 15) & ~15ull);
        }
    } else if (footprint <= PROG_LDS_MAX && (cfg->exec_flags & DPEMU_X_PROG_LDS)) {
        feat |= FEAT_PROG_LDS;
        pl.prog_lds_words = (uint32_t)std::max<uint64_t>(16, (footprint + 15) & ~15ull);
    }
    if (f.has_fproc) feat |= (cfg->fproc_mode == DPEMU_FPROC_LUT) ? FEAT_LUT : FEAT_FPROC;
    if (f.has_sync) feat |= FEAT_SYNC;
    if (f.straight) feat |= FEAT_STRAIGHT;
    pl.feat = feat;
    // outcome histogram.  Direct: one u64 atomic per shot into out->hist --
    // cheapest when concurrent shots spread over many bins.  Replicas: R
    // privatised u32 copies picked by workgroup, then a reduce kernel (or the
    // interpreter's own last workgroup: hist_fold below) -- for
    // few bins hit by every wave at once (e.g. one program, 10^6 shots), where
    // direct atomics serialise on a few cache lines.  Default: replicas when
    // the bins a wave population touches concurrently are few.
    if (want_hist) {
        pl.bins = (uint64_t)ng << C;
        const uint64_t spg = std::max<uint64_t>(1, cfg->shots_per_group);
        // groups live at once across ~64K resident lanes
        const uint64_t live_groups = std::min<uint64_t>(ng, (65536 / C) / spg + 1);
        bool repl = (live_groups << C) < 4096;
        if (cfg->exec_flags & DPEMU_X_HIST_DIRECT) repl = false;
        if (cfg->exec_flags & DPEMU_X_HIST_REPL) repl = true;
        if (repl) {
            const uint64_t stride = (pl.bins + 31) & ~31ull;     // replicas on separate 128-B lines
            pl.hist_repl = true;
            pl.R = (uint32_t)std::min<uint64_t>({64, blocks, std::max<uint64_t>(1, (2ull << 20) / (stride * 4))});
            pl.hist_stride = stride;
            pl.hist_lds = pl.bins <= HIST_LDS_MAX && (BLOCK / C) >= 4 * pl.bins;   // LDS pre-aggregation pays
        }
    }
    // branch.hip for every other program, the meas_lut back end included
    // (DPEMU_X_GENERAL / DPEMU_X_PROG_LDS: everything on the general
    // interpreter).  Its workgroup's programs are staged in LDS when they are
    // few commands: a fetch from LDS does not wait behind the lane's event
    // stores, which share vmcnt with global loads on gfx950
    // (DPEMU_X_PROG_MAJOR keeps the global fetch).
    const bool branch = states || (!uniform && !macro && !(cfg->exec_flags & (DPEMU_X_GENERAL | DPEMU_X_PROG_LDS)));
    pl.bfeat = (feat & (FEAT_FPROC | FEAT_LUT | FEAT_SYNC)) | (f.reg_writes ? FEAT_REGS : 0) | (demod ? FEAT_DEMOD : 0) |
               (states ? FEAT_STATES : 0);
    if (branch) {
        pl.prog_lds_words = 0;
        if (footprint <= BRANCH_LDS_MAX && !(cfg->exec_flags & DPEMU_X_PROG_MAJOR)) {
            pl.bfeat |= FEAT_PROG_LDS;
            pl.prog_lds_words = (uint32_t)std::max<uint64_t>(16, (footprint + 15) & ~15ull);
        }
    }
    pl.family = uniform ? K_STRAIGHT : macro ? K_MACRO : branch ? K_BRANCH : K_INTERP;
    // few bins in LDS-aggregated replicas: straight_kernel's last workgroup
    // sums them (lane.h count_outcome_block); the other kernels keep the reduce launch
    pl.hist_fold = uniform && pl.hist_repl && pl.hist_lds;
    char name[96];
    if (uniform)
        snprintf(name, sizeof name, "straight_kernel<%s,fb%d>",
                 pl.src == STRAIGHT_ROWS ? "rows" : pl.src == STRAIGHT_PROG ? "prog" : "lds", pl.fetch_batch);
    else if (macro && pl.slots)
        snprintf(name, sizeof name, "macro_staged_kernel<%d%s%s>", f.macro_nr, f.macro_addid ? ",addid" : "",
                 pl.slots > MACRO_SLOTS ? ",12" : "");
    else if (macro)
        snprintf(name, sizeof name, "macro_kernel");
    else if (branch)
        snprintf(name, sizeof name, "branch_kernel<feat=0x%x%s>", pl.bfeat, C == 8 ? ",c8" : "");
    else
        snprintf(name, sizeof name, "interp_kernel<feat=0x%x>", feat);
    pl.name = name;
    return pl;
}

// The DDS tile kernel's LDS plan (DDSParams fields of the same names) from the
// channel descriptors (DDS_CH_WORDS u32 each): the staging capacities are the
// largest tables that fit, the stripes follow the record capacity
struct DdsPlan {
    uint32_t ev_lds, rec_lds, env_lds, freq_lds, tiles, stripes, wg_tiles;
    bool dense;                             // every record staged under DDS_WG_LDS_DENSE
};

inline DdsPlan plan_dds(const uint32_t *desc, uint32_t n_channels, uint32_t n_samples, uint32_t event_cap)
{
    uint32_t env_max = 0, freq_max = 0;         // LDS staging sizes: largest tables that fit
    for (uint32_t i = 0; i < n_channels; i++) {
        const uint32_t *d = desc + (size_t)i * DDS_CH_WORDS;
        // staged words: (E, E') pairs for interp 1 (swizzled chunks), (R, R') pairs of the freq entries
        const uint32_t ew = d[3] == 1 ? dds_env_pairs_words(d[5]) : d[5], fw = 2 * d[7];
        if (ew <= DDS_ENV_LDS_MAX) env_max = std::max(env_max, ew);
        if (fw <= DDS_FREQ_LDS_MAX) freq_max = std::max(freq_max, fw);
    }
    DdsPlan p{};
    p.ev_lds = std::max<uint32_t>(8, (event_cap + 7) & ~7u);
    p.env_lds = (env_max + 3) & ~3u;
    p.freq_lds = (freq_max + 3) & ~3u;
    p.tiles = (uint32_t)(((uint64_t)n_samples + DDS_TILE - 1) / DDS_TILE);
    auto stripe_plan = [&](uint32_t per_stripe) {
        p.stripes = std::max<uint32_t>(1, (p.tiles + per_stripe - 1) / per_stripe);
        p.wg_tiles = (p.tiles + p.stripes - 1) / p.stripes;
        return dds_lds_bytes(0, p.wg_tiles, p.env_lds, p.freq_lds);
    };
    const uint32_t fixed = stripe_plan(DDS_TILES_PER_STRIPE);
    const uint32_t fit = fixed < DDS_WG_LDS_BUDGET ? (DDS_WG_LDS_BUDGET - fixed) / 20 & ~7u : 0u;
    p.rec_lds = std::min(p.ev_lds, std::max(fit, DDS_REC_LDS_MIN));
    if (p.rec_lds < p.ev_lds) {
        // dense channels: stage every record under the larger budget, with
        // more tiles per workgroup to spread its larger prologue
        if (stripe_plan(DDS_TILES_PER_STRIPE_DENSE) + p.ev_lds * 20 <= (uint32_t)DDS_WG_LDS_DENSE) {
            p.rec_lds = p.ev_lds;
            p.dense = true;
        } else {
            stripe_plan(DDS_TILES_PER_STRIPE);
        }
    }
    return p;
}

// The iq_stats grid width for n columns of C cores and S grid rows: a
// workgroup's flush is at most 26 C atomics per slot, so it gets at least
// IQ_STATS_COLS_PER_C * C columns (8 B per readout) before another workgroup
// is added; and no more workgroups than the device holds at once (all grid
// rows together): the columns are dealt round-robin, so a second, partly
// filled round of workgroups would only add a tail
inline uint32_t iq_stats_grid(uint32_t n, uint32_t C, uint64_t S, uint32_t wgs_per_cu, uint32_t n_cu)
{
    const uint64_t per_wg = std::max<uint64_t>(BLOCK, (uint64_t)IQ_STATS_COLS_PER_C * C);
    const uint64_t resident = std::max<uint64_t>(1, (uint64_t)wgs_per_cu * n_cu / S);
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(1, (n + per_wg - 1) / per_wg), resident);
}

// The feedline_trace_kernel grid: the pair table sorted by (core, spc_lo) and
// cut into chunks of one group each, and the tiles of BLOCK 4-sample groups
// that cover the longest stretch of a window any bin can take a sample from.
// tab = the chunk descriptors (TRACE_CHUNK_WORDS u32 each: core, log2 spc_lo,
// first, end) followed by perm [n_pairs].  A workgroup's flush is at most 8
// atomics per thread, so a chunk gets at least TRACE_PAIRS_PER_WG pairs (when
// its group has them) before another is added, and more when the grid (tiles
// x chunks x S layers) would exceed the workgroups the device holds at once.
struct TracePlan {
    std::vector<uint32_t> tab;
    uint32_t n_chunks = 0, tiles = 0;
};

inline TracePlan plan_traces(const uint32_t *core, const uint32_t *spc_lo, uint32_t n_pairs, uint32_t n_samples_lo,
                             uint32_t ro_cpw, uint32_t n_bins, uint32_t bin_clocks, uint32_t S, uint32_t wgs_per_cu,
                             uint32_t n_cu)
{
    TracePlan pl;
    auto log2u = [](uint32_t v) { uint32_t l = 0; while ((1u << l) < v) l++; return l; };
    std::vector<uint32_t> perm(n_pairs);
    for (uint32_t i = 0; i < n_pairs; i++) perm[i] = i;
    auto key = [&](uint32_t i) { return (core[i] << 8) | log2u(spc_lo[i]); };
    std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return key(a) < key(b); });
    uint32_t max_spc = 1;
    for (uint32_t i = 0; i < n_pairs; i++) max_spc = std::max(max_spc, spc_lo[i]);
    // samples from a window's start that can reach a bin: the bins' span, the longest window, the rows
    const uint64_t span = std::min<uint64_t>({(uint64_t)n_bins * bin_clocks * max_spc, 4096ull * ro_cpw * max_spc,
                                              (uint64_t)n_samples_lo});
    pl.tiles = (uint32_t)std::max<uint64_t>(1, ((span + 3) / 4 + BLOCK - 1) / BLOCK);
    const uint64_t resident = std::max<uint64_t>(1, (uint64_t)wgs_per_cu * n_cu / ((uint64_t)pl.tiles * S));
    const uint32_t per = (uint32_t)std::max<uint64_t>(TRACE_PAIRS_PER_WG, (n_pairs + resident - 1) / resident);
    for (uint32_t b = 0; b < n_pairs;) {
        uint32_t e = b;
        while (e < n_pairs && key(perm[e]) == key(perm[b])) e++;
        for (uint32_t k = b; k < e; k += per) {
            const uint32_t d[TRACE_CHUNK_WORDS] = {core[perm[b]], log2u(spc_lo[perm[b]]), k, std::min(k + per, e)};
            pl.tab.insert(pl.tab.end(), d, d + TRACE_CHUNK_WORDS);
        }
        b = e;
    }
    pl.n_chunks = (uint32_t)(pl.tab.size() / TRACE_CHUNK_WORDS);
    pl.tab.insert(pl.tab.end(), perm.begin(), perm.end());
    return pl;
}

// dpemu_qsim's phase tables (include/dpemu.h "phase"): out[768][2] = {cos, sin} in Q30
inline void qsim_phase_lut(int32_t *out)
{
    const double two_pi = 6.283185307179586476925286766559, one = 1073741824.0;
    for (uint32_t i = 0; i < DPEMU_QSIM_LUT_COARSE + DPEMU_QSIM_LUT_FINE; i++) {
        const double a = i < DPEMU_QSIM_LUT_COARSE ? two_pi * i / 512.0 : two_pi * (i - DPEMU_QSIM_LUT_COARSE) / 131072.0;
        out[2 * i] = (int32_t)std::lrint(std::cos(a) * one);
        out[2 * i + 1] = (int32_t)std::lrint(std::sin(a) * one);
    }
    const int32_t q[4][2] = {{1 << 30, 0}, {0, 1 << 30}, {-(1 << 30), 0}, {0, -(1 << 30)}};
    for (uint32_t k = 0; k < 4; k++) {                  // the quarter turns, exactly
        out[2 * 128 * k] = q[k][0];
        out[2 * 128 * k + 1] = q[k][1];
    }
    out[2 * DPEMU_QSIM_LUT_COARSE] = 1 << 30;
    out[2 * DPEMU_QSIM_LUT_COARSE + 1] = 0;
}

// dpemu_qsim: the checks of the host tables (include/dpemu.h lists them) and
// qsim_kernel's table -- the phase table, reg_core, slot_first (register r's
// cores own dictionary slots slot_first[r] and, for a second core, the next),
// detune [64] and the dictionary, one slot of DPEMU_QSIM_GATES_MAX entries per
// register core; lds_bytes = the phase table and the slots of the most cores a
// workgroup's BLOCK consecutive rows can belong to.  err: why the arguments
// are refused (empty: they are not).  meas: dpemu_qsim_meas's call -- the same
// table (the two calls share the uploaded copy), and cfg->meas_elem is checked
// as its readout element.
struct QsimPlan {
    std::vector<uint32_t> tab;
    uint32_t off_reg = 0, off_slot = 0, off_det = 0, off_dict = 0, lds_bytes = 0;
    std::string err;
};

inline QsimPlan plan_qsim(const dpemu_config *cfg, const dpemu_qsim_args *qs, bool meas = false)
{
    QsimPlan pl;
    char buf[160];
    auto bad = [&](const char *fmt, unsigned a = 0, unsigned b = 0) {
        snprintf(buf, sizeof buf, fmt, a, b);
        pl.err = buf;
        return pl;
    };
    const uint32_t C = cfg->cores_per_shot, none = 0xFFFFFFFFu;
    if (C == 0 || C > DPEMU_MAX_CORES || (C & (C - 1))) return bad("cores_per_shot %u is not a power of two in [1, 64]", C);
    if (cfg->lane_order > DPEMU_LANES_SHOT_MAJOR) return bad("lane_order %u is not DPEMU_LANES_CORE_MAJOR / SHOT_MAJOR", cfg->lane_order);
    if (qs->n_regs == 0) return bad("n_regs must be >= 1");
    if (!qs->reg_core) return bad("reg_core is NULL");
    if (qs->n_gates && !qs->gates) return bad("gates is NULL");
    if (qs->drv_elem > 3) return bad("drv_elem %u must be 0..3", qs->drv_elem);
    if (meas && cfg->meas_elem > 3) return bad("meas_elem %u must be 0..3", cfg->meas_elem);
    if (meas && cfg->meas_elem == qs->drv_elem) return bad("meas_elem %u is the drive element", cfg->meas_elem);
    if (qs->event_cap > DPEMU_MAX_EVENT_CAP) return bad("event_cap %u exceeds DPEMU_MAX_EVENT_CAP", qs->event_cap);
    if ((uint64_t)qs->n_lanes != qs->n_shots * C) return bad("n_lanes %u is not n_shots * cores_per_shot", qs->n_lanes);
    if (qs->n_regs > C) return bad("n_regs %u exceeds cores_per_shot %u (a core is in one register)", qs->n_regs, C);
    if ((uint64_t)qs->n_regs * qs->n_shots > (1ull << 31)) return bad("n_regs * n_shots exceeds 2^31");
    // registers: where every core sits
    uint32_t slot_of[DPEMU_MAX_CORES], second[DPEMU_MAX_CORES], lonely[DPEMU_MAX_CORES];
    std::fill(slot_of, slot_of + DPEMU_MAX_CORES, none);
    std::vector<uint32_t> slot_first(qs->n_regs + 1, 0);
    for (uint32_t r = 0; r < qs->n_regs; r++) {
        uint32_t n = 0;
        for (uint32_t q = 0; q < 2; q++) {
            const uint32_t c = qs->reg_core[2 * r + q];
            if (c == none && q == 1) continue;
            if (c >= C) return bad("register %u: core %u >= cores_per_shot", r, c);
            if (slot_of[c] != none) return bad("core %u is in two registers (the second: %u)", c, r);
            slot_of[c] = slot_first[r] + n++;
            second[c] = q;
            lonely[c] = qs->reg_core[2 * r + 1] == none;
        }
        slot_first[r + 1] = slot_first[r] + n;
    }
    const uint32_t n_slots = slot_first[qs->n_regs];
    pl.off_reg = QSIM_LUT_WORDS;
    pl.off_slot = pl.off_reg + 2 * qs->n_regs;
    pl.off_det = pl.off_slot + qs->n_regs + 1;
    pl.off_dict = pl.off_det + DPEMU_MAX_CORES;
    pl.tab.assign(pl.off_dict + (size_t)n_slots * QSIM_SLOT_WORDS, 0u);
    for (uint32_t s = 0; s < n_slots * DPEMU_QSIM_GATES_MAX; s++) pl.tab[pl.off_dict + (size_t)s * QSIM_GATE_WORDS + 1] = QSIM_NO_GATE;
    uint32_t fill[DPEMU_MAX_CORES] = {0};
    for (uint32_t g = 0; g < qs->n_gates; g++) {
        const dpemu_qsim_gate &e = qs->gates[g];
        if (e.core >= C || slot_of[e.core] == none) return bad("gate %u: core %u is in no register", g, e.core);
        if (e.kind > 1) return bad("gate %u: kind %u must be 0 or 1", g, e.kind);
        if (e.kind == 1 && (second[e.core] || lonely[e.core]))
            return bad("gate %u: kind 1 needs core %u to be the first of a two-qubit register", g, e.core);
        if (fill[e.core] == DPEMU_QSIM_GATES_MAX) return bad("more than %u entries for core %u", DPEMU_QSIM_GATES_MAX, e.core);
        for (uint32_t k = 0; k < 16; k++)
            if (e.m[k >> 3][k & 7] > (1 << 30) || e.m[k >> 3][k & 7] < -(1 << 30))
                return bad("gate %u: matrix component %u is beyond +-2^30", g, k);
        uint32_t *slot = &pl.tab[pl.off_dict + (size_t)slot_of[e.core] * QSIM_SLOT_WORDS];
        for (uint32_t k = 0; k < fill[e.core]; k++) {
            const uint32_t *o = slot + k * QSIM_GATE_WORDS;
            if (o[1] == e.freq && o[2] == e.env && o[3] == e.amp) return bad("gate %u: core %u has this key already", g, e.core);
        }
        static_assert(sizeof(dpemu_qsim_gate) == QSIM_GATE_WORDS * 4, "a dictionary entry is a dpemu_qsim_gate");
        memcpy(slot + fill[e.core]++ * QSIM_GATE_WORDS, &e, sizeof e);
    }
    qsim_phase_lut(reinterpret_cast<int32_t *>(pl.tab.data()));
    std::copy(qs->reg_core, qs->reg_core + 2 * qs->n_regs, pl.tab.begin() + pl.off_reg);
    std::copy(slot_first.begin(), slot_first.end(), pl.tab.begin() + pl.off_slot);
    if (qs->detune) std::copy(qs->detune, qs->detune + C, pl.tab.begin() + pl.off_det);
    // BLOCK consecutive rows belong to at most (BLOCK - 1) / n_shots + 2 consecutive registers
    const uint64_t span = qs->n_shots ? std::min<uint64_t>(qs->n_regs, (BLOCK - 1) / qs->n_shots + 2) : 1;
    uint32_t most = 0;
    for (uint32_t r = 0; r + span <= qs->n_regs; r++) most = std::max(most, slot_first[r + span] - slot_first[r]);
    pl.lds_bytes = (QSIM_LUT_WORDS + most * QSIM_SLOT_WORDS) * 4u;
    return pl;
}

// dpemu_qsim_decay: the checks of its own argument (plan_qsim checks the rest)
// and the kernel's decay table, a table apart from plan_qsim's: per core
// QSIM_DECAY_WORDS words, damp[32] then deph[32].  It is read from global
// memory (kernels.h QsimParams::decay), so it adds nothing to lds_bytes.
struct QsimDecayPlan {
    std::vector<uint32_t> tab;
    std::string err;
};

inline QsimDecayPlan plan_qsim_decay(const dpemu_config *cfg, const dpemu_qsim_decay_args *dec)
{
    QsimDecayPlan pl;
    char buf[160];
    auto bad = [&](const char *fmt, unsigned a = 0, unsigned b = 0) {
        snprintf(buf, sizeof buf, fmt, a, b);
        pl.err = buf;
        return pl;
    };
    const uint32_t C = cfg->cores_per_shot;
    if (C == 0 || C > DPEMU_MAX_CORES) return bad("cores_per_shot %u is not in [1, 64]", C);
    if (!dec) return bad("dec is NULL");
    if (!dec->damp) return bad("damp is NULL");
    if (!dec->deph) return bad("deph is NULL");
    for (uint32_t c = 0; c < C; c++)
        for (uint32_t i = 0; i < 32; i++) {
            if (dec->damp[32 * c + i] > (1u << 30)) return bad("damp: entry %u of core %u is above 2^30", i, c);
            if (dec->deph[32 * c + i] > (1u << 30)) return bad("deph: entry %u of core %u is above 2^30", i, c);
        }
    pl.tab.resize((size_t)C * QSIM_DECAY_WORDS);
    for (uint32_t c = 0; c < C; c++) {
        std::copy(dec->damp + 32 * c, dec->damp + 32 * c + 32, pl.tab.begin() + (size_t)c * QSIM_DECAY_WORDS);
        std::copy(dec->deph + 32 * c, dec->deph + 32 * c + 32, pl.tab.begin() + (size_t)c * QSIM_DECAY_WORDS + 32);
    }
    return pl;
}

}  // namespace dpemu
