// kernels.h -- device-side parameter blocks and launchers of libdpemu.so.
// The formats, caps and sizes the host planners share with them: uop.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dpemu.h"
#include "uop.h"

namespace dpemu {

constexpr uint32_t MEAS_LOOKUP = DPEMU_MEAS_LOOKUP;
constexpr uint32_t LUT_FIRE_CAP = DPEMU_LUT_FIRE_CAP;

// exclusive block scan of v (BLOCK threads); returns the prefix, *total the sum
__device__ __forceinline__ uint32_t block_exclusive_scan(uint32_t v, uint32_t *s_tmp, uint32_t *total)
{
    const uint32_t tid = threadIdx.x, wl = tid & 63, wv = tid >> 6;
    uint32_t x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, o, 64);
        if (wl >= (uint32_t)o) x += y;
    }
    if (wl == 63) s_tmp[wv] = x;
    __syncthreads();
    uint32_t off = 0, tot = 0;
#pragma unroll
    for (uint32_t k = 0; k < BLOCK / 64; k++) {
        const uint32_t t = s_tmp[k];
        off += (k < wv) ? t : 0u;
        tot += t;
    }
    __syncthreads();
    *total = tot;
    return off + x - v;
}

constexpr uint32_t ST_DONE = DPEMU_ST_DONE, ST_MAX_CYCLES = DPEMU_ST_MAX_CYCLES;
constexpr uint32_t ST_HUNG_OPCODE = DPEMU_ST_HUNG_OPCODE, ST_DEADLOCK = DPEMU_ST_DEADLOCK;
constexpr uint32_t F_LATE = DPEMU_F_LATE, F_EVENT_OVF = DPEMU_F_EVENT_OVF;
constexpr uint32_t F_TRACE_OVF = DPEMU_F_TRACE_OVF, F_MEAS_OVF = DPEMU_F_MEAS_OVF;
constexpr uint32_t F_DOUBLE_STROBE = DPEMU_F_DOUBLE_STROBE, F_GUARD = DPEMU_F_GUARD;
constexpr uint32_t TRACE_QCLK_LOAD = DPEMU_TRACE_QCLK_LOAD, TRACE_QCLK_RST = DPEMU_TRACE_QCLK_RST;

struct KParams {
    // programs, as decode_cmd words (16 B per command)
    const uint4 *uops;            // program-major: program p's command i at offsets[p] + i
    const uint4 *fetch;           // the image the loop fetches from: command i of program p at
    uint32_t fetch_stride;        //   i * fetch_stride + (stride 1 ? offsets[p] : p); stride = the
                                  //   program count selects the command-major copy (zero past a
                                  //   program's end), where adjacent lanes -- adjacent programs --
                                  //   fetch adjacent commands
    const uint32_t *offsets, *n_instr, *prog_table;   // uops: a zero guard command follows every program
    uint32_t max_len;             // longest program; the command-major image's guard row
    const uint4 *macros;          // macro.hip image: 2 x uint4 per macro (program_image.h build_macros)
    const uint32_t *macro_off;    // [n_programs + 1]: program p's macros [macro_off[p], macro_off[p + 1])
    const uint32_t *macro_chunk;  // per (program, MACRO_CHUNK-macro chunk): the largest pulse cmd_time of a
                                  //   chunk whose macros are all MACRO_SIMPLE (0: no pulse), else
                                  //   MACRO_CHUNK_MIXED (program_image.h mark_lean_chunks)
    const uint32_t *macro_coff;   // [n_programs]: program p's chunk c at macro_chunk[macro_coff[p] + c]
    uint64_t reg_map;             // macro image register slots: reg_file register r is slot (reg_map >> 4 r) & 15
    uint64_t reg_inv;             //   for r in the reg_used mask (others are never named: they read 0);
    uint32_t reg_used;            //   slot s holds register (reg_inv >> 4 s) & 15 (trace addresses)
    uint32_t macro_rs;            // UOP_RS_* fields some pulse slot of the macro image register-sources
    uint32_t macro_w3;            // the macro image is MACRO_W3 (three ALU slots; always with 2 register slots)
    const uint32_t *p1_thr;
    const uint64_t *lut_table;
    // outputs (device, nullable); lane L = core * n_shots + shot (core-major)
    uint32_t *summary;
    uint4 *events;                // {t, env | cfg << 24 | kind << 28, phase | freq << 17, amp}
    uint4 *trace;
    uint2 *meas;
    uint32_t *regs_out;
    unsigned long long *hist;
    // run
    uint64_t shot_begin;
    uint32_t n_lanes, n_shots, C, log2C, n_groups, shots_per_group;
    uint32_t shot_major;          // dpemu_config.lane_order: lane = shot * C + core (else core * n_shots + shot)
    uint32_t grp_g0, grp_r0;      // (shot_begin / spg) % n_groups, shot_begin % spg
    uint32_t spg_div[3], ng_div[3];   // FastDiv of shots_per_group / n_groups (shot_group)
    uint32_t max_cycles, event_cap, trace_cap, meas_cap;
    uint32_t fproc_mode, meas_elem, meas_latency, sync_latency;
    uint64_t sync_mask, seed;
    uint32_t lut_mask;
    uint32_t meas_model;          // DPEMU_MEAS_STATE / DPEMU_MEAS_READOUT (ro_*: include/dpemu.h)
    int32_t ro_sep, ro_thr;
    uint32_t ro_sigma, ro_win, ro_wrecip;   // ro_wrecip = floor(2^24 / ro_win)
    // DEMOD readout model (lane.h demod_readout): config fields, the per-core
    // axes, the frequency tables (dpemu_load_readout_freqs) and the acc output
    uint32_t ro_drv_elem, ro_cpw, ro_delay, ro_theta0, ro_theta1, ro_gain0, ro_gain1;
    const uint32_t *ro_axis;      // [64] Q15 I | Q << 16
    const uint32_t *ro_fq;        // frequency words
    const uint4 *ro_hdr;          // [n_programs] {drv_off, drv_len, lo_off, lo_len}
    int2 *acc;                    // dpemu_outputs.acc (nullable)
    uint32_t iter_guard;
    uint32_t ev_stream;           // DPEMU_X_STREAM_EVENTS: the macro kernels' event rows nontemporal
    uint32_t prog_lds_words;      // dynamic LDS commands (FEAT_PROG_LDS)
    uint32_t hist_fold;           // straight_kernel reduces the replicas itself (lane.h fold_replicas) into hist
                                  //   = out->hist: HIST_FOLD_ADD adds the sums, HIST_FOLD_ASSIGN stores them; 0: the
                                  //   reduce launch does.  (In what was padding: the block's other offsets stay)
    uint32_t *hist_rep;           // [hist_reps][hist_stride] u32 replicas (128-B aligned rows); with hist_fold
                                  //   hist_reps + 1 tickets follow, HIST_TICKET_PITCH words apart
    uint32_t hist_reps, hist_lds; // hist_lds: n_groups << C <= HIST_LDS_MAX, aggregate in LDS
    uint64_t hist_stride;
    unsigned long long *hist_next;  // dpemu_outputs.hist_next (nullable): zeroed by the kernel
    uint64_t hist_bins;             // n_groups << C (hist_next's words)
    const uint32_t *states;         // dpemu_run_states (branch_kernel<FEAT_STATES>): [n_lanes] words in the run's
                                    //   lane order, readout m's prepared state in bit m; no other kernel reads it
};

hipError_t launch_hist_reduce(uint32_t *rep, uint32_t R, uint64_t stride, uint64_t bins, bool assign,
                              unsigned long long *hist, hipStream_t stream);

hipError_t launch_interp(const KParams &p, int feat, hipStream_t stream);
// pulse-only programs (straight.hip); src: where commands are fetched from (STRAIGHT_*);
// fb: commands fetched per batch (1 or 4)
hipError_t launch_straight(const KParams &p, int src, int fb, hipStream_t stream);
// dynamic LDS above 64 KiB for kernel `fn` on the current device: the opt-in,
// recorded per (device, kernel) under a lock (capi.cpp, lds_grants.h)
hipError_t opt_in_dynamic_lds(const void *fn, size_t bytes);
// programs with jumps / fproc_meas / sync (branch.hip): FEAT_FPROC | FEAT_SYNC | FEAT_REGS | FEAT_PROG_LDS bits of feat;
// with FEAT_STATES (branch_states.hip) any program, its prepared states read from p.states
hipError_t launch_branch(const KParams &p, int feat, hipStream_t stream);
// branch-free programs with reg_alu / inc_qclk (macro.hip; the kernel choice: uop.h MACRO_SLOTS)
// addid: every ALU slot of the image is reg_alu id0 / add (RB phase updates)
// slots: 0 = macro_kernel (per-lane fetch), else the staged kernel's program slots per wave
hipError_t launch_macro(const KParams &p, uint32_t slots, int nr, bool addid, hipStream_t stream);

// ---- DDS ------------------------------------------------------------------
// Two launches per synthesis (dds.hip): dds_index_kernel compacts each
// channel's strobes and pulse resets once and writes every sample tile's
// window of them; dds_tile_kernel, grid (DDS stripes, channels), sweeps the
// tiles of a channel round-robin over its stripe workgroups, so the
// workgroups of a channel write adjacent tiles at the same time.
struct DDSParams {
    const uint32_t *summary;
    const uint4 *events;           // dpemu_run event records, slot-major
    const uint32_t *env, *freq;
    const int16_t *sin_lut;        // Q15 sine table [4096]
    const uint32_t *ch;            // per-channel descriptors, DDS_CH_WORDS u32 each
    uint32_t *iq;                  // [n_channels][n_samples] packed {I16 low, Q16 high}
    uint32_t n_channels, n_lanes, n_samples, event_cap;
    uint32_t ev_lds;               // compacted-event slots per channel (>= event_cap, multiple of 8)
    uint32_t rec_lds;              // strobe records / reset times a tile workgroup stages in LDS (<= ev_lds)
    uint32_t env_lds, freq_lds;    // LDS staging capacity for a channel's env / freq table (words, as staged)
    uint32_t tiles;                // tile windows per channel (DDS_TILE samples each)
    uint32_t stripes;              // tile workgroups per channel
    uint32_t wg_tiles;             // most tiles one workgroup sweeps (its LDS window slots)
    // event index (dds_index_kernel -> dds_tile_kernel)
    uint4 *xs;                     // [n_channels][ev_lds] strobes {t, env word, phase | freq << 17, amp}
    uint32_t *xr;                  // [n_channels][ev_lds] pulse_reset times
    uint2 *cnt;                    // [n_channels] {strobes, resets}
    uint32_t pair_lanes;           // channels 2i, 2i + 1 share a lane (one index workgroup per pair)
};

hipError_t launch_dds_index(const DDSParams &p, hipStream_t stream);
hipError_t launch_dds(const DDSParams &p, hipStream_t stream);

// ---- waveform demodulation (demod_iq.hip, dpemu_demod_iq) -------------------
// demod_iq_kernel, grid (meas_cap, pairs): one workgroup accumulates one
// readout of one (drive channel, LO channel) pair; readout_result_kernel
// (this stage's and dpemu_demod_feedline's) then packs each pair's outcome
// bits from the stored {I, Q}: result[pr].y from acc[m][pr], m < result[pr].x.
// The pair descriptor's words: uop.h PAIR_*.
struct DemodParams {
    const uint32_t *summary;
    const uint4 *events;           // dpemu_run event records, slot-major
    const uint32_t *iq_drv, *iq_lo;   // dpemu_dds output rows, {I16 low, Q16 high}
    const int16_t *sin_lut;        // Q15 sine table [4096]
    const uint32_t *pairs;         // per-pair descriptors, DEMOD_PAIR_WORDS u32 each
    int2 *acc;                     // [meas_cap][n_pairs] {I, Q}
    uint2 *result;                 // [n_pairs] {count, outcome bits}
    uint32_t n_pairs, n_lanes, event_cap, meas_cap;
    uint32_t n_samples_drv, n_samples_lo;
    uint64_t seed;
    uint32_t meas_elem, ro_cpw, ro_delay, ro_theta0, ro_theta1, ro_gain0, ro_gain1, ro_sigma;
    int32_t ro_thr;
};

hipError_t launch_demod_iq(const DemodParams &p, hipStream_t stream);
hipError_t launch_readout_result(const uint32_t *pairs, const int2 *acc, uint2 *result, uint32_t n_pairs, int32_t ro_thr,
                                 hipStream_t stream);

// ---- multiplexed readout (feedline.hip, dpemu_feedline_adc / dpemu_demod_feedline) ----
// feedline_index_kernel (one workgroup per pair) writes each pair's kept
// readouts, their count and prepared states to `rd` / `hdr`;
// feedline_adc_kernel, grid (sample tiles, lines), sums the members' returns
// into the line's ADC row; feedline_demod_kernel, grid (meas_cap, pairs),
// mixes that row with the pair's LO; readout_result_kernel packs the bits.
// Pair descriptors are dpemu_demod_iq's (DEMOD_PAIR_WORDS).
struct FeedlineParams {
    const uint32_t *summary;
    const uint4 *events;           // dpemu_run event records, slot-major
    const uint32_t *iq_drv, *iq_lo;   // dpemu_dds output rows (iq_drv: the ADC stage; iq_lo: the demodulator)
    const int16_t *sin_lut;        // Q15 sine table [4096]
    const uint32_t *pairs;         // per-pair descriptors, DEMOD_PAIR_WORDS u32 each
    const uint32_t *line_first;    // [n_lines + 1] CSR offsets into member
    const uint32_t *member;        // pair indices, line by line
    const uint32_t *line_of;       // [n_pairs] the pair's line (the demodulator: every pair has one)
    uint2 *rd;                     // [n_pairs][FEEDLINE_RD_SLOTS] kept readouts {t_lo, env word}; unused: t = 2^32 - 1
    uint2 *hdr;                    // [n_pairs] {count, prepared state of readout m in bit m (bit 0 always drawn)}
    uint32_t *adc;                 // [n_lines][n_samples_lo] {I16 low, Q16 high}
    int2 *acc;                     // [meas_cap][n_pairs] {I, Q}
    uint2 *result;                 // [n_pairs] {count, outcome bits}
    uint32_t n_pairs, n_lines, n_lanes, event_cap, meas_cap;
    uint32_t n_samples_drv, n_samples_lo;
    uint64_t seed;
    uint32_t meas_elem, ro_cpw, ro_delay, ro_theta0, ro_theta1, ro_gain0, ro_gain1, ro_sigma;
    int32_t ro_thr;
    const uint32_t *states;        // [n_lanes] the *_st calls: readout m's state in bit m of the lane's word,
                                   //   in place of the draw (null: the draw)
};

hipError_t launch_feedline_index(const FeedlineParams &p, hipStream_t stream);
hipError_t launch_feedline_adc(const FeedlineParams &p, hipStream_t stream);
hipError_t launch_feedline_demod(const FeedlineParams &p, hipStream_t stream);

// ---- resonator response (resonator.hip, dpemu_feedline_adc_res) -------------
// feedline_res_kernel, one single-wave workgroup per run of whole lines with
// at most RES_MEMBERS members (packed greedily by the host: wg_first, after
// line_of in the line table): a lane owns one member's one-pole recurrence
// and walks the LO samples in tiles of RES_TILE.  Reads the index
// feedline_index_kernel wrote (f.rd / f.hdr).
struct ResonatorParams {
    FeedlineParams f;
    const int4 *coef;              // [n_pairs][2 states] {pole_re, pole_im, coup_re, coup_im}, Q30; then one zero int4
    const uint32_t *wg_first;      // [n_wgs + 1] the workgroups' first lines
    uint32_t n_wgs, adc_sigma;
};

hipError_t launch_feedline_res(const ResonatorParams &p, hipStream_t stream);

// ---- averaged readout traces (traces.hip, dpemu_feedline_traces) ------------
// feedline_trace_kernel, grid (sample tiles, chunks, by_slot ? meas_cap : 1): a
// workgroup takes a chunk of the pairs of one (core, spc_lo) group (the host
// sorts them: launch_plan.h plan_traces) and BLOCK groups of 4 LO samples
// counted from each readout's window start; it stages its pairs' windows in
// LDS from the index feedline_index_kernel wrote (f.rd / f.hdr), then a thread
// sums its 4 samples' products per prepared state in registers and adds them
// to `traces` (zeroed by the host before the launch) at the end.
struct TraceParams {
    FeedlineParams f;
    const uint4 *chunks;           // [n_chunks] {core, log2 spc_lo, first, end}: pairs perm[first .. end)
    const uint32_t *perm;          // [n_pairs] pair indices, sorted by (core, spc_lo)
    unsigned long long *traces;    // [S][C][2][n_bins][DPEMU_TRACE_WORDS] int64
    uint32_t n_chunks, tiles, n_bins, bin_clocks, by_slot, C;
};

uint32_t trace_wgs_per_cu();        // resident workgroups per CU (occupancy query), 0 = unknown
hipError_t launch_feedline_trace(const TraceParams &p, hipStream_t stream);

// ---- readout IQ statistics (iq_stats.hip, dpemu_iq_stats) --------------------
// iq_stats_kernel, grid (gx, by_slot ? meas_cap : 1): one streaming pass over
// acc that sums the 16 words of every (slot, core, prepared state) class into
// `stats` (zeroed by the host before the launch) and packs the re-discriminated
// outcome bits.  The per-core constants travel by value (768 B).
struct IqStatsParams {
    const int2 *acc;               // [meas_cap][n_cols] {I, Q}
    const uint32_t *counts;        // readouts of column c at counts[c * count_stride]
    unsigned long long *stats;     // [S][C][2][DPEMU_IQ_STAT_WORDS] int64, S = by_slot ? meas_cap : 1
    uint32_t *bits;                // [n_cols], nullable
    const uint64_t *x_shot;        // explicit columns: global shot and core of each, else null: the run
    const uint32_t *x_core;        //   layout (lane order, C, shot_begin, n_shots = n_cols / C)
    uint64_t seed, shot_begin;
    uint32_t n_cols, meas_cap, by_slot, count_stride;
    uint32_t C, log2C, shot_major, n_shots;
    uint32_t ns_div[3];            // FastDiv of n_shots (core-major: core = col / n_shots)
    uint32_t red_c;                // cores a wave's lanes hold in the pattern lane & (red_c - 1): C for
                                   //   shot-major lanes, else 1 (checked per wave, iq_stats.hip)
    uint32_t p1[DPEMU_MAX_CORES];  // dpemu_config.p1_threshold
    uint32_t axis[DPEMU_MAX_CORES];
    int32_t thr[DPEMU_MAX_CORES];
    const uint32_t *states;        // [n_cols] dpemu_iq_stats_st: readout m's state in bit m of the column's
                                   //   word, in place of the draw (null: the draw)
};

uint32_t iq_stats_wgs_per_cu();     // resident workgroups per CU (occupancy query), 0 = unknown
hipError_t launch_iq_stats(const IqStatsParams &p, uint32_t gx, hipStream_t stream);

// ---- qubit state from the drive pulses (qsim.hip, dpemu_qsim / dpemu_qsim_meas / dpemu_qsim_decay) ----
// qsim_kernel<MEAS, DECAY>, one thread per (register, shot) row, rows register-major.  `tab`
// is the host's table (launch_plan.h plan_qsim): the phase table, the register
// cores, each register's first dictionary slot, the detunings and the
// dictionary, a slot of DPEMU_QSIM_GATES_MAX entries per register core in
// register order.  A workgroup stages the phase table and the slots of the
// registers its rows belong to in lds_bytes of dynamic LDS.
struct QsimParams {
    const uint32_t *summary;
    const uint4 *events;           // dpemu_run event records, slot-major
    const uint32_t *tab;           // words: lut [1536] | reg_core [2 n_regs] | slot_first [n_regs + 1] | detune [64] | dict
    unsigned long long *pops;      // [n_regs][n_shots][4]
    uint4 *result;                 // [n_regs][n_shots] {outcome, n_gates, n_unmatched, n_errors | ovf << 31}
    uint64_t seed, shot_begin;
    uint32_t n_regs, n_shots, n_rows, n_lanes, event_cap, C, shot_major, drv_elem;
    uint32_t ns_div[3];            // FastDiv of n_shots (register = row / n_shots)
    uint32_t off_reg, off_slot, off_det, off_dict;   // word offsets into tab
    uint32_t lds_bytes;            // phase table + the most dictionary slots one workgroup stages
    // dpemu_qsim_meas (qsim_kernel<true>): strobes of element meas_elem measure
    uint32_t meas;                 // 1: launch the measuring instantiation
    uint32_t meas_elem;
    uint32_t *states;              // [n_lanes] post-measurement bit of the lane's readout m in bit m (zeroed by the host)
    // dpemu_qsim_decay (qsim_kernel<MEAS, true>): a qubit is advanced over the clocks since its last advance
    // before a gate or a readout acts on it.  The table stays in global memory: a row reads popcount(dt) entries
    // of its core's 256 bytes per advance, and 16 KB at 64 cores are cache-resident
    const uint32_t *decay;         // [C][64] Q30: damp[32], then deph[32] of the core (null: no decay instantiation)
    uint32_t *counts;              // [n_regs][n_shots][4] {jumps, flips} of the first qubit, then the second's; nullable
    uint32_t t_final;              // != 0: every qubit is advanced to this clock before pops are taken
};

hipError_t launch_qsim(const QsimParams &p, hipStream_t stream);

}  // namespace dpemu
