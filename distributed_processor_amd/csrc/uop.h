// uop.h -- the formats and sizes host and device share: the pre-decoded
// command, the macro image's bit positions, the LDS caps and table sizes the
// host planners (program_image.h, launch_plan.h) and the kernels both read.
// Nothing from HIP: it compiles with a plain C++ compiler.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define DPEMU_HD __host__ __device__
#else
#define DPEMU_HD
#endif

namespace dpemu {

constexpr uint32_t BLOCK = 256;                 // 4 wavefronts per workgroup

// kernel specialisations, chosen per run from the opcodes the programs use
constexpr int FEAT_FPROC = 1;   // fproc_meas reads (ALU_FPROC / JUMP_FPROC)
constexpr int FEAT_SYNC = 2;    // SYNC barriers
constexpr int FEAT_LUT = 4;     // fproc_lut back end
constexpr int FEAT_PROG_LDS = 8; // the workgroup's programs staged in LDS (fits PROG_LDS_MAX)
constexpr int FEAT_STRAIGHT = 16; // only pulse / idle / done / hang opcodes: no register file
constexpr int FEAT_REGS = 32;   // branch.hip: some command writes the reg_file (reg_alu / alu_fproc)
constexpr int FEAT_DEMOD = 64;  // branch.hip: meas_model DPEMU_MEAS_DEMOD (lane.h demod_readout)
constexpr int FEAT_STATES = 128; // branch.hip: prepared states from the caller's words (dpemu_run_states), not drawn
constexpr uint32_t PROG_LDS_MAX = 1024;   // commands (16 KiB) of dynamic LDS per workgroup
constexpr uint32_t BRANCH_LDS_MAX = 512;  // commands (8 KiB): branch.hip stages its programs up to this

// Pre-decoded command: dpemu_load_programs re-packs every 128-bit cmd_mem
// word (decode_cmd) so the interpreter reads fields at fixed 32-bit
// positions instead of slicing hdl/proc.sv:89-107's layout (the same 16
// bytes per command):
//   x  cmd_time (cmd[36:5]) for pulse / idle; ALU immediate in0 (cmd[119:88])
//   y  op4[31:28]; pulse writes: env[23:0] cfg[27:24] immediates (zero when the
//      field is not written or register-sourced); other ops: alu[2:0]
//      in0_reg[3] rs1[7:4] rd[11:8]
//   z  pulse writes: phase[16:0] freq[25:17] immediates (bits 31:26 zero);
//      other ops: target[15:0] fproc_id[23:16]
//   w  rs0[23:20] (cmd[119:116]); pulse writes: amp[15:0] immediate,
//      register-sourced env[16] phase[17] freq[18] amp[19], write enables
//      env[24] cfg[25] phase[26] freq[27] amp[28] (hdl/pulse_reg.sv:38-97),
//      any register-sourced field[29]
constexpr uint32_t UOP_RS_ENV = 1u << 16, UOP_RS_PH = 1u << 17, UOP_RS_FR = 1u << 18, UOP_RS_AMP = 1u << 19;
constexpr uint32_t UOP_ANY_RS = 1u << 29;

DPEMU_HD inline void decode_cmd(const uint32_t w[4], uint32_t u[4])
{
    const uint32_t op4 = w[3] >> 28;
    const uint32_t rs0 = (w[3] >> 20) & 15u;
    u[0] = (op4 == 0x9 || op4 == 0xC) ? ((w[0] >> 5) | (w[1] << 27)) : ((w[2] >> 24) | (w[3] << 8));
    u[1] = (op4 << 28) | ((w[3] >> 24) & 7u) | (((w[3] >> 27) & 1u) << 3) | (((w[2] >> 20) & 15u) << 4) |
           (((w[2] >> 16) & 15u) << 8);
    u[2] = ((w[2] >> 4) & 0xFFFFu) | (((w[1] >> 20) & 0xFFu) << 16);
    u[3] = rs0 << 20;
    if (op4 == 0x8 || op4 == 0x9) {
        const uint32_t env_i = ((w[2] >> 26) | (w[3] << 6)) & 0xFFFFFFu, ph_i = (w[2] >> 7) & 0x1FFFFu;
        const uint32_t fr_i = ((w[1] >> 28) | (w[2] << 4)) & 0x1FFu, amp_i = (w[1] >> 10) & 0xFFFFu;
        const uint32_t cfg_i = (w[1] >> 5) & 0xFu;
        const uint32_t env_we = (w[3] >> 19) & 1u, env_rs = (w[3] >> 18) & 1u;
        const uint32_t ph_we = (w[2] >> 25) & 1u, ph_rs = (w[2] >> 24) & 1u;
        const uint32_t fr_we = (w[2] >> 6) & 1u, fr_rs = (w[2] >> 5) & 1u;
        const uint32_t amp_we = (w[1] >> 27) & 1u, amp_rs = (w[1] >> 26) & 1u;
        const uint32_t cfg_we = (w[1] >> 9) & 1u;
        const uint32_t rs = (env_we & env_rs) | ((ph_we & ph_rs) << 1) | ((fr_we & fr_rs) << 2) | ((amp_we & amp_rs) << 3);
        u[1] = (op4 << 28) | (env_we && !env_rs ? env_i : 0u) | (cfg_we ? cfg_i << 24 : 0u);
        u[2] = (ph_we && !ph_rs ? ph_i : 0u) | (fr_we && !fr_rs ? fr_i << 17 : 0u);
        u[3] = (rs0 << 20) | (amp_we && !amp_rs ? amp_i : 0u) | (rs << 16) | (env_we << 24) | (cfg_we << 25) |
               (ph_we << 26) | (fr_we << 27) | (amp_we << 28) | ((rs ? 1u : 0u) << 29);
    }
}

// Division of a 32-bit n by a run constant d >= 1 without a divide sequence
// (Hacker's Delight 10-8, unsigned): l = ceil(log2 d), m = floor(2^32 (2^l -
// d) / d) + 1 < 2^32, q = (t + ((n - t) >> min(l, 1))) >> max(l - 1, 0) with
// t = mulhi(m, n); exact for every n < 2^32 (tests/test_fast_div.py checks the
// formula).  A runtime-divisor u32 division costs ~20 VALU per lane.
inline void fast_div_init(uint32_t d, uint32_t out[3])
{
    uint32_t l = 0;
    while (l < 32 && (1ull << l) < d) l++;
    out[0] = (uint32_t)(((1ull << 32) * ((1ull << l) - d)) / d + 1);
    out[1] = l < 1 ? l : 1u;
    out[2] = l > 1 ? l - 1 : 0u;
}

constexpr uint32_t HIST_LDS_MAX = 1024;   // histogram bins a workgroup pre-aggregates in LDS (KParams::hist_lds)
// The folded reduce (KParams::hist_fold, lane.h count_outcome_block): R + 1
// ticket words follow the R replica rows, one per row and one for the rows,
// each on a 128-B line of its own
constexpr uint32_t HIST_TICKET_PITCH = 32;   // u32 words between tickets
enum { HIST_FOLD_ADD = 1, HIST_FOLD_ASSIGN = 2 };   // KParams::hist_fold

// pulse-only programs (straight.hip); src: where commands are fetched from
enum { STRAIGHT_ROWS = 0, STRAIGHT_PROG = 1, STRAIGHT_LDS = 2 };
constexpr uint32_t STRAIGHT_LDS_MAX = 9216;   // commands (144 KiB) of dynamic LDS per workgroup

// branch-free programs with reg_alu / inc_qclk (macro.hip): macro_staged_kernel
// when every wave runs at most MACRO_SLOTS distinct programs (nr = the
// register slots the macro image names: 2, else 16 in LDS), or at most
// MACRO_SLOTS_WIDE with nr == 2, else macro_kernel (slots = 0)
constexpr uint32_t MACRO_SLOTS = 8;     // distinct programs per wave whose macros are staged in LDS
constexpr uint32_t MACRO_SLOTS_WIDE = 12;   // ... for runs whose waves span 9-12 programs (NR == 2 images)
constexpr uint32_t MACRO_CHUNK = 16;    // macros per program per staged chunk (8: 3.84-4.12 vs 3.60 ms)
constexpr uint32_t MACRO_ABSENT = 0x80000000u;   // pulse slot w bit 31: no command; ALU ctl bit 31: present
// pulse slot w bit 30 (program_image.h mark_simple_macros): not a program's first
// macro, its ALU slots are reg_alu (no inc_qclk) and its pulse slot is a
// PULSE_WRITE_TRIG or absent -- the shape macro_staged_kernel retires on its
// lean path (runtime conditions permitting)
constexpr uint32_t MACRO_SIMPLE = 0x40000000u;
constexpr uint32_t MACRO_CHUNK_MIXED = 0xFFFFFFFFu;   // macro_chunk: not every macro MACRO_SIMPLE
// MACRO_W3 image (KParams::macro_w3; the image names at most 2 registers):
// THREE ALU slots in the same 32 B, {imm0, packed ctl, imm1, imm2} + pulse
// slot.  Slot k's ctl is the 9-bit field at bit 10 k: op[2:0] in0_reg[3]
// rs1[4] rd[5] rs0[6] inc_qclk[7] present[8] (register fields are slots 0 /
// 1 after program_image.h remap_macro_regs).  w3_ctl expands a field to the legacy
// ctl layout (present[31] inc_qclk[30] rs0[15:12] rd[11:8] rs1[7:4]
// in0_reg[3] op[2:0]); w3_pack is its inverse on 1-bit register fields.
constexpr uint32_t W3_OP = 0, W3_IN0 = 3, W3_RS1 = 4, W3_RD = 5, W3_RS0 = 6, W3_INC = 7, W3_PRES = 8;
DPEMU_HD inline uint32_t w3_ctl(uint32_t packed, int k)
{
    const uint32_t f = packed >> (10 * k);
    return (f & 0x1Fu) | (((f >> W3_RD) & 1u) << 8) | (((f >> W3_RS0) & 1u) << 12) | (((f >> W3_INC) & 1u) << 30) |
           (((f >> W3_PRES) & 1u) << 31);
}
DPEMU_HD inline uint32_t w3_pack(uint32_t ctl)
{
    if (!(ctl >> 31)) return 0u;
    return (ctl & 0x1Fu) | (((ctl >> 8) & 1u) << W3_RD) | (((ctl >> 12) & 1u) << W3_RS0) |
           (((ctl >> 30) & 1u) << W3_INC) | (1u << W3_PRES);
}

// ---- DDS (dds.hip; DDSParams in kernels.h) ----------------------------------
constexpr uint32_t DDS_CH_WORDS = 8;   // lane, elem, spc, interp, env_off, env_len, freq_off, freq_len
constexpr uint32_t DDS_MAX_EVENTS = 1024;
constexpr uint32_t DDS_TILE = 4 * BLOCK;      // samples per tile: 4 per thread, one 16-B store each
// tiles per stripe workgroup: 8 / 12 / 20 / 24 / 32 measured 0.419 / 0.346 /
// 0.315 / 0.325 / 0.345 ms against 0.313 for 16 (config 5)
#ifndef DDS_TILES_PER_STRIPE
#define DDS_TILES_PER_STRIPE 16u
#endif
constexpr uint32_t DDS_ENV_LDS_MAX = 8192;    // words: tables up to 32 KiB are staged in LDS
constexpr uint32_t DDS_FREQ_LDS_MAX = 2048;   // words: 64 freq entries as (R, R') pairs

// dynamic LDS bytes of dds_tile_kernel: quarter sine table (entries
// 0..1031) | strobe records (16 B) | reset times | tile windows | env | freq |
// the cycle sweep's per-wave store transpose (1 KiB per wave)
constexpr uint32_t DDS_LUT_BYTES = 1032 * 2;
constexpr uint32_t DDS_XPOSE_BYTES = (BLOCK / 64) * 1024;
DPEMU_HD inline uint32_t dds_lds_bytes(uint32_t rec_lds, uint32_t tiles_per_stripe, uint32_t env_lds,
                                       uint32_t freq_lds)
{
    return DDS_LUT_BYTES + rec_lds * 20 + tiles_per_stripe * 16 + (env_lds + freq_lds) * 4 + DDS_XPOSE_BYTES;
}
// LDS budget of a tile workgroup: 8 workgroups (32 waves, the VGPR-bound
// occupancy) share a CU's 160 KiB.  The record capacity is what is left of
// it (at least DDS_REC_LDS_MIN); a stripe whose window holds more strobes or
// resets than that reads them from the global index instead.
// (less 512 B: the compiler's static LDS of the kernel, so 8 fit in 160 KiB)
constexpr uint32_t DDS_WG_LDS_BUDGET = 20 * 1024 - 512;
constexpr uint32_t DDS_REC_LDS_MIN = 64;
// Dense channels (more strobes than the 20-KiB budget holds, e.g. depth-200
// two-qubit RB drive channels, ~560-720 strobes): every record is staged when
// the workgroup then stays within this larger budget (fewer workgroups per CU,
// but no sweep reading records from the global index)
#ifndef DDS_WG_LDS_DENSE
#define DDS_WG_LDS_DENSE (32 * 1024 - 512)
#endif
// tiles per stripe workgroup under the dense budget (5 workgroups per CU
// instead of 8): config 5 on the two-qubit RB timelines, 16 / 20 / 22 / 24 /
// 26 / 28 / 32 tiles: 0.892 / 0.809 / 0.795 / 0.780 / 0.785 / 0.859 / 0.861
// ms (profiles/r06_dds_dense_ab.json); the sparse case keeps 16
#ifndef DDS_TILES_PER_STRIPE_DENSE
#define DDS_TILES_PER_STRIPE_DENSE 24u
#endif

// LDS words of an interp-1 envelope of n words staged as swizzled (E, E')
// pairs (dds.hip env_pair): whole groups of 8 16-B chunks
DPEMU_HD inline uint32_t dds_env_pairs_words(uint32_t n) { return (2 * n + 31) & ~31u; }

// bytes of the event index (xs, xr, cnt)
inline uint64_t dds_index_bytes(uint32_t n_channels, uint32_t ev_lds)
{
    return (uint64_t)n_channels * ev_lds * 20 + (uint64_t)n_channels * 8;
}

// ---- readout stages ----------------------------------------------------------
// pair descriptor of dpemu_demod_iq and the feedline stages (stage_plan.h describe_pairs writes it): the
// pair's lane, core, global shot, rows of iq_drv / iq_lo and their rates, then the core's p1 threshold and axis
enum {
    PAIR_LANE, PAIR_CORE, PAIR_SHOT_LO, PAIR_SHOT_HI, PAIR_DRV_ROW, PAIR_LO_ROW, PAIR_SPC_DRV, PAIR_SPC_LO,
    PAIR_P1_THR, PAIR_AXIS
};
constexpr uint32_t DEMOD_PAIR_WORDS = PAIR_AXIS + 1;
DPEMU_HD inline uint64_t pair_shot(const uint32_t *d) { return (uint64_t)d[PAIR_SHOT_LO] | ((uint64_t)d[PAIR_SHOT_HI] << 32); }
constexpr uint32_t FEEDLINE_RD_SLOTS = 32;      // readout slots per pair of the index (meas_cap <= 32)

#ifndef RES_MEMBERS_PER_WG
#define RES_MEMBERS_PER_WG 16
#endif
constexpr uint32_t RES_MEMBERS = RES_MEMBERS_PER_WG;   // members per workgroup (<= RES_WAVE: one lane each in the walk)
constexpr uint32_t RES_WAVE = 64;               // threads per workgroup
constexpr uint32_t RES_TILE = 64;               // LO samples per time tile: one per lane in the gather and the sum

// the workgroups of feedline_res_kernel: consecutive whole lines, greedily, <= RES_MEMBERS members each
// (line_first: CSR offsets of n_lines lines of 1..DPEMU_FEEDLINE_MAX members); appends n_wgs + 1 line offsets
template <class Vec> inline void res_pack_lines(const uint32_t *line_first, uint32_t n_lines, Vec &out)
{
    uint32_t begin = 0;
    out.push_back(0u);
    for (uint32_t l = 0; l < n_lines; l++)
        if (line_first[l + 1] - line_first[begin] > RES_MEMBERS) {
            out.push_back(l);
            begin = l;
        }
    out.push_back(n_lines);
}

// iq_stats_kernel: columns per workgroup before the grid grows: a workgroup's
// flush is at most 26 C atomics per slot, its stream 8 B per readout
constexpr uint32_t IQ_STATS_COLS_PER_C = 128;

// feedline_trace_kernel: pairs of one (core, spc_lo) group per workgroup before the grid grows.  A thread's
// flush is at most 8 atomics per bin it holds (2 states x 4 words), its stream 32 B (16 of each row) per
// pair and readout: 64 pairs of one readout stream 2 KiB per thread against those 8 atomics.  A build
// constant (-DTRACE_PAIRS=n) for A/B runs: 16 / 32 / 64 / 128 measured 0.088 / 0.085 / 0.070 / 0.098 ms on
// scripts/trace_time.py's inputs
#ifndef TRACE_PAIRS
#define TRACE_PAIRS 64
#endif
constexpr uint32_t TRACE_PAIRS_PER_WG = TRACE_PAIRS;
constexpr uint32_t TRACE_ITEMS = 1024;          // windows a workgroup stages in LDS at a time (16 KiB; >= 32 pairs' worth)
constexpr uint32_t TRACE_CHUNK_WORDS = 4;       // chunk descriptor: core, log2 spc_lo, first and end index into perm

// qsim_kernel's table (launch_plan.h plan_qsim): a dictionary entry is a dpemu_qsim_gate as it stands
// {core, freq, env, amp, kind, err_thr, m[2][8]}; an unused entry has freq = QSIM_NO_GATE (no event's: 15 bits)
constexpr uint32_t QSIM_GATE_WORDS = 22;
constexpr uint32_t QSIM_SLOT_WORDS = 8 * QSIM_GATE_WORDS;   // DPEMU_QSIM_GATES_MAX entries of one core
constexpr uint32_t QSIM_LUT_WORDS = 2 * (512 + 256);        // {cos, sin} Q30: 512 coarse, then 256 fine
constexpr uint32_t QSIM_NO_GATE = 0xFFFFFFFFu;
constexpr uint32_t QSIM_DECAY_WORDS = 64;                  // dpemu_qsim_decay's table per core: damp[32], then deph[32]

}  // namespace dpemu
