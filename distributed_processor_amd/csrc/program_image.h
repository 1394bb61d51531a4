// program_image.h -- everything dpemu_load_programs derives from the
// assembled programs before it touches the device: the pre-decoded commands
// in both orders, the macro image of branch-free register programs and the
// facts the kernel choice reads (launch_plan.h).  Host-only and HIP-free
// (tests/program_image_test.cpp builds it with a plain C++ compiler).
#pragma once

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "uop.h"

namespace dpemu {

// what the kernel choice needs to know of the loaded programs
struct ProgramFacts {
    uint32_t n_programs = 0, n_groups = 0, C = 0;
    bool has_fproc = false, has_sync = false, straight = false, linear = false, reg_writes = false;
    bool has_macros = false;                // a macro image was built (branch-free programs with register commands)
    bool has_cmd_major = false;             // a command-major copy was built
    // register slots of the macro image (remap_macro_regs): 2 in VGPRs, else 16 (identity map)
    int macro_nr = 16;
    bool macro_addid = false;               // every ALU slot of the macro image is id0 / add
    bool macro_w3 = false;                  // the macro image has three ALU slots (uop.h MACRO_W3)
    uint32_t macro_rs = 0;                  // UOP_RS_* fields its pulse slots register-source
    uint64_t reg_map = 0xFEDCBA9876543210ull, reg_inv = 0xFEDCBA9876543210ull;
    uint32_t reg_used = 0xFFFFu;
    uint32_t max_len = 0;                   // longest program (commands)
    std::vector<uint64_t> group_len;        // instructions of all C programs of each group, guards included
};

struct ProgramImage {
    std::string err;                        // not empty: the program set is refused (a size limit), nothing else is valid
    ProgramFacts facts;
    std::vector<uint32_t> uops, goff;       // decode_cmd words, program-major, and each program's offset (commands)
    std::vector<uint32_t> uops_t;           // command-major copy, or empty
    std::vector<uint32_t> macro, moff;      // macro image (8 u32 per macro) and its per-program offsets, or empty
    std::vector<uint32_t> mchunk, mcoff;    // lean chunks (mark_lean_chunks) and their per-program offsets
};

inline bool is_alu_cmd(const uint32_t *c) { const uint32_t op4 = c[1] >> 28; return op4 == 0x1 || op4 == 0x6; }
// done / 0000 / hang: a branch-free program's last command
inline bool is_terminal_cmd(const uint32_t *c) { const uint32_t op4 = c[1] >> 28; return op4 == 0x0 || op4 == 0xA || op4 >= 0xD; }

// ALU slot ctl of a reg_alu / inc_qclk command: present[31] inc_qclk[30]
// rs0[15:12] rd[11:8] rs1[7:4] in0_reg[3] op[2:0]
inline uint32_t alu_ctl(const uint32_t *c)
{
    return 0x80000000u | ((c[1] >> 28) == 0x6 ? 0x40000000u : 0u) | (c[1] & 0xFFFu) | (((c[3] >> 20) & 15u) << 12);
}

// The reg_file registers a macro slot names -- the one statement of the rule.
// ALU slot ctl: rs0 when in0_reg, rd and rs1 of reg_alu; an operand the ALU
// op ignores -- in1 of id0 / zero, in0 of id1 / zero -- names nothing, nor do
// inc_qclk's rd / rs1.  Pulse slot (any other command's w): rs0 when a field
// is register-sourced.
inline uint32_t alu_slot_regs(uint32_t ctl)
{
    if (!(ctl >> 31)) return 0u;
    uint32_t used = 0;
    const uint32_t op = ctl & 7u;                       // alu.v: 0 id0, 6 id1, 7 zero
    if ((ctl & 8u) && op != 6u && op != 7u) used |= 1u << ((ctl >> 12) & 15u);
    if (!((ctl >> 30) & 1u)) {
        used |= 1u << ((ctl >> 8) & 15u);
        if (op != 0u && op != 7u) used |= 1u << ((ctl >> 4) & 15u);
    }
    return used;
}
inline uint32_t pulse_slot_regs(uint32_t w) { return (!(w >> 31) && (w & UOP_ANY_RS)) ? 1u << ((w >> 20) & 15u) : 0u; }

// Registers the macro image of program u[0, n) will name: the rule over the
// commands build_macros consumes, each program up to and including its first
// terminal command (the zero = DONE guard past the end is one)
inline uint32_t named_regs(const uint32_t *u, uint32_t n)
{
    uint32_t used = 0;
    for (uint32_t k = 0; k < n; k++) {
        const uint32_t *c = u + 4ull * k;
        used |= is_alu_cmd(c) ? alu_slot_regs(alu_ctl(c)) : pulse_slot_regs(c[3]);
        if (is_terminal_cmd(c)) break;
    }
    return used;
}

// Macro image of a branch-free program (macro.hip): from its decoded
// commands u[0, n) (and the zero = DONE guard past the end), macros of up to
// `max_alu` consecutive reg_alu / inc_qclk commands followed by the next other
// command, until the first terminal command (done / 0000 / hang) -- the
// program's last macro, which the kernel re-reads once a lane has finished.
// Built WIDE, MACRO_WIDE u32 per macro: {imm, ctl} x 3 ALU slots (alu_ctl)
// then the pulse slot's decode_cmd word (w bit 31 = no command).
// pack_macros turns it into the 32-B device image (uop.h MACRO_W3).
constexpr uint32_t MACRO_WIDE = 10;
inline void build_macros(const uint32_t *u, uint32_t n, uint32_t max_alu, std::vector<uint32_t> &out)
{
    static const uint32_t zero[4] = {0, 0, 0, 0};
    uint32_t k = 0;
    for (;;) {
        uint32_t m[MACRO_WIDE] = {0, 0, 0, 0, 0, 0, 0, 0, 0, MACRO_ABSENT};
        const uint32_t *c = k < n ? u + 4ull * k : zero;
        for (uint32_t a = 0; a < max_alu; a++) {
            if (!is_alu_cmd(c)) break;
            m[2 * a] = c[0];
            m[2 * a + 1] = alu_ctl(c);
            k++;
            c = k < n ? u + 4ull * k : zero;
        }
        const bool slot = !is_alu_cmd(c);      // the slot's command (else: another ALU command opens the next macro)
        if (slot) {
            memcpy(m + 6, c, 16);
            k++;
        }
        out.insert(out.end(), m, m + MACRO_WIDE);
        if (slot && is_terminal_cmd(c)) return;
    }
}

// ALU slot k's ctl of a packed macro (8 u32, macro.hip): legacy {imm0, ctl0,
// imm1, ctl1, pulse}, or MACRO_W3 {imm0, packed ctl, imm1, imm2, pulse}
inline uint32_t macro_ctl(const uint32_t *m, int k, bool w3)
{
    if (!w3) return k < 2 ? m[2 * k + 1] : 0u;
    return w3_ctl(m[1], k);
}

// The 32-B device image from the wide one: MACRO_W3 packs three ALU slots
// (their ctl fields with 1-bit register slots, uop.h w3_pack) when the
// image names at most 2 registers; else two slots, legacy layout.
inline void pack_macros(const std::vector<uint32_t> &wide, bool w3, std::vector<uint32_t> &mac)
{
    const size_t n = wide.size() / MACRO_WIDE;
    mac.resize(8 * n);
    for (size_t i = 0; i < n; i++) {
        const uint32_t *w = &wide[MACRO_WIDE * i];
        uint32_t *m = &mac[8 * i];
        if (w3) {
            uint32_t pk = 0;
            for (int k = 0; k < 3; k++) pk |= w3_pack(w[2 * k + 1]) << (10 * k);
            m[0] = w[0]; m[1] = pk; m[2] = w[2]; m[3] = w[4];
        } else {
            m[0] = w[0]; m[1] = w[1]; m[2] = w[2]; m[3] = w[3];
        }
        memcpy(m + 4, w + 6, 16);
    }
}

// The registers `used` the image names (named_regs over its programs)
// renumbered to slots 0..n-1 in place when there are at most 2, so
// macro_staged_kernel keeps them in VGPRs.  Unnamed registers are never
// written and read as 0 (reg_file.v resets to 0); a field that names no
// register maps to slot 0 (its value is selected away).  Returns the slot
// count (2, or 16 = left as is) and the maps (KParams::reg_map / reg_inv).
inline int remap_macro_regs(std::vector<uint32_t> &mac, uint64_t &map, uint64_t &inv, uint32_t &used)
{
    if (__builtin_popcount(used) > 2) {
        map = inv = 0xFEDCBA9876543210ull;
        used = 0xFFFFu;
        return 16;
    }
    uint32_t slot[16] = {0};
    map = inv = 0;
    for (uint32_t r = 0, k = 0; r < 16; r++)
        if ((used >> r) & 1u) { slot[r] = k; map |= (uint64_t)k << (4 * r); inv |= (uint64_t)r << (4 * k); k++; }
    auto re = [&](uint32_t v, int sh) { return (v & ~(15u << sh)) | (slot[(v >> sh) & 15u] << sh); };
    for (size_t i = 0; i < mac.size(); i += MACRO_WIDE) {
        for (int a = 0; a < 3; a++) {
            uint32_t &ctl = mac[i + 2 * a + 1];
            if (ctl >> 31) ctl = re(re(re(ctl, 12), 8), 4);
        }
        uint32_t &w = mac[i + 9];
        if (!(w >> 31) && (w & UOP_ANY_RS)) w = re(w, 20);
    }
    return 2;
}

// Mark every macro of the lean-path shape (MACRO_SIMPLE, uop.h) in the
// image's pulse slots, and return whether every ALU slot is reg_alu id0 / add
// (alu.v ops 0 / 1) and which pulse fields are register-sourced
inline bool mark_simple_macros(std::vector<uint32_t> &mac, const std::vector<uint32_t> &moff, bool w3, uint32_t &rs)
{
    bool addid = true;
    rs = 0;
    size_t prog = 0;
    for (size_t m = 0, i = 0; i < mac.size(); i += 8, m++) {
        while (prog + 1 < moff.size() && moff[prog + 1] <= m) prog++;
        const bool first = moff[prog] == m;
        bool simple = !first;
        for (int a = 0; a < 3; a++) {
            const uint32_t ctl = macro_ctl(&mac[i], a, w3);
            if (!(ctl >> 31)) continue;
            if ((ctl >> 30) & 1u) simple = false;               // inc_qclk
            if ((ctl & 7u) > 1u) addid = false;
        }
        uint32_t &w = mac[i + 7];
        if (!(w >> 31)) {
            if ((mac[i + 5] >> 28) != 0x9u) simple = false;    // not PULSE_WRITE_TRIG
            rs |= w & (UOP_RS_ENV | UOP_RS_PH | UOP_RS_FR | UOP_RS_AMP);
        }
        if (simple) w |= MACRO_SIMPLE;
    }
    return addid;
}

// Per (program, chunk of MACRO_CHUNK macros as macro_staged_kernel stages
// them: macros [c CH, (c + 1) CH) of the program, the terminal macro
// repeating past its end): the largest pulse-slot cmd_time when every macro
// of the chunk is MACRO_SIMPLE and none is the terminal one (0 when no slot
// holds a pulse), else MACRO_CHUNK_MIXED.  A wave whose running lanes all
// hold such a chunk and can reach no max_cycles stop before its end runs the
// chunk's macros with no per-macro test (macro.hip lean_chunk_ok).
// chunk_off[p]: program p's first entry.
inline void mark_lean_chunks(const std::vector<uint32_t> &mac, const std::vector<uint32_t> &moff,
                             std::vector<uint32_t> &chunk, std::vector<uint32_t> &chunk_off)
{
    const size_t n_prog = moff.size() - 1;
    chunk_off.resize(n_prog);
    chunk.clear();
    for (size_t pr = 0; pr < n_prog; pr++) {
        chunk_off[pr] = (uint32_t)chunk.size();
        const uint32_t nm = moff[pr + 1] - moff[pr];              // macros, the terminal one included
        for (uint32_t c = 0; c * MACRO_CHUNK < nm; c++) {
            uint32_t v = 0;
            if ((c + 1) * MACRO_CHUNK >= nm) v = MACRO_CHUNK_MIXED;  // reaches the terminal macro
            for (uint32_t j = 0; j < MACRO_CHUNK && v != MACRO_CHUNK_MIXED; j++) {
                const uint32_t *m = &mac[8ull * (moff[pr] + c * MACRO_CHUNK + j)];
                if (!(m[7] & MACRO_SIMPLE)) v = MACRO_CHUNK_MIXED;
                else if (!(m[7] >> 31)) v = std::max(v, m[4]);        // a pulse slot: its cmd_time
            }
            chunk.push_back(v);
        }
    }
}

// The image of a checked program set (dpemu_load_programs: every program
// within its 2^16 commands and inside `words`, every prog_table entry a
// program): n_programs programs of n_instr[i] 128-bit commands at
// words + 4 offsets[i], n_groups x C table entries.
inline ProgramImage build_program_image(const uint32_t *words, const uint32_t *offsets, const uint32_t *n_instr,
                                        uint32_t n_programs, const uint32_t *prog_table, uint32_t n_groups, uint32_t C)
{
    ProgramImage im;
    ProgramFacts &f = im.facts;
    f.n_programs = n_programs; f.n_groups = n_groups; f.C = C;
    f.straight = f.linear = true;
    for (uint32_t i = 0; i < n_programs; i++)
        for (uint32_t k = 0; k < n_instr[i]; k++) {
            const uint32_t op4 = words[4 * ((uint64_t)offsets[i] + k) + 3] >> 28;
            f.has_fproc |= (op4 == 4 || op4 == 5);
            f.has_sync |= (op4 == 7);
            f.reg_writes |= (op4 == 1 || op4 == 4);            // reg_alu / alu_fproc write the reg_file
            f.straight &= !(op4 >= 1 && op4 <= 7);
            f.linear &= !(op4 >= 2 && op4 <= 5) && op4 != 7;   // no jump / fproc / sync: ip advances by 1
        }
    // every command pre-decoded once (uop.h decode_cmd), program-major with
    // a zero (DONE) guard command after every program ...
    im.goff.resize(n_programs);
    uint64_t tot = 0;
    for (uint32_t i = 0; i < n_programs; i++) { im.goff[i] = (uint32_t)tot; tot += (uint64_t)n_instr[i] + 1; }
    if (tot >= (1ull << 32)) { im.err = "program set exceeds 2^32 commands"; return im; }
    im.uops.assign(tot * 4, 0u);
    for (uint32_t i = 0; i < n_programs; i++)
        for (uint32_t k = 0; k < n_instr[i]; k++)
            decode_cmd(words + 4 * ((uint64_t)offsets[i] + k), &im.uops[4 * ((uint64_t)im.goff[i] + k)]);
    for (uint32_t i = 0; i < n_programs; i++) f.max_len = std::max(f.max_len, n_instr[i]);
    // ... the macro image of branch-free programs with register commands
    if (f.linear && !f.straight && f.max_len < 65536u) {
        // three ALU slots per macro when the image names at most 2 registers
        // (MACRO_W3: RB-like programs then have almost no macro without a
        // pulse, so a wave's programs stay on the same event slot and its
        // stores are whole rows), else two.  The register
        // count decides the layout before the image is built
        uint32_t used = 0;
        for (uint32_t pr = 0; pr < n_programs; pr++) used |= named_regs(&im.uops[4ull * im.goff[pr]], n_instr[pr]);
        const bool w3 = __builtin_popcount(used) <= 2;
        std::vector<uint32_t> wide;
        im.moff.resize(n_programs + 1);
        wide.reserve((tot * 4 + 8ull * n_programs) / 8 * MACRO_WIDE);
        for (uint32_t pr = 0; pr < n_programs; pr++) {
            im.moff[pr] = (uint32_t)(wide.size() / MACRO_WIDE);
            build_macros(&im.uops[4ull * im.goff[pr]], n_instr[pr], w3 ? 3u : 2u, wide);
            if (wide.size() / MACRO_WIDE >= (1ull << 32)) { im.err = "macro image exceeds 2^32 macros"; return im; }
        }
        im.moff[n_programs] = (uint32_t)(wide.size() / MACRO_WIDE);
        f.reg_used = used;
        f.macro_nr = remap_macro_regs(wide, f.reg_map, f.reg_inv, f.reg_used);
        f.macro_w3 = w3;                    // == (macro_nr == 2): both follow from `used`
        pack_macros(wide, w3, im.macro);
        std::vector<uint32_t>().swap(wide);
        f.macro_addid = mark_simple_macros(im.macro, im.moff, w3, f.macro_rs);
        mark_lean_chunks(im.macro, im.moff, im.mchunk, im.mcoff);
        f.has_macros = true;
    }
    // ... and command-major (zero = DONE past a program's end, and one zero row
    // past the longest program for straight.hip) when the padding stays small:
    // at most 4x the programs, 1 GiB
    const uint64_t t_cmds = ((uint64_t)f.max_len + 1) * n_programs;
    if (f.max_len && t_cmds <= std::max<uint64_t>(4 * tot, 4096) && t_cmds * 16 <= (1ull << 30)) {
        im.uops_t.assign(t_cmds * 4, 0u);
        for (uint32_t pr = 0; pr < n_programs; pr++)
            for (uint32_t k = 0; k < n_instr[pr]; k++)
                memcpy(&im.uops_t[4 * ((uint64_t)k * n_programs + pr)], &im.uops[4 * ((uint64_t)im.goff[pr] + k)], 16);
        f.has_cmd_major = true;
    }
    f.group_len.assign(n_groups, 0);
    for (uint32_t g = 0; g < n_groups; g++)
        for (uint32_t c = 0; c < C; c++) f.group_len[g] += n_instr[prog_table[(uint64_t)g * C + c]] + 1;   // + guard
    return im;
}

}  // namespace dpemu
