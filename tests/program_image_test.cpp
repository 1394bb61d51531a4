// CPU test of the load-time program image (csrc/program_image.h), built and
// run by tests/test_program_image.py with g++.  Reads program sets from the
// file named by argv[1] (u32 little-endian: n_cases, then per case C,
// n_groups, n_programs, n_cmds, offsets[], n_instr[], prog_table[], words[])
// and checks every image against the definitions, restated here from the
// comments in uop.h / program_image.h rather than by calling the builder's
// own helpers.  Prints one line of facts per case, then OK.
#include <cstdio>
#include <vector>

#include "../distributed_processor_amd/csrc/program_image.h"

using namespace dpemu;

static int failures = 0;
static int cur_case = -1;
#define CHECK(c)                                                                                   \
    do {                                                                                           \
        if (!(c)) {                                                                                \
            if (failures < 20) std::printf("FAIL case %d %s:%d %s\n", cur_case, __FILE__, __LINE__, #c); \
            failures++;                                                                            \
        }                                                                                          \
    } while (0)

static bool is_alu(uint32_t op4) { return op4 == 0x1 || op4 == 0x6; }
static bool is_terminal(uint32_t op4) { return op4 == 0x0 || op4 == 0xA || op4 >= 0xD; }

// an ALU slot against the decoded reg_alu / inc_qclk command it came from: the immediate, the
// opcode, op and in0_reg, and the register fields the command names, through reg_inv
static void check_alu_slot(uint32_t imm, uint32_t ctl, const uint32_t *u, uint64_t inv)
{
    const uint32_t op4 = u[1] >> 28, op = u[1] & 7u;
    auto reg = [&](int sh) { return (uint32_t)(inv >> (4 * ((ctl >> sh) & 15u))) & 15u; };
    CHECK(ctl >> 31);
    CHECK(imm == u[0]);
    CHECK(((ctl >> 30) & 1u) == (op4 == 0x6 ? 1u : 0u));
    CHECK((ctl & 15u) == (u[1] & 15u));
    const bool reads_in0 = op != 6 && op != 7, reads_in1 = op != 0 && op != 7;   // alu.v: 0 id0, 6 id1, 7 zero
    if ((u[1] & 8u) && reads_in0) CHECK(reg(12) == ((u[3] >> 20) & 15u));
    if (op4 == 0x1) {
        CHECK(reg(8) == ((u[1] >> 8) & 15u));
        if (reads_in1) CHECK(reg(4) == ((u[1] >> 4) & 15u));
    }
}

static void check_case(const uint32_t *&in)
{
    const uint32_t C = *in++, n_groups = *in++, n_programs = *in++, n_cmds = *in++;
    const uint32_t *offsets = in, *n_instr = in + n_programs, *table = in + 2 * n_programs;
    const uint32_t *words = table + (size_t)n_groups * C;
    in = words + 4ull * n_cmds;
    const ProgramImage im = build_program_image(words, offsets, n_instr, n_programs, table, n_groups, C);
    const ProgramFacts &f = im.facts;
    CHECK(im.err.empty());
    if (!im.err.empty()) return;

    // program-major: decode_cmd of every command, a zero guard after each program
    uint64_t tot = 0;
    uint32_t max_len = 0;
    for (uint32_t p = 0; p < n_programs; p++) {
        CHECK(im.goff[p] == tot);
        for (uint32_t k = 0; k <= n_instr[p]; k++) {
            uint32_t u[4] = {0, 0, 0, 0};
            if (k < n_instr[p]) decode_cmd(words + 4 * ((uint64_t)offsets[p] + k), u);
            CHECK(!memcmp(u, &im.uops[4 * (tot + k)], 16));
        }
        tot += n_instr[p] + 1;
        max_len = std::max(max_len, n_instr[p]);
    }
    CHECK(im.uops.size() == 4 * tot);
    CHECK(f.max_len == max_len);
    CHECK(f.group_len.size() == n_groups);
    for (uint32_t g = 0; g < n_groups; g++) {
        uint64_t len = 0;
        for (uint32_t c = 0; c < C; c++) len += n_instr[table[(size_t)g * C + c]] + 1;
        CHECK(f.group_len[g] == len);
    }

    // command-major: the transpose, zero rows past each program's end (and the guard row)
    CHECK(f.has_cmd_major == !im.uops_t.empty());
    if (f.has_cmd_major) {
        CHECK(im.uops_t.size() == 4ull * (max_len + 1) * n_programs);
        for (uint32_t k = 0; k <= max_len; k++)
            for (uint32_t p = 0; p < n_programs; p++) {
                static const uint32_t zero[4] = {0, 0, 0, 0};
                const uint32_t *want = k < n_instr[p] ? &im.uops[4 * ((uint64_t)im.goff[p] + k)] : zero;
                CHECK(!memcmp(want, &im.uops_t[4 * ((uint64_t)k * n_programs + p)], 16));
            }
    }

    // the macro image
    CHECK(f.has_macros == !im.macro.empty());
    CHECK(f.macro_w3 == (f.macro_nr == 2));
    size_t n_simple = 0;
    // of the MACRO_SIMPLE macros (the shape the lean and simple paths of macro.hip retire): those with the
    // third ALU slot, those with no pulse slot, the ALU ops they hold (a mask), their ALU slots with the
    // register form of in0, all their ALU slots; per program the macros and the chunks that are not MIXED
    size_t n_third = 0, n_absent = 0, n_in0reg = 0, n_alu_simple = 0;
    uint32_t ops_simple = 0, nm_min = ~0u, nm_max = 0, lean_min = ~0u;
    if (f.has_macros) {
        const bool w3 = f.macro_w3;
        const size_t n_macros = im.macro.size() / 8;
        CHECK(im.moff.size() == n_programs + 1 && im.moff[0] == 0 && im.moff[n_programs] == n_macros);
        CHECK(im.mcoff.size() == n_programs);
        bool addid = true;
        uint32_t rs = 0;
        size_t chunk_at = 0;
        for (uint32_t p = 0; p < n_programs; p++) {
            CHECK(im.moff[p] < im.moff[p + 1]);
            const uint32_t *u = &im.uops[4ull * im.goff[p]];     // the guard is the command at n_instr[p]
            uint32_t k = 0;                                        // next decoded command to be matched
            bool ended = false;
            const uint32_t nm = im.moff[p + 1] - im.moff[p];
            std::vector<bool> simple(nm);
            for (uint32_t j = 0; j < nm; j++) {
                const uint32_t *m = &im.macro[8ull * (im.moff[p] + j)];
                CHECK(!ended);
                bool inc = false;
                // ALU slots in order: legacy {imm0, ctl0, imm1, ctl1}, W3 {imm0, packed, imm1, imm2}
                for (int a = 0; a < (w3 ? 3 : 2); a++) {
                    const uint32_t ctl = w3 ? w3_ctl(m[1], a) : m[2 * a + 1];
                    const uint32_t imm = w3 ? (a == 0 ? m[0] : m[1 + a]) : m[2 * a];
                    if (!(ctl >> 31)) continue;
                    CHECK(k <= n_instr[p] && is_alu(u[4 * k + 1] >> 28));
                    check_alu_slot(imm, ctl, u + 4 * k, f.reg_inv);
                    inc |= (ctl >> 30) & 1u;
                    if ((ctl & 7u) > 1u) addid = false;
                    k++;
                }
                // then the pulse slot: the decoded command, rs0 through reg_inv when a field is register-sourced
                const bool present = !(m[7] >> 31);
                if (present) {
                    CHECK(k <= n_instr[p]);
                    const uint32_t *c = u + 4 * k;
                    CHECK(!is_alu(c[1] >> 28));
                    CHECK(m[4] == c[0] && m[5] == c[1] && m[6] == c[2]);
                    uint32_t w = m[7] & ~MACRO_SIMPLE;
                    if (w & UOP_ANY_RS) w = (w & ~(15u << 20)) | (((uint32_t)(f.reg_inv >> (4 * ((w >> 20) & 15u))) & 15u) << 20);
                    CHECK(w == c[3]);
                    rs |= c[3] & (UOP_RS_ENV | UOP_RS_PH | UOP_RS_FR | UOP_RS_AMP);
                    ended = is_terminal(c[1] >> 28);
                    k++;
                } else {
                    CHECK(m[7] == MACRO_ABSENT || m[7] == (MACRO_ABSENT | MACRO_SIMPLE));
                }
                // MACRO_SIMPLE: not the program's first macro, no inc_qclk, a PULSE_WRITE_TRIG or no pulse slot
                simple[j] = j != 0 && !inc && (!present || (m[5] >> 28) == 0x9u);
                CHECK(((m[7] & MACRO_SIMPLE) != 0) == simple[j]);
                n_simple += simple[j];
                if (simple[j]) {
                    n_absent += !present;
                    for (int a = 0; a < (w3 ? 3 : 2); a++) {
                        const uint32_t ctl = w3 ? w3_ctl(m[1], a) : m[2 * a + 1];
                        if (!(ctl >> 31)) continue;
                        CHECK(!((ctl >> 30) & 1u));         // a simple macro holds reg_alu only
                        n_alu_simple++;
                        n_third += a == 2;
                        n_in0reg += (ctl >> 3) & 1u;
                        ops_simple |= 1u << (ctl & 7u);
                    }
                }
            }
            CHECK(ended);                       // up to and including the first terminal command, no further
            // lean chunks: MIXED when the chunk reaches the terminal macro or holds a macro
            // that is not simple, else the largest pulse cmd_time
            CHECK(im.mcoff[p] == chunk_at);
            nm_min = std::min(nm_min, nm);
            nm_max = std::max(nm_max, nm);
            uint32_t lean_p = 0;
            for (uint32_t c = 0; c * MACRO_CHUNK < nm; c++, chunk_at++) {
                uint32_t want = 0;
                if ((c + 1) * MACRO_CHUNK >= nm) want = MACRO_CHUNK_MIXED;
                for (uint32_t j = c * MACRO_CHUNK; j < (c + 1) * MACRO_CHUNK && want != MACRO_CHUNK_MIXED; j++) {
                    const uint32_t *m = &im.macro[8ull * (im.moff[p] + j)];
                    if (!simple[j]) want = MACRO_CHUNK_MIXED;
                    else if (!(m[7] >> 31)) want = std::max(want, m[4]);
                }
                CHECK(chunk_at < im.mchunk.size() && im.mchunk[chunk_at] == want);
                lean_p += want != MACRO_CHUNK_MIXED;
            }
            CHECK(lean_p + 1 <= (nm + MACRO_CHUNK - 1) / MACRO_CHUNK);     // the terminal chunk is never lean
            lean_min = std::min(lean_min, lean_p);
        }
        CHECK(chunk_at == im.mchunk.size());
        CHECK(f.macro_addid == addid);
        CHECK(f.macro_rs == rs);
        CHECK(!addid || (ops_simple & ~3u) == 0u);
        CHECK(n_third <= n_simple && n_absent <= n_simple && n_in0reg <= n_alu_simple);
        CHECK(w3 || n_third == 0);
        CHECK(nm_min >= 1 && nm_min <= nm_max && nm_max <= n_macros);
    }
    std::printf("case %d straight=%d linear=%d macros=%d cm=%d nr=%d w3=%d addid=%d used=0x%x simple=%zu lean=%zu",
                cur_case, f.straight, f.linear, f.has_macros, f.has_cmd_major, f.macro_nr, f.macro_w3, f.macro_addid,
                f.reg_used, n_simple,
                (size_t)std::count_if(im.mchunk.begin(), im.mchunk.end(), [](uint32_t v) { return v != MACRO_CHUNK_MIXED; }));
    if (f.has_macros)
        std::printf(" nm_min=%u nm_max=%u lean_min=%u rs=0x%x third=%zu absent=%zu ops=0x%x in0reg=%zu", nm_min, nm_max,
                    lean_min, f.macro_rs, n_third, n_absent, ops_simple, n_in0reg);
    std::printf("\n");
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
    const uint32_t *in = buf.data();
    const uint32_t n_cases = *in++;
    for (cur_case = 0; cur_case < (int)n_cases; cur_case++) check_case(in);
    CHECK(in == buf.data() + buf.size());
    if (failures) { std::printf("%d failure(s)\n", failures); return 1; }
    std::printf("OK\n");
    return 0;
}
