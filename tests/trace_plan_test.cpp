// CPU driver of dpemu_feedline_traces' grid (csrc/launch_plan.h plan_traces),
// built and run by tests/test_trace_plan.py with g++: the sort of the pair
// table by feedline_trace_kernel's key, the cut into chunks of one (core,
// spc_lo) group each, the growth of a chunk once the grid would exceed what the
// device holds at once, and the sample tiles -- on hand-written and random
// columns.  Without arguments it prints "ok <checks>" and returns 0, or the
// first failed check.  With a file (n_pairs n_samples_lo ro_cpw n_bins
// bin_clocks S wgs_per_cu n_cu, then the core and the spc_lo column) it checks
// that table too and prints the plan: "const BLOCK TRACE_ITEMS
// TRACE_PAIRS_PER_WG", "tiles", one "chunk core log2_spc first end" per chunk
// and "perm ...".
#include <algorithm>
#include <cstdio>
#include <vector>

#include "../distributed_processor_amd/csrc/launch_plan.h"

using namespace dpemu;

static int n_checks = 0;
#define CHECK(cond)                                                        \
    do {                                                                   \
        n_checks++;                                                        \
        if (!(cond)) { std::printf("line %d: %s\n", __LINE__, #cond); return 1; } \
    } while (0)

struct Table {
    std::vector<uint32_t> core, spc;
    uint32_t n_lo = 1204, ro_cpw = 4, n_bins = 300, bin_clocks = 1, S = 1, wgs_per_cu = 8, n_cu = 256;
};

static uint32_t log2_of(uint32_t v)
{
    uint32_t l = 0;
    while ((1u << l) < v) l++;
    return l;
}

static uint32_t key_of(const Table &t, uint32_t i) { return (t.core[i] << 8) | log2_of(t.spc[i]); }

// the expected tiles and pairs per chunk, restated from the header comment of plan_traces
static uint32_t want_tiles(const Table &t)
{
    uint64_t max_spc = 1;
    for (uint32_t v : t.spc) max_spc = std::max<uint64_t>(max_spc, v);
    const uint64_t span = std::min<uint64_t>({(uint64_t)t.n_bins * t.bin_clocks * max_spc, 4096ull * t.ro_cpw * max_spc,
                                              (uint64_t)t.n_lo});
    const uint64_t steps = (span + 4ull * BLOCK - 1) / (4ull * BLOCK);      // 1,024 samples each
    return (uint32_t)std::max<uint64_t>(1, steps);
}

static uint32_t want_per(const Table &t)
{
    const uint64_t n = t.core.size();
    const uint64_t fits = (uint64_t)t.wgs_per_cu * t.n_cu / ((uint64_t)want_tiles(t) * t.S);   // chunks resident at once
    if (fits * TRACE_PAIRS_PER_WG >= n) return TRACE_PAIRS_PER_WG;          // (fits >= n / 64: no growth)
    const uint64_t resident = std::max<uint64_t>(1, fits);
    return (uint32_t)std::max<uint64_t>(TRACE_PAIRS_PER_WG, (n + resident - 1) / resident);   // (fits 0, n < 64)
}

static int check_plan(const Table &t, TracePlan *out = nullptr)
{
    const uint32_t n = (uint32_t)t.core.size();
    const TracePlan pl = plan_traces(t.core.data(), t.spc.data(), n, t.n_lo, t.ro_cpw, t.n_bins, t.bin_clocks, t.S,
                                     t.wgs_per_cu, t.n_cu);
    if (out) *out = pl;
    CHECK(pl.tab.size() == (size_t)pl.n_chunks * TRACE_CHUNK_WORDS + n);
    CHECK(pl.tiles == want_tiles(t));
    // perm: a permutation, sorted by the kernel's key
    const uint32_t *perm = pl.tab.data() + (size_t)pl.n_chunks * TRACE_CHUNK_WORDS;
    std::vector<uint32_t> seen(n, 0);
    for (uint32_t k = 0; k < n; k++) {
        CHECK(perm[k] < n);
        seen[perm[k]]++;
        CHECK(k == 0 || key_of(t, perm[k - 1]) <= key_of(t, perm[k]));
    }
    for (uint32_t i = 0; i < n; i++) CHECK(seen[i] == 1);
    // the chunks: consecutive, none empty, none across two groups, `per` pairs each but a group's last
    const uint32_t per = want_per(t);
    CHECK(per >= TRACE_PAIRS_PER_WG);
    CHECK((n == 0) == (pl.n_chunks == 0));
    uint32_t at = 0;
    for (uint32_t c = 0; c < pl.n_chunks; c++) {
        const uint32_t *d = &pl.tab[(size_t)c * TRACE_CHUNK_WORDS];
        CHECK(d[2] == at && d[3] > d[2] && d[3] <= n);
        for (uint32_t k = d[2]; k < d[3]; k++) CHECK(t.core[perm[k]] == d[0] && log2_of(t.spc[perm[k]]) == d[1]);
        const bool group_goes_on = d[3] < n && key_of(t, perm[d[3]]) == key_of(t, perm[d[2]]);
        if (group_goes_on) CHECK(d[3] - d[2] == per);
        else CHECK(d[3] - d[2] <= per);
        // a chunk starts a group or follows a full chunk of its group: the group is cut from its own start
        if (d[2] > 0 && key_of(t, perm[d[2] - 1]) == key_of(t, perm[d[2]])) CHECK(d[2] - d[-2] == per);
        at = d[3];
    }
    CHECK(at == n);
    return 0;
}

static uint32_t rnd(uint64_t &s)
{
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(s >> 33);
}

static int print_plan(const char *path)
{
    FILE *f = std::fopen(path, "r");
    if (!f) { std::printf("cannot open %s\n", path); return 1; }
    Table t;
    unsigned n = 0;
    if (std::fscanf(f, "%u %u %u %u %u %u %u %u", &n, &t.n_lo, &t.ro_cpw, &t.n_bins, &t.bin_clocks, &t.S, &t.wgs_per_cu,
                    &t.n_cu) != 8) { std::printf("bad header\n"); return 1; }
    t.core.resize(n);
    t.spc.resize(n);
    for (auto *col : {&t.core, &t.spc})
        for (unsigned i = 0; i < n; i++)
            if (std::fscanf(f, "%u", &(*col)[i]) != 1) { std::printf("short column\n"); return 1; }
    std::fclose(f);
    TracePlan pl;
    if (check_plan(t, &pl)) return 1;
    std::printf("const %u %u %u\ntiles %u\n", BLOCK, TRACE_ITEMS, TRACE_PAIRS_PER_WG, pl.tiles);
    for (uint32_t c = 0; c < pl.n_chunks; c++) {
        const uint32_t *d = &pl.tab[(size_t)c * TRACE_CHUNK_WORDS];
        std::printf("chunk %u %u %u %u\n", d[0], d[1], d[2], d[3]);
    }
    std::printf("perm");
    for (size_t k = (size_t)pl.n_chunks * TRACE_CHUNK_WORDS; k < pl.tab.size(); k++) std::printf(" %u", pl.tab[k]);
    std::printf("\n");
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 1) return print_plan(argv[1]);
    TracePlan pl;

    // ---- a hand-written table: cores interleaved, two spc_lo in core 1 ----
    {
        Table t;
        t.core = {3, 1, 0, 1, 3, 1, 0, 1};
        t.spc = {4, 4, 1, 1, 4, 4, 1, 1};
        if (check_plan(t, &pl)) return 1;
        const uint32_t want[] = {0, 0, 0, 2, /**/ 1, 0, 2, 4, /**/ 1, 2, 4, 6, /**/ 3, 2, 6, 8, /* perm */ 2, 6, 3, 7, 1, 5, 0, 4};
        CHECK(pl.n_chunks == 4 && pl.tab == std::vector<uint32_t>(want, want + 24));
        CHECK(pl.tiles == 2);                               // 300 bins x 4 samples = 1,200 samples: two steps of 1,024
    }
    // ---- groups around the chunk size: 63, 64, 65, 128, 129 pairs, and the four groups of the hand-built case ----
    for (const std::vector<uint32_t> &sizes : {std::vector<uint32_t>{63, 64, 65, 128, 129}, std::vector<uint32_t>{33, 5, 72, 32}}) {
        Table t;
        uint64_t s = 7;
        std::vector<uint32_t> left = sizes;
        for (bool any = true; any;) {                       // dealt at random: the sort has work to do
            any = false;
            const uint32_t g = rnd(s) % (uint32_t)left.size();
            if (left[g]) { left[g]--; t.core.push_back(g); t.spc.push_back(4); }
            for (uint32_t v : left) any = any || v;
        }
        if (check_plan(t, &pl)) return 1;
        uint32_t want_chunks = 0;
        for (uint32_t v : sizes) want_chunks += (v + 63) / 64;
        CHECK(pl.n_chunks == want_chunks);
        std::vector<uint32_t> got;
        for (uint32_t c = 0; c < pl.n_chunks; c++) got.push_back(pl.tab[4 * c + 3] - pl.tab[4 * c + 2]);
        if (sizes.size() == 5) CHECK(got == (std::vector<uint32_t>{63, 64, 64, 1, 64, 64, 64, 64, 1}));
        else CHECK(got == (std::vector<uint32_t>{33, 5, 64, 8, 32}));
    }
    // ---- per: 6,400 pairs of one group; 64 until the device holds fewer than 100 chunks, then ceil(n / resident) ----
    {
        Table t;
        t.core.assign(6400, 5);
        t.spc.assign(6400, 1);
        t.n_bins = 100;                                     // one tile
        struct { uint32_t S, wgs, n_cu, per; } rows[] = {
            {1, 2, 256, 64},        // 512 resident
            {32, 2, 256, 400},      // 16 resident
            {1, 1, 100, 64},        // 100 = 6,400 / 64: the last grid that is not grown
            {1, 1, 99, 65},
            {32, 25, 128, 64},      // 100 again, by S
            {32, 25, 127, 65},      // 99
            {32, 1, 31, 6400},      // less than one: a chunk per group
            {1, 0, 256, 6400},      // occupancy unknown
        };
        for (const auto &r : rows) {
            t.S = r.S; t.wgs_per_cu = r.wgs; t.n_cu = r.n_cu;
            CHECK(want_per(t) == r.per);
            if (check_plan(t, &pl)) return 1;
            CHECK(pl.tiles == 1 && pl.n_chunks == (6400 + r.per - 1) / r.per && pl.tab[3] == r.per);
        }
        t.n_bins = 4096; t.bin_clocks = 10; t.ro_cpw = 8; t.n_lo = 40000;   // 32 tiles divide the device as well
        t.S = 1; t.wgs_per_cu = 8; t.n_cu = 256;            // 2,048 / 32 = 64 resident: per = 6,400 / 64 = 100
        if (check_plan(t, &pl)) return 1;
        CHECK(pl.tiles == 32 && pl.tab[3] == 100);
    }
    // ---- tiles: each of the three bounds in turn, in steps of 1,024 samples; 1 for an empty span ----
    {
        Table t;
        t.core = {0, 1};
        t.spc = {4, 16};
        struct { uint32_t n_bins, bin_clocks, ro_cpw, n_lo, tiles; } rows[] = {
            {64, 1, 4, 1u << 20, 1},            // 64 x 16 = 1,024 samples of the bins
            {65, 1, 4, 1u << 20, 2},
            {4096, 100, 1, 1u << 20, 64},       // the longest window: 4,096 x 1 x 16 samples
            {4096, 100, 8, 1u << 20, 512},
            {4096, 100, 8, 1024, 1},            // the rows
            {4096, 100, 8, 1028, 2},
            {4096, 100, 8, 0, 1},               // no samples at all
        };
        for (const auto &r : rows) {
            t.n_bins = r.n_bins; t.bin_clocks = r.bin_clocks; t.ro_cpw = r.ro_cpw; t.n_lo = r.n_lo;
            if (check_plan(t, &pl)) return 1;
            CHECK(pl.tiles == r.tiles);
        }
        t.spc = {1, 1};                         // max_spc 1: 65 bins are one tile again
        t.n_bins = 65; t.bin_clocks = 1; t.ro_cpw = 4; t.n_lo = 1u << 20;
        if (check_plan(t, &pl)) return 1;
        CHECK(pl.tiles == 1);
    }
    // ---- no pairs ----
    {
        Table t;
        if (check_plan(t, &pl)) return 1;
        CHECK(pl.n_chunks == 0 && pl.tab.empty() && pl.tiles == 1);
    }
    // ---- random tables: up to 64 cores, five spc_lo, every grid shape ----
    uint64_t s = 12345;
    for (int round = 0; round < 300; round++) {
        Table t;
        const uint32_t n = rnd(s) % (round % 3 ? 700 : 6000), n_cores = 1 + rnd(s) % 64, n_spc = 1 + rnd(s) % 5;
        for (uint32_t i = 0; i < n; i++) {
            t.core.push_back(rnd(s) % n_cores);
            t.spc.push_back(1u << (rnd(s) % n_spc));
        }
        t.n_lo = 4 * (rnd(s) % 20000);
        t.ro_cpw = 1 + rnd(s) % 8;
        t.n_bins = 1 + rnd(s) % 4096;
        t.bin_clocks = 1 + rnd(s) % 5;
        t.S = round % 2 ? 32 : 1;
        t.wgs_per_cu = rnd(s) % 9;
        t.n_cu = 1 + rnd(s) % 256;
        if (check_plan(t)) { std::printf("random round %d\n", round); return 1; }
    }
    std::printf("ok %d\n", n_checks);
    return 0;
}
