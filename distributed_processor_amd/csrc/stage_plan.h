// stage_plan.h -- the host half of every entry point but dpemu_qsim (whose
// plan_qsim is in launch_plan.h): the conditions under which include/dpemu.h
// refuses a call, and the tables the accepted call uploads -- channel and pair
// descriptors (uop.h DDS_CH_WORDS, DEMOD_PAIR_WORDS), the line table the
// feedline kernels share, the padded resonator coefficients and the explicit
// columns of dpemu_iq_stats.  A planner is a pure function of the caller's
// host structs and arrays: it returns a plan that carries the refusal (a
// return code and the dpemu_last_error text) or what capi.cpp is to upload,
// and never follows a device pointer.  Conditions are tested in the order
// they are written here; the first that holds names the refusal.  Nothing
// here touches the device (tests/stage_plan_test.cpp builds it with a plain
// C++ compiler).
#pragma once

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/dpemu.h"
#include "program_image.h"
#include "uop.h"

namespace dpemu {

struct Refusal {
    int code = DPEMU_OK;                    // DPEMU_E_INVALID or DPEMU_E_NOPROG: the call is refused ...
    std::string err;                        // ... with this dpemu_last_error text
    bool refused() const { return code != DPEMU_OK; }
};

// the plan, refused with a printf-style message
template <class Plan> __attribute__((format(printf, 3, 4))) inline Plan &refuse(Plan &pl, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    pl.code = code;
    pl.err = buf;
    return pl;
}

// ---- dpemu_run / dpemu_run_host: the config against the loaded programs ----
// have_readout_freqs: dpemu_load_readout_freqs was called for them (DEMOD runs need it)
inline Refusal check_run(const ProgramFacts &f, bool have_readout_freqs, const dpemu_config *cfg, uint64_t n_shots,
                         bool want_hist)
{
    Refusal r;
    if (!cfg) return refuse(r, DPEMU_E_INVALID, "null config");
    if (!f.n_programs) return refuse(r, DPEMU_E_NOPROG, "run before load_programs");
    if (cfg->cores_per_shot != f.C)
        return refuse(r, DPEMU_E_INVALID, "cores_per_shot %u != loaded %u", cfg->cores_per_shot, f.C);
    if (cfg->n_groups != f.n_groups)
        return refuse(r, DPEMU_E_INVALID, "n_groups %u != loaded %u", cfg->n_groups, f.n_groups);
    if (cfg->shots_per_group == 0) return refuse(r, DPEMU_E_INVALID, "shots_per_group == 0");
    if (cfg->n_groups > 0x80000000u) return refuse(r, DPEMU_E_INVALID, "n_groups > 2^31");
    if (cfg->max_cycles == 0 || cfg->max_cycles > 0x7FFFFFC0u)
        return refuse(r, DPEMU_E_INVALID, "max_cycles must be in (0, 2^31 - 64]");
    if (cfg->meas_latency < 1 || cfg->meas_latency > (1u << 20) || cfg->sync_latency < 1 ||
        cfg->sync_latency > (1u << 20))
        return refuse(r, DPEMU_E_INVALID, "meas_latency / sync_latency must be in [1, 2^20]");
    if (cfg->meas_model > DPEMU_MEAS_DEMOD)
        return refuse(r, DPEMU_E_INVALID, "meas_model must be DPEMU_MEAS_STATE, _READOUT or _DEMOD");
    if (cfg->meas_model == DPEMU_MEAS_DEMOD) {
        if (cfg->ro_drv_elem > 3 || cfg->ro_drv_elem == cfg->meas_elem)
            return refuse(r, DPEMU_E_INVALID, "ro_drv_elem %u must be an element 0..3 other than meas_elem",
                          cfg->ro_drv_elem);
        if (cfg->ro_cpw < 1 || cfg->ro_cpw > DPEMU_RO_CPW_MAX)
            return refuse(r, DPEMU_E_INVALID, "ro_cpw %u not in [1, %u]", cfg->ro_cpw, DPEMU_RO_CPW_MAX);
        if (cfg->ro_delay >= (1u << 20)) return refuse(r, DPEMU_E_INVALID, "ro_delay must be < 2^20");
        if (cfg->ro_gain[0] > 65536 || cfg->ro_gain[1] > 65536)
            return refuse(r, DPEMU_E_INVALID, "ro_gain must be <= 65536 (1.0 in Q16)");
        if (cfg->ro_sigma >= (1u << 24)) return refuse(r, DPEMU_E_INVALID, "DEMOD: ro_sigma must be < 2^24");
        if ((uint64_t)cfg->max_cycles + cfg->meas_latency + 4096ull * DPEMU_RO_CPW_MAX + 64 >= 0x80000000ull)
            return refuse(r, DPEMU_E_INVALID, "max_cycles + meas_latency + the readout window must stay below 2^31");
        if (!have_readout_freqs)
            return refuse(r, DPEMU_E_INVALID, "DEMOD run without readout frequency tables (dpemu_load_readout_freqs)");
    }
    if (cfg->hist_assign > 1) return refuse(r, DPEMU_E_INVALID, "hist_assign must be 0 or 1");
    if (cfg->lane_order > DPEMU_LANES_SHOT_MAJOR)
        return refuse(r, DPEMU_E_INVALID, "lane_order %u is not DPEMU_LANES_CORE_MAJOR / SHOT_MAJOR", cfg->lane_order);
    if (cfg->ro_win >= 4096)
        return refuse(r, DPEMU_E_INVALID, "ro_win %u must fit the 12-bit envelope-length field", cfg->ro_win);
    if ((uint64_t)cfg->max_cycles + cfg->meas_latency + 16 >= 0x80000000ull)
        return refuse(r, DPEMU_E_INVALID, "max_cycles + meas_latency must stay below 2^31");
    if (cfg->meas_cap > 32) return refuse(r, DPEMU_E_INVALID, "meas_cap > 32");
    if (cfg->event_cap > DPEMU_MAX_EVENT_CAP || cfg->trace_cap > DPEMU_MAX_EVENT_CAP)
        return refuse(r, DPEMU_E_INVALID, "event_cap / trace_cap > %u", DPEMU_MAX_EVENT_CAP);
    if (cfg->fproc_mode > 1) return refuse(r, DPEMU_E_INVALID, "fproc_mode %u", cfg->fproc_mode);
    if (cfg->lut_mask == 0) return refuse(r, DPEMU_E_INVALID, "lut_mask must be nonzero");
    if (n_shots * cfg->cores_per_shot >= 0x80000000ull)
        return refuse(r, DPEMU_E_INVALID, "n_shots * cores_per_shot must be < 2^31 per run");
    if (want_hist && cfg->cores_per_shot > 12)
        return refuse(r, DPEMU_E_INVALID, "histogram needs cores_per_shot <= 12");
    return r;
}

// ---- dpemu_dds: the channel descriptors (uop.h DDS_CH_WORDS) ----
struct ChannelPlan : Refusal {
    std::vector<uint32_t> desc;             // empty: no channels or no samples, the call has nothing to do
    // channels 2i and 2i + 1 on one lane (a qdrv / rdrv pair per core, say): one
    // index workgroup loads that lane's events once for both
    bool pair_lanes = false;
};

inline ChannelPlan plan_channels(const dpemu_dds_channels *ch)
{
    ChannelPlan pl;
    if (ch->n_samples % 4) return refuse(pl, DPEMU_E_INVALID, "n_samples must be a multiple of 4");
    if (ch->event_cap > DDS_MAX_EVENTS) return refuse(pl, DPEMU_E_INVALID, "event_cap > %u", DDS_MAX_EVENTS);
    if (ch->n_channels == 0 || ch->n_samples == 0) return pl;
    if (ch->n_channels > 65535) return refuse(pl, DPEMU_E_INVALID, "n_channels > 65535");
    pl.desc.resize((size_t)ch->n_channels * DDS_CH_WORDS);
    for (uint32_t i = 0; i < ch->n_channels; i++) {
        uint32_t *d = &pl.desc[(size_t)i * DDS_CH_WORDS];
        d[0] = ch->ch_lane[i]; d[1] = ch->ch_elem[i] & 3u; d[2] = ch->spc[i]; d[3] = ch->interp[i];
        d[4] = ch->env_off[i]; d[5] = ch->env_len[i]; d[6] = ch->freq_off[i]; d[7] = ch->freq_len[i];
        if (d[0] >= ch->n_lanes) return refuse(pl, DPEMU_E_INVALID, "channel %u: lane %u >= n_lanes", i, d[0]);
        if (d[2] < 1 || d[2] > 16) return refuse(pl, DPEMU_E_INVALID, "channel %u: spc %u not in [1, 16]", i, d[2]);
        if (d[3] < 1) return refuse(pl, DPEMU_E_INVALID, "channel %u: interp must be >= 1", i);
    }
    pl.pair_lanes = ch->n_channels % 2 == 0;
    for (uint32_t i = 0; pl.pair_lanes && i < ch->n_channels; i += 2)
        pl.pair_lanes = pl.desc[(size_t)i * DDS_CH_WORDS] == pl.desc[(size_t)(i + 1) * DDS_CH_WORDS];
    return pl;
}

// ---- the pair table of dpemu_demod_iq and of the feedline stages (uop.h DEMOD_PAIR_WORDS) ----
// In two steps, because a caller has checks of its own between them (dpemu_demod_iq: iq_lo's
// alignment; the feedline stages: the lines' pointers): check_pairs for the table's scalars and
// array pointers (need_drv: the stage reads the drive rows), then describe_pairs for the
// descriptors.  n_pairs == 0 passes check_pairs once the caps, ro_cpw and cores_per_shot are in
// range: the arrays and the row lengths are not looked at.
struct PairPlan : Refusal {
    std::vector<uint32_t> desc;
};

template <class Plan = PairPlan>
inline Plan check_pairs(const dpemu_config *cfg, const dpemu_demod_pairs *pairs, const char *what, bool need_drv)
{
    Plan pl;
    if (pairs->event_cap > DDS_MAX_EVENTS) return refuse(pl, DPEMU_E_INVALID, "event_cap > %u", DDS_MAX_EVENTS);
    if (pairs->meas_cap < 1 || pairs->meas_cap > 32)
        return refuse(pl, DPEMU_E_INVALID, "meas_cap %u not in [1, 32]", pairs->meas_cap);
    if (cfg->ro_cpw < 1 || cfg->ro_cpw > DPEMU_RO_CPW_MAX)
        return refuse(pl, DPEMU_E_INVALID, "ro_cpw %u not in [1, %u]", cfg->ro_cpw, DPEMU_RO_CPW_MAX);
    if (cfg->cores_per_shot < 1 || cfg->cores_per_shot > DPEMU_MAX_CORES)
        return refuse(pl, DPEMU_E_INVALID, "cores_per_shot %u not in [1, %u]", cfg->cores_per_shot, DPEMU_MAX_CORES);
    if (pairs->n_pairs == 0) return pl;
    if (pairs->n_pairs > 65535) return refuse(pl, DPEMU_E_INVALID, "n_pairs > 65535");
    const struct { const void *p; const char *name; } arrays[] = {
        {pairs->lane, "pairs->lane"}, {pairs->core, "pairs->core"}, {pairs->shot, "pairs->shot"},
        {pairs->drv_row, "pairs->drv_row"}, {pairs->lo_row, "pairs->lo_row"}, {pairs->spc_drv, "pairs->spc_drv"},
        {pairs->spc_lo, "pairs->spc_lo"}};
    for (const auto &a : arrays)
        if (!a.p) return refuse(pl, DPEMU_E_INVALID, "%s: %s is NULL", what, a.name);
    // the sweeps read LO-rate rows in 16-B groups (dpemu_dds rows are multiples of 4 samples)
    if (pairs->n_samples_lo == 0 || pairs->n_samples_lo % 4)
        return refuse(pl, DPEMU_E_INVALID, "n_samples_lo must be a nonzero multiple of 4");
    if (need_drv && pairs->n_samples_drv == 0) return refuse(pl, DPEMU_E_INVALID, "n_samples_drv must be nonzero");
    return pl;
}

template <class Plan> inline Plan &describe_pairs(Plan &pl, const dpemu_config *cfg, const dpemu_demod_pairs *pairs)
{
    pl.desc.assign((size_t)pairs->n_pairs * DEMOD_PAIR_WORDS, 0u);
    for (uint32_t i = 0; i < pairs->n_pairs; i++) {
        uint32_t *d = &pl.desc[(size_t)i * DEMOD_PAIR_WORDS];
        const uint32_t lane = pairs->lane[i], core = pairs->core[i];
        const uint32_t spc_drv = pairs->spc_drv[i], spc_lo = pairs->spc_lo[i];
        d[PAIR_LANE] = lane; d[PAIR_CORE] = core;
        d[PAIR_SHOT_LO] = (uint32_t)pairs->shot[i]; d[PAIR_SHOT_HI] = (uint32_t)(pairs->shot[i] >> 32);
        d[PAIR_DRV_ROW] = pairs->drv_row[i]; d[PAIR_LO_ROW] = pairs->lo_row[i];
        d[PAIR_SPC_DRV] = spc_drv; d[PAIR_SPC_LO] = spc_lo;
        if (lane >= pairs->n_lanes) return refuse(pl, DPEMU_E_INVALID, "pair %u: lane %u >= n_lanes", i, lane);
        if (core >= cfg->cores_per_shot)
            return refuse(pl, DPEMU_E_INVALID, "pair %u: core %u >= cores_per_shot", i, core);
        if (spc_lo < 1 || spc_lo > 16 || (spc_lo & (spc_lo - 1)))
            return refuse(pl, DPEMU_E_INVALID, "pair %u: spc_lo %u is not a power of two in [1, 16]", i, spc_lo);
        if (spc_drv < 1 || spc_drv > 16 || spc_drv % spc_lo)
            return refuse(pl, DPEMU_E_INVALID, "pair %u: spc_drv %u is not a multiple of spc_lo %u in [1, 16]", i, spc_drv,
                          spc_lo);
        d[PAIR_P1_THR] = cfg->p1_threshold[core];
        d[PAIR_AXIS] = cfg->ro_axis[core];
    }
    return pl;
}

// ---- the feedline stages: the pair table and the line table ----
// What the stages differ in:           drive rows read   ro_gain <= 65536   a pair in no line
//   FEEDLINE_ADC      (the ADC stage)        yes               yes               allowed
//   FEEDLINE_ADC_RES  (the resonators)       yes         no (plan_resonators)    allowed
//   FEEDLINE_DEMOD    (demodulator, traces)  no                no                refused
enum FeedlineStage { FEEDLINE_ADC, FEEDLINE_ADC_RES, FEEDLINE_DEMOD };

// tab = line_first [n_lines + 1] | member [M] | line_of [n_pairs] (~0: in no line) | wg_first [n_wgs + 1], the
// offsets of feedline_res_kernel's workgroups (res_pack_lines).  Those are appended for every
// stage -- O(n_lines) host work and n_wgs + 1 more words: the stages share one cached copy of
// the table on the device, and were the offsets appended only for the resonator stage, the
// stages would hold differently sized tables in that cache and every alternation between them
// would synchronise the stream and upload the table again.
struct FeedlinePlan : PairPlan {
    std::vector<uint32_t> tab;
    uint32_t n_pairs = 0, n_lines = 0;
    uint32_t member = 0, line_of = 0, wg_first = 0;     // where the parts after line_first begin in tab (words)
    uint32_t n_wgs = 0;
};

inline FeedlinePlan plan_feedlines(const dpemu_config *cfg, const dpemu_demod_pairs *pairs, const dpemu_feedlines *lines,
                                   const char *what, FeedlineStage stage)
{
    FeedlinePlan pl = check_pairs<FeedlinePlan>(cfg, pairs, what, stage != FEEDLINE_DEMOD);
    if (pl.refused()) return pl;
    if (lines->n_lines == 0) return refuse(pl, DPEMU_E_INVALID, "%s: n_lines is 0", what);
    if (!lines->line_first || !lines->member)
        return refuse(pl, DPEMU_E_INVALID, "%s: lines->%s is NULL", what, lines->line_first ? "member" : "line_first");
    if (describe_pairs(pl, cfg, pairs).refused()) return pl;
    const uint32_t L = pl.n_lines = lines->n_lines, n = pl.n_pairs = pairs->n_pairs;
    if (lines->line_first[0] != 0) return refuse(pl, DPEMU_E_INVALID, "line_first[0] must be 0");
    std::vector<uint32_t> &tab = pl.tab;
    tab.assign(lines->line_first, lines->line_first + L + 1);
    for (uint32_t l = 0; l < L; l++) {
        if (tab[l + 1] <= tab[l]) return refuse(pl, DPEMU_E_INVALID, "line %u is empty", l);
        if (tab[l + 1] - tab[l] > DPEMU_FEEDLINE_MAX)
            return refuse(pl, DPEMU_E_INVALID, "line %u has %u members (> %u)", l, tab[l + 1] - tab[l],
                          (unsigned)DPEMU_FEEDLINE_MAX);
    }
    const uint32_t M = tab[L];
    tab.insert(tab.end(), lines->member, lines->member + M);
    std::vector<uint32_t> line_of(n, 0xFFFFFFFFu);
    for (uint32_t l = 0; l < L; l++)
        for (uint32_t i = tab[l]; i < tab[l + 1]; i++) {
            const uint32_t m = lines->member[i], m0 = lines->member[tab[l]];
            if (m >= n) return refuse(pl, DPEMU_E_INVALID, "line %u: member %u >= n_pairs", l, m);
            if (line_of[m] != 0xFFFFFFFFu)
                return refuse(pl, DPEMU_E_INVALID, "pair %u is in two lines (%u and %u)", m, line_of[m], l);
            line_of[m] = l;
            if (pairs->spc_drv[m] != pairs->spc_drv[m0] || pairs->spc_lo[m] != pairs->spc_lo[m0])
                return refuse(pl, DPEMU_E_INVALID, "line %u: pairs %u and %u differ in spc_drv / spc_lo", l, m0, m);
        }
    if (stage == FEEDLINE_DEMOD)
        for (uint32_t i = 0; i < n; i++)
            if (line_of[i] == 0xFFFFFFFFu) return refuse(pl, DPEMU_E_INVALID, "pair %u is in no line", i);
    pl.member = L + 1;
    pl.line_of = pl.member + M;
    tab.insert(tab.end(), line_of.begin(), line_of.end());
    pl.wg_first = (uint32_t)tab.size();
    res_pack_lines(lines->line_first, L, tab);
    pl.n_wgs = (uint32_t)tab.size() - pl.wg_first - 1;
    if (stage == FEEDLINE_ADC && (cfg->ro_gain[0] > 65536u || cfg->ro_gain[1] > 65536u))
        return refuse(pl, DPEMU_E_INVALID, "ro_gain must be <= 65536");
    return pl;
}

// ---- dpemu_feedline_adc_res: the coefficients, after every check of plan_feedlines ----
// the pole inside |a| <= 1 - 2^-12 (y then stays below 2^28), the coupling's components within +-2^30
struct ResonatorPlan : Refusal {
    std::vector<int32_t> coef;              // [n_pairs][2][4], then four zero words: the kernel's gather reads its zeros there
};

inline ResonatorPlan plan_resonators(const dpemu_resonators *res, uint32_t n_pairs)
{
    ResonatorPlan pl;
    const size_t n_coef = (size_t)n_pairs * 8;
    for (size_t i = 0; i < n_coef; i += 4) {
        const int64_t a_re = res->coef[i], a_im = res->coef[i + 1], c_re = res->coef[i + 2], c_im = res->coef[i + 3];
        const int64_t lim = (1ll << 30) - (1ll << 18);
        if (a_re * a_re + a_im * a_im > lim * lim)
            return refuse(pl, DPEMU_E_INVALID, "pair %zu state %zu: pole (%lld, %lld) outside |a| <= 2^30 - 2^18", i / 8,
                          i / 4 % 2, (long long)a_re, (long long)a_im);
        if (c_re < -(1ll << 30) || c_re > (1ll << 30) || c_im < -(1ll << 30) || c_im > (1ll << 30))
            return refuse(pl, DPEMU_E_INVALID, "pair %zu state %zu: coupling (%lld, %lld) outside +-2^30", i / 8,
                          i / 4 % 2, (long long)c_re, (long long)c_im);
    }
    pl.coef.assign(res->coef, res->coef + n_coef);
    pl.coef.resize(n_coef + 4, 0);
    return pl;
}

// ---- dpemu_feedline_traces: the bins, then the demodulator's tables (plan_traces of launch_plan.h
// follows an accepted call) ----
inline FeedlinePlan plan_trace_feedlines(const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                         const dpemu_feedlines *lines, const dpemu_trace_bins *bins, const char *what)
{
    FeedlinePlan pl;
    if (bins->n_bins < 1 || bins->n_bins > DPEMU_TRACE_BINS_MAX)
        return refuse(pl, DPEMU_E_INVALID, "n_bins %u not in [1, %u]", bins->n_bins, (unsigned)DPEMU_TRACE_BINS_MAX);
    if (bins->bin_clocks < 1) return refuse(pl, DPEMU_E_INVALID, "bin_clocks must be >= 1");
    if (bins->by_slot > 1) return refuse(pl, DPEMU_E_INVALID, "by_slot %u must be 0 or 1", bins->by_slot);
    // a (class, bin) sums at most n_pairs meas_cap readouts x 16 bin_clocks samples of magnitude <= 2^31
    if ((unsigned __int128)pairs->n_pairs * pairs->meas_cap * bins->bin_clocks * 16u > (1ull << 31))
        return refuse(pl, DPEMU_E_INVALID,
                      "n_pairs * meas_cap * bin_clocks * 16 = %llu * %u exceeds 2^31 (the int64 sums' bound)",
                      (unsigned long long)pairs->n_pairs * pairs->meas_cap * 16u, bins->bin_clocks);
    return plan_feedlines(cfg, pairs, lines, what, FEEDLINE_DEMOD);
}

// ---- dpemu_iq_stats: the columns and the per-core discriminators ----
struct IqColumnsPlan : Refusal {
    bool expl = false;                      // explicit columns (cols->core / shot), else the run layout
    std::vector<uint8_t> tab;               // explicit columns: [n] u64 shots then [n] u32 cores
    uint32_t p1[DPEMU_MAX_CORES] = {}, axis[DPEMU_MAX_CORES] = {};      // IqStatsParams' arrays of the same names
    int32_t thr[DPEMU_MAX_CORES] = {};
};

inline IqColumnsPlan plan_iq_columns(const dpemu_config *cfg, const dpemu_iq_columns *cols)
{
    IqColumnsPlan pl;
    const uint32_t C = cfg->cores_per_shot, n = cols->n_cols;
    if (C == 0 || C > DPEMU_MAX_CORES || (C & (C - 1)))
        return refuse(pl, DPEMU_E_INVALID, "cores_per_shot %u is not a power of two in [1, 64]", C);
    if (cols->meas_cap < 1 || cols->meas_cap > 32)
        return refuse(pl, DPEMU_E_INVALID, "meas_cap %u not in [1, 32]", cols->meas_cap);
    if (cols->by_slot > 1) return refuse(pl, DPEMU_E_INVALID, "by_slot %u must be 0 or 1", cols->by_slot);
    if (cols->count_stride < 1) return refuse(pl, DPEMU_E_INVALID, "count_stride must be >= 1");
    if ((uint64_t)n * cols->meas_cap > (1ull << 31))
        return refuse(pl, DPEMU_E_INVALID, "n_cols * meas_cap = %llu exceeds 2^31 (the int64 sums' bound)",
                      (unsigned long long)n * cols->meas_cap);
    if ((cols->core == nullptr) != (cols->shot == nullptr))
        return refuse(pl, DPEMU_E_INVALID, "explicit columns need both core and shot (%s is NULL)",
                      cols->core ? "shot" : "core");
    pl.expl = cols->core != nullptr;
    if (!pl.expl) {
        if (cfg->lane_order > DPEMU_LANES_SHOT_MAJOR)
            return refuse(pl, DPEMU_E_INVALID, "lane_order %u is not DPEMU_LANES_CORE_MAJOR / SHOT_MAJOR",
                          cfg->lane_order);
        if (n % C)
            return refuse(pl, DPEMU_E_INVALID, "run layout: n_cols %u is not a multiple of cores_per_shot %u", n, C);
    } else {
        for (uint32_t i = 0; i < n; i++)
            if (cols->core[i] >= C)
                return refuse(pl, DPEMU_E_INVALID, "column %u: core %u >= cores_per_shot", i, cols->core[i]);
        pl.tab.resize(12ull * n);
        if (n) {
            memcpy(pl.tab.data(), cols->shot, 8ull * n);
            memcpy(pl.tab.data() + 8ull * n, cols->core, 4ull * n);
        }
    }
    for (uint32_t c = 0; c < DPEMU_MAX_CORES; c++) {
        pl.p1[c] = cfg->p1_threshold[c];
        pl.axis[c] = (cols->axis && c < C) ? cols->axis[c] : cfg->ro_axis[c];
        pl.thr[c] = (cols->thr && c < C) ? cols->thr[c] : cfg->ro_thr;
    }
    return pl;
}

}  // namespace dpemu
