// capi.cpp -- the extern "C" boundary of libdpemu.so (include/dpemu.h).
//
// Replaces the reference's simulation harness: where the
// cocotb testbench loaded cmd_mem word by word (cocotb/proc/test_proc.py:29-38)
// and clocked one Verilator toplevel_sim, dpemu_load_programs uploads every
// assembled program once and dpemu_run executes n_shots x C cores on the GPU.
// This file holds the entry points, the context's lifetime and the uploads:
// an entry point checks its own pointer arguments, asks a planner, refuses
// with the planner's message or uploads the planner's tables, fills the
// kernel's parameter block and launches.  What is refused, what is uploaded
// and which kernel runs is decided in program_image.h (the load-time image),
// stage_plan.h (the argument checks and device tables of the calls) and
// launch_plan.h (the per-call choices), all host-only.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "kernels.h"
#include "launch_plan.h"
#include "lds_grants.h"
#include "program_image.h"
#include "stage_plan.h"

using namespace dpemu;

namespace dpemu {
static LdsGrants g_lds_grants;     // the process's dynamic-LDS opt-ins, per (device, kernel)

hipError_t opt_in_dynamic_lds(const void *fn, size_t bytes)
{
    if (bytes <= LdsGrants::DEFAULT_LIMIT) return hipSuccess;
    int dev = 0;
    const hipError_t de = hipGetDevice(&dev);
    if (de != hipSuccess) return de;
    return (hipError_t)g_lds_grants.ensure(dev, fn, bytes, [&] {
        return (int)hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    });
}
}  // namespace dpemu

static int fail(dpemu_ctx *ctx, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));

// A device buffer the context keeps across calls, with the host copy of the
// bytes it holds.  Tables (channel, pair, line, resonator, column descriptors)
// change rarely: upload() copies only when the bytes differ from the cache.
// Scratch buffers (event indexes, histogram replicas) only reserve().  Both
// grow and never shrink, and synchronise the stream before they free or
// overwrite what an earlier launch may still read.
struct DevTable {
    void *d = nullptr;
    size_t cap = 0;                         // bytes allocated
    std::vector<uint8_t> cache;             // the bytes on the device (empty: none known)

    template <class T> T *as() const { return static_cast<T *>(d); }

    hipError_t reserve(size_t bytes, hipStream_t s)
    {
        if (bytes <= cap) return hipSuccess;
        hipError_t e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        (void)hipFree(d);
        d = nullptr; cap = 0;
        cache.clear();
        e = hipMalloc(&d, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }

    hipError_t upload(const void *src, size_t bytes, hipStream_t s)
    {
        if (bytes == cache.size() && (!bytes || !memcmp(cache.data(), src, bytes))) return hipSuccess;
        hipError_t e = bytes > cap ? reserve(bytes, s) : hipStreamSynchronize(s);   // an earlier launch may still read it
        if (e != hipSuccess) return e;
        cache.clear();                      // not valid until the copy has landed
        e = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        if (e == hipSuccess) cache.assign(static_cast<const uint8_t *>(src), static_cast<const uint8_t *>(src) + bytes);
        return e;
    }
    template <class T> hipError_t upload(const std::vector<T> &v, hipStream_t s) { return upload(v.data(), v.size() * sizeof(T), s); }

    void release() { (void)hipFree(d); d = nullptr; cap = 0; cache.clear(); }
};

struct dpemu_ctx {
    int device = 0;
    uint32_t n_cu = 256;                    // compute units of the device (hipDeviceAttributeMultiprocessorCount)
    std::string err;
    // programs (program_image.h)
    uint4 *d_uops = nullptr;                // decode_cmd words, program-major (KParams::uops)
    uint4 *d_uops_t = nullptr;              // command-major copy (KParams::fetch), or null
    uint4 *d_macro = nullptr;               // macro image of branch-free ALU programs (macro.hip), or null
    uint32_t *d_moff = nullptr;             // its per-program offsets (in macros)
    uint32_t *d_mchunk = nullptr, *d_mcoff = nullptr;   // lean chunks (mark_lean_chunks) and their offsets
    uint32_t *d_offsets = nullptr, *d_ninstr = nullptr, *d_table = nullptr;
    ProgramFacts facts;                     // what the kernel choice reads of them (n_programs == 0: none loaded)
    // DEMOD frequency tables (dpemu_load_readout_freqs), per loaded program
    uint32_t *d_ro_fq = nullptr;
    uint4 *d_ro_hdr = nullptr;
    // run constants: p1 thresholds [64] then DEMOD axes [64]
    uint32_t *d_thr = nullptr;
    uint64_t *d_lut = nullptr;
    std::vector<uint32_t> thr_cache;
    std::vector<uint64_t> lut_cache;
    int16_t *d_sin = nullptr;               // Q15 sine table of the DDS
    DevTable ch;                            // DDS channel descriptors
    DevTable dds_index;                     // event index of dds_index_kernel
    DevTable pairs;                         // pair table of dpemu_demod_iq and the feedline stages
    // multiplexed readout (dpemu_feedline_adc / dpemu_demod_feedline): the line table (line_first |
    // member | line_of | wg_first) and the readout index feedline_index_kernel writes
    DevTable lines, fl_index;
    DevTable res;                           // resonator coefficients (dpemu_feedline_adc_res), four zero words after them
    DevTable iqcols;                        // dpemu_iq_stats explicit columns: [n] u64 shots then [n] u32 cores
    uint32_t iq_wgs_per_cu = 0;             // resident iq_stats_kernel workgroups per CU (0: not asked yet)
    DevTable trace_tab;                     // dpemu_feedline_traces: chunk descriptors, then the sorted pair indices
    uint32_t trace_wgs_per_cu = 0;          // resident feedline_trace_kernel workgroups per CU (0: not asked yet)
    DevTable qsim_tab;                      // dpemu_qsim: phase table, registers, detunings and the gate dictionary
    DevTable qsim_decay_tab;                // dpemu_qsim_decay: per core damp[32], deph[32]
    std::string last_kernel;               // variant the last dpemu_run launched (dpemu_last_kernel)
    // kernel timing (dpemu_set_kernel_timing): event pairs recorded around main kernels
    bool timing = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_used, ev_free;
    // privatised outcome histograms (R replicas, reduced after the interpreter)
    DevTable hist_rep;
    bool hist_rep_dirty = true;     // replicas not known to be zero
    // call ordering across streams: the last call's stream and an event after its work
    // (ord_pending: not recorded yet -- order_begin)
    hipEvent_t ord_ev = nullptr;
    hipStream_t ord_stream = nullptr;
    bool ord_valid = false, ord_pending = false;
};

static int fail(dpemu_ctx *ctx, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                  \
    do {                                                                                   \
        hipError_t e_ = (call);                                                            \
        if (e_ != hipSuccess)                                                              \
            return fail(ctx, DPEMU_E_DEVICE, "%s: %s", #call, hipGetErrorString(e_));      \
    } while (0)

// the pointer arguments of an entry point: the first that is NULL is named (an entry without a name is not asked for)
struct NamedPtr { const void *p; const char *name; };
static int check_ptrs(dpemu_ctx *ctx, const char *what, std::initializer_list<NamedPtr> ptrs)
{
    for (const NamedPtr &a : ptrs)
        if (a.name && !a.p) return fail(ctx, DPEMU_E_INVALID, "%s: %s is NULL", what, a.name);
    return DPEMU_OK;
}

// Work of one context runs in call order whatever the streams: a call on a
// stream other than the previous call's first waits for the previous call's
// work (the scratch buffers -- histogram replicas, DDS index, thresholds, LUT
// table, channel descriptors -- are shared by the context's calls).  The event
// that marks the end of a call's work is recorded when the call returns,
// except on the default stream (handle 0), where it is recorded only when
// somebody needs it -- a call on another stream, a reload, the destroy -- and
// then covers at least that call's work: most contexts never leave the
// default stream, and a marker after every launch costs step time (DESIGN.md
// §4.5).  A created stream may be destroyed by its owner between two calls,
// so a late record on it could be invalid: those keep the record at the end
// of the call.
static hipError_t order_mark(dpemu_ctx *ctx)
{
    if (!ctx->ord_pending) return hipSuccess;
    const hipError_t e = hipEventRecord(ctx->ord_ev, ctx->ord_stream);
    ctx->ord_pending = false;
    ctx->ord_valid = e == hipSuccess;
    return e;
}

static hipError_t order_begin(dpemu_ctx *ctx, hipStream_t s)
{
    if (s == ctx->ord_stream) return hipSuccess;
    const hipError_t e = order_mark(ctx);
    if (e != hipSuccess) return e;
    return ctx->ord_valid ? hipStreamWaitEvent(s, ctx->ord_ev, 0) : hipSuccess;
}

static hipError_t order_end(dpemu_ctx *ctx, hipStream_t s)
{
    ctx->ord_stream = s;
    ctx->ord_pending = true;
    return s ? order_mark(ctx) : hipSuccess;   // the default stream: when it is needed
}

// the host waits for the context's work (whose buffers are about to be freed)
static hipError_t order_sync(dpemu_ctx *ctx)
{
    const hipError_t e = order_mark(ctx);
    if (e != hipSuccess) return e;
    return ctx->ord_valid ? hipEventSynchronize(ctx->ord_ev) : hipSuccess;
}

// A main-kernel launch on `stream`, between the events of a timing pair while
// kernel timing is on (dpemu_set_kernel_timing)
template <class Launch> static hipError_t timed(dpemu_ctx *ctx, hipStream_t stream, Launch launch)
{
    if (!ctx->timing) return launch();
    std::pair<hipEvent_t, hipEvent_t> e;
    if (!ctx->ev_free.empty()) {
        e = ctx->ev_free.back();
        ctx->ev_free.pop_back();
    } else {
        hipError_t r = hipEventCreate(&e.first);
        if (r != hipSuccess) return r;
        r = hipEventCreate(&e.second);
        if (r != hipSuccess) { (void)hipEventDestroy(e.first); return r; }
    }
    ctx->ev_used.push_back(e);
    hipError_t r = hipEventRecord(e.first, stream);
    if (r == hipSuccess) r = launch();
    if (r == hipSuccess) r = hipEventRecord(e.second, stream);
    return r;
}

// the readout fields of dpemu_config in a kernel's parameter block (KParams, DemodParams, FeedlineParams)
template <class P> static void set_readout(P &p, const dpemu_config *cfg)
{
    p.seed = cfg->seed;
    p.meas_elem = cfg->meas_elem; p.ro_cpw = cfg->ro_cpw; p.ro_delay = cfg->ro_delay;
    p.ro_theta0 = cfg->ro_theta[0]; p.ro_theta1 = cfg->ro_theta[1];
    p.ro_gain0 = cfg->ro_gain[0]; p.ro_gain1 = cfg->ro_gain[1];
    p.ro_sigma = cfg->ro_sigma; p.ro_thr = cfg->ro_thr;
}

// n u32 words of a program image in a new device buffer (none, and a null pointer, for an empty one)
template <class T> static hipError_t to_device(T *&d, const uint32_t *src, uint64_t n)
{
    if (!n) return hipSuccess;
    const hipError_t e = hipMalloc(&d, n * 4);
    return e != hipSuccess ? e : hipMemcpy(d, src, n * 4, hipMemcpyHostToDevice);
}

static void free_programs(dpemu_ctx *ctx)
{
    for (void *q : {(void *)ctx->d_uops, (void *)ctx->d_uops_t, (void *)ctx->d_macro, (void *)ctx->d_moff,
                    (void *)ctx->d_mchunk, (void *)ctx->d_mcoff,
                    (void *)ctx->d_offsets, (void *)ctx->d_ninstr, (void *)ctx->d_table})
        (void)hipFree(q);
    ctx->d_uops = ctx->d_uops_t = ctx->d_macro = nullptr;
    ctx->d_mchunk = ctx->d_mcoff = nullptr;
    ctx->d_moff = ctx->d_offsets = ctx->d_ninstr = ctx->d_table = nullptr;
    ctx->facts = ProgramFacts();
    (void)hipFree(ctx->d_ro_fq);
    (void)hipFree(ctx->d_ro_hdr);
    ctx->d_ro_fq = nullptr;
    ctx->d_ro_hdr = nullptr;
}

extern "C" {

int dpemu_abi_version(void) { return DPEMU_ABI_VERSION; }

int dpemu_struct_sizes(uint64_t *out)
{
    if (!out) return DPEMU_E_INVALID;
    out[0] = sizeof(dpemu_config);
    out[1] = sizeof(dpemu_outputs);
    out[2] = sizeof(dpemu_dds_channels);
    return DPEMU_OK;
}

int dpemu_create(int device, dpemu_ctx **out)
{
    if (!out) return DPEMU_E_INVALID;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || device < 0 || device >= n) return DPEMU_E_DEVICE;
    if (hipSetDevice(device) != hipSuccess) return DPEMU_E_DEVICE;
    dpemu_ctx *ctx = new dpemu_ctx();
    ctx->device = device;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
        ctx->n_cu = (uint32_t)cus;
    std::vector<int16_t> lut(4096);
    dpemu_dds_sin_lut(lut.data());
    if (hipMalloc(&ctx->d_thr, 2 * DPEMU_MAX_CORES * sizeof(uint32_t)) != hipSuccess ||
        hipMalloc(&ctx->d_lut, 256 * sizeof(uint64_t)) != hipSuccess ||
        hipMalloc(&ctx->d_sin, 4096 * sizeof(int16_t)) != hipSuccess ||
        hipMemcpy(ctx->d_sin, lut.data(), 4096 * sizeof(int16_t), hipMemcpyHostToDevice) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ord_ev, hipEventDisableTiming) != hipSuccess) {
        dpemu_destroy(ctx);
        return DPEMU_E_NOMEM;
    }
    *out = ctx;
    return DPEMU_OK;
}

int dpemu_destroy(dpemu_ctx *ctx)
{
    if (!ctx) return DPEMU_E_INVALID;
    (void)hipSetDevice(ctx->device);
    (void)order_sync(ctx);                  // the context's work is done with its buffers
    free_programs(ctx);
    (void)hipFree(ctx->d_thr); (void)hipFree(ctx->d_lut); (void)hipFree(ctx->d_sin);
    for (DevTable *t : {&ctx->ch, &ctx->dds_index, &ctx->pairs, &ctx->lines, &ctx->fl_index, &ctx->res, &ctx->iqcols,
                        &ctx->trace_tab, &ctx->qsim_tab, &ctx->qsim_decay_tab, &ctx->hist_rep})
        t->release();
    for (auto *v : {&ctx->ev_used, &ctx->ev_free})
        for (auto &e : *v) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    if (ctx->ord_ev) (void)hipEventDestroy(ctx->ord_ev);
    delete ctx;
    return DPEMU_OK;
}

const char *dpemu_last_error(dpemu_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

const char *dpemu_last_kernel(dpemu_ctx *ctx) { return ctx ? ctx->last_kernel.c_str() : ""; }

int dpemu_set_kernel_timing(dpemu_ctx *ctx, int enable)
{
    if (!ctx) return DPEMU_E_INVALID;
    ctx->timing = enable != 0;
    return DPEMU_OK;
}

int dpemu_kernel_times(dpemu_ctx *ctx, float *ms, int max_n, int *n_out)
{
    if (!ctx || (max_n > 0 && !ms)) return DPEMU_E_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int n = 0;
    for (auto &e : ctx->ev_used) {
        HIPCHK(ctx, hipEventSynchronize(e.second));
        if (n < max_n) HIPCHK(ctx, hipEventElapsedTime(&ms[n], e.first, e.second));
        n++;
    }
    ctx->ev_free.insert(ctx->ev_free.end(), ctx->ev_used.begin(), ctx->ev_used.end());
    ctx->ev_used.clear();
    if (n_out) *n_out = n < max_n ? n : max_n;
    return DPEMU_OK;
}

int dpemu_load_programs(dpemu_ctx *ctx, const uint32_t *words, uint64_t n_cmds, const uint32_t *offsets,
                        const uint32_t *n_instr, uint32_t n_programs, const uint32_t *prog_table,
                        uint32_t n_groups, uint32_t cores_per_shot)
{
    if (!ctx) return DPEMU_E_INVALID;
    if ((!words && n_cmds) || !offsets || !n_instr || !prog_table || n_programs == 0 || n_groups == 0)
        return fail(ctx, DPEMU_E_INVALID, "load_programs: null array or empty program set");
    const uint32_t C = cores_per_shot;
    if (C == 0 || C > DPEMU_MAX_CORES || (C & (C - 1)))
        return fail(ctx, DPEMU_E_INVALID, "cores_per_shot %u is not a power of two in [1, 64]", C);
    if ((uint64_t)n_groups * C > 0xFFFFFFFFull) return fail(ctx, DPEMU_E_INVALID, "n_groups * C exceeds 2^32");
    for (uint32_t i = 0; i < n_programs; i++) {
        if (n_instr[i] > 65536u)
            return fail(ctx, DPEMU_E_INVALID, "program %u: %u commands exceed the 2^16-deep cmd_mem", i, n_instr[i]);
        if ((uint64_t)offsets[i] + n_instr[i] > n_cmds)
            return fail(ctx, DPEMU_E_INVALID, "program %u: offset %u + %u commands run past the %llu commands",
                        i, offsets[i], n_instr[i], (unsigned long long)n_cmds);
    }
    for (uint64_t i = 0; i < (uint64_t)n_groups * C; i++)
        if (prog_table[i] >= n_programs)
            return fail(ctx, DPEMU_E_INVALID, "prog_table[%llu] = %u >= n_programs", (unsigned long long)i, prog_table[i]);
    const ProgramImage im = build_program_image(words, offsets, n_instr, n_programs, prog_table, n_groups, C);
    if (!im.err.empty()) return fail(ctx, DPEMU_E_INVALID, "%s", im.err.c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, order_sync(ctx));           // earlier runs may still read the old image
    free_programs(ctx);
    HIPCHK(ctx, to_device(ctx->d_uops, im.uops.data(), im.uops.size()));
    HIPCHK(ctx, to_device(ctx->d_uops_t, im.uops_t.data(), im.uops_t.size()));
    HIPCHK(ctx, to_device(ctx->d_macro, im.macro.data(), im.macro.size()));
    HIPCHK(ctx, to_device(ctx->d_moff, im.moff.data(), im.moff.size()));
    HIPCHK(ctx, to_device(ctx->d_mchunk, im.mchunk.data(), im.mchunk.size()));
    HIPCHK(ctx, to_device(ctx->d_mcoff, im.mcoff.data(), im.mcoff.size()));
    HIPCHK(ctx, to_device(ctx->d_offsets, im.goff.data(), n_programs));
    HIPCHK(ctx, to_device(ctx->d_ninstr, n_instr, n_programs));
    HIPCHK(ctx, to_device(ctx->d_table, prog_table, (uint64_t)n_groups * C));
    ctx->facts = im.facts;
    return DPEMU_OK;
}

int dpemu_load_readout_freqs(dpemu_ctx *ctx, const uint32_t *words, uint64_t n_words, const uint32_t *drv_off,
                             const uint32_t *drv_len, const uint32_t *lo_off, const uint32_t *lo_len)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (!ctx->facts.n_programs) return fail(ctx, DPEMU_E_NOPROG, "load_readout_freqs before load_programs");
    if ((!words && n_words) || !drv_off || !drv_len || !lo_off || !lo_len)
        return fail(ctx, DPEMU_E_INVALID, "load_readout_freqs: null array");
    std::vector<uint32_t> hdr(4ull * ctx->facts.n_programs);
    for (uint32_t i = 0; i < ctx->facts.n_programs; i++) {
        if ((uint64_t)drv_off[i] + drv_len[i] > n_words || (uint64_t)lo_off[i] + lo_len[i] > n_words)
            return fail(ctx, DPEMU_E_INVALID, "load_readout_freqs: program %u's table runs past the %llu words", i,
                        (unsigned long long)n_words);
        hdr[4 * i] = drv_off[i]; hdr[4 * i + 1] = drv_len[i]; hdr[4 * i + 2] = lo_off[i]; hdr[4 * i + 3] = lo_len[i];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, order_sync(ctx));           // earlier runs may still read the old tables
    (void)hipFree(ctx->d_ro_fq);
    (void)hipFree(ctx->d_ro_hdr);
    ctx->d_ro_fq = nullptr;
    ctx->d_ro_hdr = nullptr;
    HIPCHK(ctx, hipMalloc(&ctx->d_ro_fq, std::max<uint64_t>(n_words, 1) * 4));
    if (n_words) HIPCHK(ctx, hipMemcpy(ctx->d_ro_fq, words, n_words * 4, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMalloc(&ctx->d_ro_hdr, hdr.size() * 4));
    HIPCHK(ctx, hipMemcpy(ctx->d_ro_hdr, hdr.data(), hdr.size() * 4, hipMemcpyHostToDevice));
    return DPEMU_OK;
}

static int validate(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t n_shots, bool want_hist)
{
    const Refusal r = check_run(ctx->facts, ctx->d_ro_hdr != nullptr, cfg, n_shots, want_hist);
    return r.refused() ? fail(ctx, r.code, "%s", r.err.c_str()) : DPEMU_OK;
}

// `states`: dpemu_run_states' per-lane words (null: dpemu_run, the draws)
static int run_impl(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
                    const dpemu_outputs *out, hipStream_t stream, const uint32_t *states = nullptr)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, order_begin(ctx, stream));
    const uint32_t C = cfg->cores_per_shot;
    // run constants, uploaded when they change (stream-ordered: the copy lands
    // before this call's kernel and after the previous call's)
    std::vector<uint32_t> thr(cfg->p1_threshold, cfg->p1_threshold + DPEMU_MAX_CORES);
    thr.insert(thr.end(), cfg->ro_axis, cfg->ro_axis + DPEMU_MAX_CORES);   // d_thr[64..127]: DEMOD axes
    std::vector<uint64_t> lut(cfg->lut_table, cfg->lut_table + 256);
    if (thr != ctx->thr_cache) {
        ctx->thr_cache = thr;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_thr, ctx->thr_cache.data(), thr.size() * 4, hipMemcpyHostToDevice, stream));
    }
    if (lut != ctx->lut_cache) {
        ctx->lut_cache = lut;
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_lut, ctx->lut_cache.data(), lut.size() * 8, hipMemcpyHostToDevice, stream));
    }
    KParams p{};
    const ProgramFacts &f = ctx->facts;
    const RunPlan pl = plan_run(f, cfg, n_shots, out->hist != nullptr, states != nullptr);
    p.states = states;
    p.uops = ctx->d_uops;
    p.fetch = pl.cmd_major ? ctx->d_uops_t : ctx->d_uops;
    p.fetch_stride = pl.cmd_major ? f.n_programs : 1u;
    p.offsets = ctx->d_offsets; p.n_instr = ctx->d_ninstr; p.prog_table = ctx->d_table;
    p.max_len = f.max_len;
    p.macros = ctx->d_macro; p.macro_off = ctx->d_moff;
    p.macro_chunk = ctx->d_mchunk; p.macro_coff = ctx->d_mcoff;
    p.reg_map = f.reg_map; p.reg_inv = f.reg_inv; p.reg_used = f.reg_used;
    p.macro_rs = f.macro_rs;
    p.macro_w3 = f.macro_w3 ? 1u : 0u;
    p.p1_thr = ctx->d_thr; p.lut_table = ctx->d_lut;
    p.summary = out->summary;
    p.events = reinterpret_cast<uint4 *>(out->events);
    p.trace = reinterpret_cast<uint4 *>(out->trace);
    p.meas = reinterpret_cast<uint2 *>(out->meas);
    p.regs_out = out->regs;
    p.hist = reinterpret_cast<unsigned long long *>(out->hist);
    p.hist_next = reinterpret_cast<unsigned long long *>(out->hist_next);
    p.hist_bins = (uint64_t)cfg->n_groups << C;
    p.shot_begin = shot_begin;
    p.n_lanes = (uint32_t)(n_shots * C);
    p.n_shots = (uint32_t)n_shots;
    p.shot_major = cfg->lane_order == DPEMU_LANES_SHOT_MAJOR;
    p.C = C;
    p.log2C = 0;
    while ((1u << p.log2C) < C) p.log2C++;
    p.n_groups = cfg->n_groups; p.shots_per_group = cfg->shots_per_group;
    p.grp_g0 = (uint32_t)((shot_begin / cfg->shots_per_group) % cfg->n_groups);
    p.grp_r0 = (uint32_t)(shot_begin % cfg->shots_per_group);
    fast_div_init(cfg->shots_per_group, p.spg_div);
    fast_div_init(cfg->n_groups, p.ng_div);
    p.max_cycles = cfg->max_cycles;
    p.event_cap = cfg->event_cap;           // the overflow flags follow the caps whether or not a buffer is given
    p.trace_cap = cfg->trace_cap;
    p.meas_cap = cfg->meas_cap;
    p.fproc_mode = cfg->fproc_mode;
    p.meas_latency = cfg->meas_latency; p.sync_latency = cfg->sync_latency;
    const uint64_t all = (C >= 64) ? ~0ull : ((1ull << C) - 1);
    p.sync_mask = cfg->sync_mask ? (cfg->sync_mask & all) : all;
    set_readout(p, cfg);
    p.meas_model = cfg->meas_model; p.ro_sep = cfg->ro_sep;
    p.ro_win = cfg->ro_win;
    p.ro_wrecip = cfg->ro_win ? (1u << 24) / cfg->ro_win : 0u;
    p.ro_drv_elem = cfg->ro_drv_elem;
    p.ro_axis = ctx->d_thr + DPEMU_MAX_CORES;
    p.ro_fq = ctx->d_ro_fq; p.ro_hdr = ctx->d_ro_hdr;
    p.acc = reinterpret_cast<int2 *>(out->acc);
    p.lut_mask = cfg->lut_mask;
    const uint64_t guard = (uint64_t)C * (cfg->max_cycles / 3u + 4u) + 1024u;
    p.iter_guard = guard > 0xFFFFFFF0ull ? 0xFFFFFFF0u : (uint32_t)guard;
    p.ev_stream = (cfg->exec_flags & DPEMU_X_STREAM_EVENTS) ? 1u : 0u;
    p.prog_lds_words = pl.prog_lds_words;
    // the outcome histogram (plan_run): direct atomics into out->hist, or R
    // privatised replicas picked by workgroup, then the reduce kernel -- or,
    // with hist_fold, straight_kernel's own last workgroup in its place
    if (pl.hist_repl) {
        const size_t cap0 = ctx->hist_rep.cap;
        HIPCHK(ctx, ctx->hist_rep.reserve((size_t)pl.hist_rep_words() * 4, stream));   // earlier work may still use the old replicas
        if (ctx->hist_rep.cap != cap0) ctx->hist_rep_dirty = true;
        // the reduce (kernel or folded) leaves every replica word it read and
        // every ticket zero, so the allocation is zeroed once (or after a failed run)
        if (ctx->hist_rep_dirty) {
            HIPCHK(ctx, hipMemsetAsync(ctx->hist_rep.d, 0, ctx->hist_rep.cap, stream));
            ctx->hist_rep_dirty = false;
        }
        if (!pl.hist_fold) p.hist = nullptr;
        p.hist_fold = !pl.hist_fold ? 0u : cfg->hist_assign ? HIST_FOLD_ASSIGN : HIST_FOLD_ADD;
        p.hist_rep = ctx->hist_rep.as<uint32_t>();
        p.hist_reps = pl.R;
        p.hist_stride = pl.hist_stride;
        p.hist_lds = pl.hist_lds;
    }
    if (out->hist && !p.hist_rep && cfg->hist_assign)      // direct atomics: assign = zero, then add
        HIPCHK(ctx, hipMemsetAsync(out->hist, 0, pl.bins * sizeof(uint64_t), stream));
    // from the main launch until the reduce is enqueued the replicas may hold
    // counts: a failure in between leaves them to the next run's memset
    if (p.hist_rep) ctx->hist_rep_dirty = true;
    HIPCHK(ctx, timed(ctx, stream, [&] {
        switch (pl.family) {
        case K_STRAIGHT: return launch_straight(p, pl.src, pl.fetch_batch, stream);
        case K_MACRO: return launch_macro(p, pl.slots, f.macro_nr, f.macro_addid, stream);
        case K_BRANCH: return launch_branch(p, pl.bfeat, stream);
        default: return launch_interp(p, pl.feat, stream);
        }
    }));
    ctx->last_kernel = pl.name;
    if (p.hist_rep) {
        if (!pl.hist_fold)
            HIPCHK(ctx, launch_hist_reduce(p.hist_rep, pl.R, pl.hist_stride, pl.bins, cfg->hist_assign != 0,
                                           reinterpret_cast<unsigned long long *>(out->hist), stream));
        ctx->hist_rep_dirty = false;
    }
    HIPCHK(ctx, order_end(ctx, stream));
    return DPEMU_OK;
}

// dpemu_run and, with `states`, dpemu_run_states
static int run_device(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
                      const dpemu_outputs *out, const uint32_t *states, void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (!out) return fail(ctx, DPEMU_E_INVALID, "null outputs");
    int rc = validate(ctx, cfg, n_shots, out->hist != nullptr || out->hist_next != nullptr);
    if (rc) return rc;
    if (out->acc && cfg->meas_model != DPEMU_MEAS_DEMOD)
        return fail(ctx, DPEMU_E_INVALID, "acc: DEMOD runs only");
    if (states && cfg->meas_model == DPEMU_MEAS_DEMOD)
        return fail(ctx, DPEMU_E_INVALID, "dpemu_run_states: meas_model DEMOD with states (the *_st readout stages "
                                          "take the states of a DEMOD chain)");
    if (reinterpret_cast<uintptr_t>(states) % sizeof(uint32_t))
        return fail(ctx, DPEMU_E_INVALID, "dpemu_run_states: states is not 4-byte aligned");
    if (out->hist_next) {
        const uint64_t bytes = ((uint64_t)cfg->n_groups << cfg->cores_per_shot) * sizeof(uint64_t);
        const uintptr_t a = (uintptr_t)out->hist, b = (uintptr_t)out->hist_next;
        if (out->hist && a < b + bytes && b < a + bytes)
            return fail(ctx, DPEMU_E_INVALID, "hist_next overlaps hist");
        if (b % sizeof(uint64_t)) return fail(ctx, DPEMU_E_INVALID, "hist_next is not 8-byte aligned");
    }
    if (n_shots == 0) {
        if (out->hist_next) {                                // the contract holds for an empty run too,
            hipStream_t s = (hipStream_t)stream;             // in call order like any other call
            HIPCHK(ctx, hipSetDevice(ctx->device));
            HIPCHK(ctx, order_begin(ctx, s));
            HIPCHK(ctx, hipMemsetAsync(out->hist_next, 0,
                                       ((size_t)cfg->n_groups << cfg->cores_per_shot) * sizeof(uint64_t), s));
            HIPCHK(ctx, order_end(ctx, s));
        }
        return DPEMU_OK;
    }
    return run_impl(ctx, cfg, shot_begin, n_shots, out, (hipStream_t)stream, states);
}

int dpemu_run(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
              const dpemu_outputs *out, void *stream)
{
    return run_device(ctx, cfg, shot_begin, n_shots, out, nullptr, stream);
}

int dpemu_run_states(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
                     const dpemu_outputs *out, const uint32_t *states, void *stream)
{
    return run_device(ctx, cfg, shot_begin, n_shots, out, states, stream);
}

int dpemu_run_host(dpemu_ctx *ctx, const dpemu_config *cfg, uint64_t shot_begin, uint64_t n_shots,
                   const dpemu_outputs *host_out)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (!host_out) return fail(ctx, DPEMU_E_INVALID, "null outputs");
    if (host_out->hist_next) return fail(ctx, DPEMU_E_INVALID, "hist_next: device runs (dpemu_run) only");
    int rc = validate(ctx, cfg, n_shots, host_out->hist != nullptr);
    if (rc) return rc;
    if (host_out->acc && cfg->meas_model != DPEMU_MEAS_DEMOD)
        return fail(ctx, DPEMU_E_INVALID, "acc: DEMOD runs only");
    if (n_shots == 0) return DPEMU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const uint64_t nl = n_shots * cfg->cores_per_shot;
    struct Buf { void *host; void *dev; size_t bytes; bool in; };
    Buf bufs[7] = {
        {host_out->summary, nullptr, nl * 32, false},
        {host_out->events, nullptr, (size_t)cfg->event_cap * nl * 16, false},
        {host_out->trace, nullptr, (size_t)cfg->trace_cap * nl * 16, false},
        {host_out->meas, nullptr, (size_t)cfg->meas_cap * nl * 8, false},
        {host_out->regs, nullptr, nl * 64, false},
        {host_out->hist, nullptr, (size_t)cfg->n_groups * (cfg->cores_per_shot <= 12 ? (1u << cfg->cores_per_shot) : 0) * 8, true},
        {host_out->acc, nullptr, (size_t)cfg->meas_cap * nl * 8, false},
    };
    int result = DPEMU_OK;
    for (auto &b : bufs) {
        if (!b.host || !b.bytes) { b.host = nullptr; continue; }
        if (hipMalloc(&b.dev, b.bytes) != hipSuccess) { result = fail(ctx, DPEMU_E_NOMEM, "device allocation of %zu bytes failed", b.bytes); break; }
        hipError_t e = b.in ? hipMemcpy(b.dev, b.host, b.bytes, hipMemcpyHostToDevice) : hipMemset(b.dev, 0, b.bytes);
        if (e != hipSuccess) { result = fail(ctx, DPEMU_E_DEVICE, "%s", hipGetErrorString(e)); break; }
    }
    if (result == DPEMU_OK) {
        dpemu_outputs d{};
        d.summary = (uint32_t *)bufs[0].dev; d.events = (uint32_t *)bufs[1].dev;
        d.trace = (uint32_t *)bufs[2].dev; d.meas = (uint32_t *)bufs[3].dev;
        d.regs = (uint32_t *)bufs[4].dev; d.hist = (uint64_t *)bufs[5].dev;
        d.acc = (int32_t *)bufs[6].dev;
        result = run_impl(ctx, cfg, shot_begin, n_shots, &d, nullptr);
        if (result == DPEMU_OK) {
            hipError_t e = hipDeviceSynchronize();
            if (e != hipSuccess) result = fail(ctx, DPEMU_E_DEVICE, "kernel: %s", hipGetErrorString(e));
        }
        for (auto &b : bufs)
            if (result == DPEMU_OK && b.host && b.dev &&
                hipMemcpy(b.host, b.dev, b.bytes, hipMemcpyDeviceToHost) != hipSuccess)
                result = fail(ctx, DPEMU_E_DEVICE, "copy back failed");
    }
    (void)hipDeviceSynchronize();
    for (auto &b : bufs) if (b.dev) (void)hipFree(b.dev);
    return result;
}

// Q15 sine table of the DDS: round(32767 sin(2 pi i / 4096)), built with integer-exact
// symmetry from the first quadrant so every build gets the same bytes.
int dpemu_dds_sin_lut(int16_t *out)
{
    if (!out) return DPEMU_E_INVALID;
    for (int i = 0; i <= 1024; i++) {
        const double v = std::round(32767.0 * std::sin(2.0 * M_PI * (double)i / 4096.0));
        const int16_t q = (int16_t)v;
        out[i & 4095] = q;                 // [0, pi/2]
        if (i < 1024) out[2048 - i] = q;   // (pi/2, pi]
        out[(2048 + i) & 4095] = (int16_t)-q;
        if (i < 1024 && i > 0) out[4096 - i] = (int16_t)-q;
    }
    return DPEMU_OK;
}

}  // extern "C"

extern "C" int dpemu_dds(dpemu_ctx *ctx, const dpemu_dds_channels *ch, const uint32_t *summary,
                         const uint32_t *events, const uint32_t *env_tables, const uint32_t *freq_tables,
                         int16_t *iq_out, void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (!ch || !summary || !events || !env_tables || !freq_tables || !iq_out)
        return fail(ctx, DPEMU_E_INVALID, "dpemu_dds: null argument");
    const ChannelPlan cp = plan_channels(ch);
    if (cp.refused()) return fail(ctx, cp.code, "%s", cp.err.c_str());
    if (ch->n_channels == 0 || ch->n_samples == 0) return DPEMU_OK;
    const DdsPlan pl = plan_dds(cp.desc.data(), ch->n_channels, ch->n_samples, ch->event_cap);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, order_begin(ctx, s));
    HIPCHK(ctx, ctx->ch.upload(cp.desc, s));   // descriptors change rarely: uploaded only then
    DDSParams p{};
    p.summary = summary;
    p.events = reinterpret_cast<const uint4 *>(events);
    p.env = env_tables; p.freq = freq_tables;
    p.sin_lut = ctx->d_sin;
    p.ch = ctx->ch.as<uint32_t>();
    p.iq = reinterpret_cast<uint32_t *>(iq_out);
    p.n_channels = ch->n_channels; p.n_lanes = ch->n_lanes; p.n_samples = ch->n_samples;
    p.event_cap = ch->event_cap;
    p.ev_lds = pl.ev_lds; p.rec_lds = pl.rec_lds; p.env_lds = pl.env_lds; p.freq_lds = pl.freq_lds;
    p.tiles = pl.tiles; p.stripes = pl.stripes; p.wg_tiles = pl.wg_tiles;
    HIPCHK(ctx, ctx->dds_index.reserve(dds_index_bytes(p.n_channels, p.ev_lds), s));   // the event index
    uint8_t *b = ctx->dds_index.as<uint8_t>();
    p.xs = reinterpret_cast<uint4 *>(b);
    p.xr = reinterpret_cast<uint32_t *>(b + (uint64_t)p.n_channels * p.ev_lds * 16);
    p.cnt = reinterpret_cast<uint2 *>(b + (uint64_t)p.n_channels * p.ev_lds * 20);
    p.pair_lanes = cp.pair_lanes;
    HIPCHK(ctx, launch_dds_index(p, s));   // outside the timed bracket: it holds the synthesis kernel alone
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_dds(p, s); }));
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

extern "C" int dpemu_demod_iq(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                              const uint32_t *summary, const uint32_t *events, const uint32_t *iq_drv,
                              const uint32_t *iq_lo, int32_t *acc, uint32_t *result, void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_ptrs(ctx, "dpemu_demod_iq", {{cfg, "cfg"}, {pairs, "pairs"}, {summary, "summary"},
                                                   {events, "events"}, {iq_drv, "iq_drv"}, {iq_lo, "iq_lo"},
                                                   {acc, "acc"}, {result, "result"}}))
        return rc;
    PairPlan pl = check_pairs(cfg, pairs, "dpemu_demod_iq", true);
    if (pl.refused()) return fail(ctx, pl.code, "%s", pl.err.c_str());
    if (pairs->n_pairs == 0) return DPEMU_OK;
    // (between the planner's two steps: the table's scalars are refused before it, the pairs after)
    if (reinterpret_cast<uintptr_t>(iq_lo) % 16) return fail(ctx, DPEMU_E_INVALID, "iq_lo must be 16-byte aligned");
    if (describe_pairs(pl, cfg, pairs).refused()) return fail(ctx, pl.code, "%s", pl.err.c_str());
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, order_begin(ctx, s));
    HIPCHK(ctx, ctx->pairs.upload(pl.desc, s));   // the table changes rarely: uploaded only then
    DemodParams p{};
    p.summary = summary;
    p.events = reinterpret_cast<const uint4 *>(events);
    p.iq_drv = iq_drv; p.iq_lo = iq_lo;
    p.sin_lut = ctx->d_sin;
    p.pairs = ctx->pairs.as<uint32_t>();
    p.acc = reinterpret_cast<int2 *>(acc);
    p.result = reinterpret_cast<uint2 *>(result);
    p.n_pairs = pairs->n_pairs; p.n_lanes = pairs->n_lanes; p.event_cap = pairs->event_cap;
    p.meas_cap = pairs->meas_cap;
    p.n_samples_drv = pairs->n_samples_drv; p.n_samples_lo = pairs->n_samples_lo;
    set_readout(p, cfg);
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_demod_iq(p, s); }));
    HIPCHK(ctx, launch_readout_result(p.pairs, p.acc, p.result, p.n_pairs, p.ro_thr, s));   // outside the timed bracket: it holds the sweep kernel alone
    ctx->last_kernel = "demod_iq_kernel";
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

// The device half every feedline stage shares, for an accepted plan
// (stage_plan.h plan_feedlines): the pair table, the line table and the readout
// index on the device, and the launch of feedline_index_kernel; fills
// everything of `p` but the stage's own buffers.  `states` (the *_st calls;
// null: the draw) are the per-lane words the index takes the prepared states
// from.
static int feedline_prepare(dpemu_ctx *ctx, const FeedlinePlan &fl, const dpemu_config *cfg,
                            const dpemu_demod_pairs *pairs, const uint32_t *summary, const uint32_t *events,
                            const uint32_t *states, hipStream_t s, FeedlineParams &p)
{
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, order_begin(ctx, s));
    HIPCHK(ctx, ctx->pairs.upload(fl.desc, s));   // the table changes rarely: uploaded only then
    // the line table and the readout index (each waits for the stream only when it has to change)
    HIPCHK(ctx, ctx->lines.upload(fl.tab, s));
    HIPCHK(ctx, ctx->fl_index.reserve((size_t)fl.n_pairs * (FEEDLINE_RD_SLOTS + 1) * sizeof(uint2), s));
    const uint32_t *d_lines = ctx->lines.as<uint32_t>();
    p.summary = summary;
    p.events = reinterpret_cast<const uint4 *>(events);
    p.sin_lut = ctx->d_sin;
    p.pairs = ctx->pairs.as<uint32_t>();
    p.line_first = d_lines;
    p.member = d_lines + fl.member;
    p.line_of = d_lines + fl.line_of;
    p.rd = ctx->fl_index.as<uint2>();
    p.hdr = p.rd + (uint64_t)fl.n_pairs * FEEDLINE_RD_SLOTS;
    p.n_pairs = fl.n_pairs; p.n_lines = fl.n_lines; p.n_lanes = pairs->n_lanes; p.event_cap = pairs->event_cap;
    p.meas_cap = pairs->meas_cap;
    p.n_samples_drv = pairs->n_samples_drv; p.n_samples_lo = pairs->n_samples_lo;
    set_readout(p, cfg);
    p.states = states;                          // the *_st calls: hdr's state bits from the caller's words
    HIPCHK(ctx, launch_feedline_index(p, s));   // outside the timed bracket, as the DDS index
    return DPEMU_OK;
}

// the pointer arguments the two ADC stages share (res: the resonator stage's table, checked when `with_res`)
static int check_adc_ptrs(dpemu_ctx *ctx, const char *what, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                          const dpemu_feedlines *lines, bool with_res, const dpemu_resonators *res,
                          const uint32_t *summary, const uint32_t *events, const uint32_t *iq_drv, const uint32_t *adc)
{
    if (int rc = check_ptrs(ctx, what, {{cfg, "cfg"}, {pairs, "pairs"}, {lines, "lines"}, {res, with_res ? "res" : nullptr},
                                        {summary, "summary"}, {events, "events"}, {iq_drv, "iq_drv"}, {adc, "adc"}}))
        return rc;
    if (with_res && !res->coef) return fail(ctx, DPEMU_E_INVALID, "%s: res->coef is NULL", what);
    if (reinterpret_cast<uintptr_t>(adc) % 16) return fail(ctx, DPEMU_E_INVALID, "adc must be 16-byte aligned");
    return DPEMU_OK;
}

// dpemu_feedline_adc and, with `states`, dpemu_feedline_adc_st
static int feedline_adc_impl(dpemu_ctx *ctx, const char *what, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                             const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                             const uint32_t *iq_drv, uint32_t *adc, const uint32_t *states, void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_adc_ptrs(ctx, what, cfg, pairs, lines, false, nullptr, summary, events, iq_drv, adc)) return rc;
    const FeedlinePlan fl = plan_feedlines(cfg, pairs, lines, what, FEEDLINE_ADC);
    if (fl.refused()) return fail(ctx, fl.code, "%s", fl.err.c_str());
    hipStream_t s = (hipStream_t)stream;
    FeedlineParams p{};
    if (int rc = feedline_prepare(ctx, fl, cfg, pairs, summary, events, states, s, p)) return rc;
    p.iq_drv = iq_drv;
    p.adc = adc;
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_feedline_adc(p, s); }));
    ctx->last_kernel = "feedline_adc_kernel";
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

extern "C" int dpemu_feedline_adc(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                  const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                                  const uint32_t *iq_drv, uint32_t *adc, void *stream)
{
    return feedline_adc_impl(ctx, "dpemu_feedline_adc", cfg, pairs, lines, summary, events, iq_drv, adc, nullptr, stream);
}

extern "C" int dpemu_feedline_adc_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                     const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                                     const uint32_t *iq_drv, uint32_t *adc, const uint32_t *states, void *stream)
{
    return feedline_adc_impl(ctx, "dpemu_feedline_adc_st", cfg, pairs, lines, summary, events, iq_drv, adc, states, stream);
}

// dpemu_feedline_adc_res and, with `states`, dpemu_feedline_adc_res_st
static int feedline_res_impl(dpemu_ctx *ctx, const char *what, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                             const dpemu_feedlines *lines, const dpemu_resonators *res, const uint32_t *summary,
                             const uint32_t *events, const uint32_t *iq_drv, uint32_t *adc, const uint32_t *states,
                             void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_adc_ptrs(ctx, what, cfg, pairs, lines, true, res, summary, events, iq_drv, adc)) return rc;
    const FeedlinePlan fl = plan_feedlines(cfg, pairs, lines, what, FEEDLINE_ADC_RES);
    if (fl.refused()) return fail(ctx, fl.code, "%s", fl.err.c_str());
    const ResonatorPlan rp = plan_resonators(res, pairs->n_pairs);
    if (rp.refused()) return fail(ctx, rp.code, "%s", rp.err.c_str());
    hipStream_t s = (hipStream_t)stream;
    ResonatorParams q{};
    if (int rc = feedline_prepare(ctx, fl, cfg, pairs, summary, events, states, s, q.f)) return rc;
    q.wg_first = q.f.line_first + fl.wg_first;
    q.n_wgs = fl.n_wgs;
    // the coefficients on the device: uploaded only when they changed, as the pair and line tables
    HIPCHK(ctx, ctx->res.upload(rp.coef, s));
    q.f.iq_drv = iq_drv;
    q.f.adc = adc;
    q.coef = ctx->res.as<const int4>();
    q.adc_sigma = res->adc_sigma;
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_feedline_res(q, s); }));
    ctx->last_kernel = "feedline_res_kernel";
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

extern "C" int dpemu_feedline_adc_res(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                      const dpemu_feedlines *lines, const dpemu_resonators *res,
                                      const uint32_t *summary, const uint32_t *events, const uint32_t *iq_drv,
                                      uint32_t *adc, void *stream)
{
    return feedline_res_impl(ctx, "dpemu_feedline_adc_res", cfg, pairs, lines, res, summary, events, iq_drv, adc,
                             nullptr, stream);
}

extern "C" int dpemu_feedline_adc_res_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                         const dpemu_feedlines *lines, const dpemu_resonators *res,
                                         const uint32_t *summary, const uint32_t *events, const uint32_t *iq_drv,
                                         uint32_t *adc, const uint32_t *states, void *stream)
{
    return feedline_res_impl(ctx, "dpemu_feedline_adc_res_st", cfg, pairs, lines, res, summary, events, iq_drv, adc,
                             states, stream);
}

extern "C" int dpemu_demod_feedline(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                    const dpemu_feedlines *lines, const uint32_t *summary, const uint32_t *events,
                                    const uint32_t *adc, const uint32_t *iq_lo, int32_t *acc, uint32_t *result,
                                    void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_ptrs(ctx, "dpemu_demod_feedline", {{cfg, "cfg"}, {pairs, "pairs"}, {lines, "lines"},
                                                         {summary, "summary"}, {events, "events"}, {adc, "adc"},
                                                         {iq_lo, "iq_lo"}, {acc, "acc"}, {result, "result"}}))
        return rc;
    if (reinterpret_cast<uintptr_t>(adc) % 16) return fail(ctx, DPEMU_E_INVALID, "adc must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(iq_lo) % 16) return fail(ctx, DPEMU_E_INVALID, "iq_lo must be 16-byte aligned");
    const FeedlinePlan fl = plan_feedlines(cfg, pairs, lines, "dpemu_demod_feedline", FEEDLINE_DEMOD);
    if (fl.refused()) return fail(ctx, fl.code, "%s", fl.err.c_str());
    hipStream_t s = (hipStream_t)stream;
    FeedlineParams p{};
    if (int rc = feedline_prepare(ctx, fl, cfg, pairs, summary, events, nullptr, s, p)) return rc;
    p.adc = const_cast<uint32_t *>(adc);    // read only by this stage
    p.iq_lo = iq_lo;
    p.acc = reinterpret_cast<int2 *>(acc);
    p.result = reinterpret_cast<uint2 *>(result);
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_feedline_demod(p, s); }));
    HIPCHK(ctx, launch_readout_result(p.pairs, p.acc, p.result, p.n_pairs, p.ro_thr, s));   // outside the timed bracket: it holds the sweep kernel alone
    ctx->last_kernel = "feedline_demod_kernel";
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

// dpemu_feedline_traces and, with `states`, dpemu_feedline_traces_st
static int feedline_traces_impl(dpemu_ctx *ctx, const char *what, const dpemu_config *cfg,
                                const dpemu_demod_pairs *pairs, const dpemu_feedlines *lines,
                                const dpemu_trace_bins *bins, const uint32_t *summary, const uint32_t *events,
                                const uint32_t *adc, const uint32_t *iq_lo, int64_t *traces, const uint32_t *states,
                                void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_ptrs(ctx, what, {{cfg, "cfg"}, {pairs, "pairs"}, {lines, "lines"}, {bins, "bins"}, {summary, "summary"},
                                        {events, "events"}, {adc, "adc"}, {iq_lo, "iq_lo"}, {traces, "traces"}}))
        return rc;
    if (reinterpret_cast<uintptr_t>(adc) % 16) return fail(ctx, DPEMU_E_INVALID, "adc must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(iq_lo) % 16) return fail(ctx, DPEMU_E_INVALID, "iq_lo must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(traces) % 8) return fail(ctx, DPEMU_E_INVALID, "traces must be 8-byte aligned");
    const FeedlinePlan fl = plan_trace_feedlines(cfg, pairs, lines, bins, what);
    if (fl.refused()) return fail(ctx, fl.code, "%s", fl.err.c_str());
    hipStream_t s = (hipStream_t)stream;
    TraceParams q{};
    if (int rc = feedline_prepare(ctx, fl, cfg, pairs, summary, events, states, s, q.f)) return rc;
    if (!ctx->trace_wgs_per_cu) {
        ctx->trace_wgs_per_cu = trace_wgs_per_cu();
        if (!ctx->trace_wgs_per_cu) ctx->trace_wgs_per_cu = 4;
    }
    const uint32_t C = cfg->cores_per_shot, S = bins->by_slot ? pairs->meas_cap : 1u;
    const TracePlan pl = plan_traces(pairs->core, pairs->spc_lo, pairs->n_pairs, pairs->n_samples_lo, cfg->ro_cpw,
                                     bins->n_bins, bins->bin_clocks, S, ctx->trace_wgs_per_cu, ctx->n_cu);
    HIPCHK(ctx, ctx->trace_tab.upload(pl.tab, s));  // follows the pair table: uploaded only when that changed
    // traces is assigned: zero, then the kernel's atomics add
    HIPCHK(ctx, hipMemsetAsync(traces, 0, (size_t)S * C * 2 * bins->n_bins * DPEMU_TRACE_WORDS * sizeof(int64_t), s));
    q.f.adc = const_cast<uint32_t *>(adc);  // read only by this stage
    q.f.iq_lo = iq_lo;
    q.chunks = ctx->trace_tab.as<const uint4>();
    q.perm = ctx->trace_tab.as<const uint32_t>() + (size_t)pl.n_chunks * TRACE_CHUNK_WORDS;
    q.traces = reinterpret_cast<unsigned long long *>(traces);
    q.n_chunks = pl.n_chunks; q.tiles = pl.tiles;
    q.n_bins = bins->n_bins; q.bin_clocks = bins->bin_clocks; q.by_slot = bins->by_slot; q.C = C;
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_feedline_trace(q, s); }));
    ctx->last_kernel = "feedline_trace_kernel";
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

extern "C" int dpemu_feedline_traces(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                     const dpemu_feedlines *lines, const dpemu_trace_bins *bins,
                                     const uint32_t *summary, const uint32_t *events, const uint32_t *adc,
                                     const uint32_t *iq_lo, int64_t *traces, void *stream)
{
    return feedline_traces_impl(ctx, "dpemu_feedline_traces", cfg, pairs, lines, bins, summary, events, adc, iq_lo,
                                traces, nullptr, stream);
}

extern "C" int dpemu_feedline_traces_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_demod_pairs *pairs,
                                        const dpemu_feedlines *lines, const dpemu_trace_bins *bins,
                                        const uint32_t *summary, const uint32_t *events, const uint32_t *adc,
                                        const uint32_t *iq_lo, int64_t *traces, const uint32_t *states, void *stream)
{
    return feedline_traces_impl(ctx, "dpemu_feedline_traces_st", cfg, pairs, lines, bins, summary, events, adc, iq_lo,
                                traces, states, stream);
}

// dpemu_iq_stats and, with `states`, dpemu_iq_stats_st
static int iq_stats_impl(dpemu_ctx *ctx, const char *what, const dpemu_config *cfg, const dpemu_iq_columns *cols,
                         const int32_t *acc, const uint32_t *counts, int64_t *stats, uint32_t *bits,
                         const uint32_t *states, void *stream)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_ptrs(ctx, what, {{cfg, "cfg"}, {cols, "cols"}, {stats, "stats"}})) return rc;
    if (cols->n_cols)                   // (nothing is read from acc / counts of no columns: they may be NULL)
        if (int rc = check_ptrs(ctx, what, {{acc, "acc"}, {counts, "counts"}})) return rc;
    const IqColumnsPlan pl = plan_iq_columns(cfg, cols);
    if (pl.refused()) return fail(ctx, pl.code, "%s", pl.err.c_str());
    const uint32_t C = cfg->cores_per_shot, n = cols->n_cols;
    const bool expl = pl.expl;
    // (after the planner: a refused column table is named before a misaligned buffer)
    if (reinterpret_cast<uintptr_t>(acc) % 8 || reinterpret_cast<uintptr_t>(stats) % 8)
        return fail(ctx, DPEMU_E_INVALID, "acc and stats must be 8-byte aligned");
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, order_begin(ctx, s));
    // stats is assigned: zero, then the kernel's atomics add
    const uint64_t S = cols->by_slot ? cols->meas_cap : 1u;
    HIPCHK(ctx, hipMemsetAsync(stats, 0, S * C * 2 * DPEMU_IQ_STAT_WORDS * sizeof(int64_t), s));
    if (n == 0) {
        HIPCHK(ctx, order_end(ctx, s));
        return DPEMU_OK;
    }
    IqStatsParams p{};
    if (expl) {                             // the column table ([n] u64 shots, [n] u32 cores) changes rarely
        HIPCHK(ctx, ctx->iqcols.upload(pl.tab, s));
        p.x_shot = ctx->iqcols.as<const uint64_t>();
        p.x_core = reinterpret_cast<const uint32_t *>(ctx->iqcols.as<const uint8_t>() + 8ull * n);
    }
    p.acc = reinterpret_cast<const int2 *>(acc);
    p.counts = counts;
    p.stats = reinterpret_cast<unsigned long long *>(stats);
    p.bits = bits;
    p.seed = cfg->seed; p.shot_begin = cols->shot_begin;
    p.n_cols = n; p.meas_cap = cols->meas_cap; p.by_slot = cols->by_slot; p.count_stride = cols->count_stride;
    p.C = C;
    while ((1u << p.log2C) < C) p.log2C++;
    p.shot_major = cfg->lane_order == DPEMU_LANES_SHOT_MAJOR;
    p.n_shots = expl ? 1u : n / C;
    fast_div_init(p.n_shots, p.ns_div);
    p.red_c = (!expl && p.shot_major) ? C : 1u;
    memcpy(p.p1, pl.p1, sizeof p.p1);
    memcpy(p.axis, pl.axis, sizeof p.axis);
    memcpy(p.thr, pl.thr, sizeof p.thr);
    p.states = states;
    if (!ctx->iq_wgs_per_cu) {
        ctx->iq_wgs_per_cu = iq_stats_wgs_per_cu();
        if (!ctx->iq_wgs_per_cu) ctx->iq_wgs_per_cu = 4;
    }
    const uint32_t gx = iq_stats_grid(n, C, S, ctx->iq_wgs_per_cu, ctx->n_cu);
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_iq_stats(p, gx, s); }));
    ctx->last_kernel = "iq_stats_kernel";
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

extern "C" int dpemu_iq_stats(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_iq_columns *cols,
                              const int32_t *acc, const uint32_t *counts, int64_t *stats, uint32_t *bits,
                              void *stream)
{
    return iq_stats_impl(ctx, "dpemu_iq_stats", cfg, cols, acc, counts, stats, bits, nullptr, stream);
}

extern "C" int dpemu_iq_stats_st(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_iq_columns *cols,
                                 const int32_t *acc, const uint32_t *counts, int64_t *stats, uint32_t *bits,
                                 const uint32_t *states, void *stream)
{
    return iq_stats_impl(ctx, "dpemu_iq_stats_st", cfg, cols, acc, counts, stats, bits, states, stream);
}

extern "C" int dpemu_qsim_phase_lut(int32_t *out)
{
    if (!out) return DPEMU_E_INVALID;
    qsim_phase_lut(out);
    return DPEMU_OK;
}

// dpemu_qsim and, with `meas`, dpemu_qsim_meas (`states`: its per-lane output); with `decay`, dpemu_qsim_decay
// of either (`dec`: its tables, `counts`: its nullable output)
static int qsim_impl(dpemu_ctx *ctx, const char *what, bool meas, const dpemu_config *cfg, const dpemu_qsim_args *qs,
                     const uint32_t *summary, const uint32_t *events, uint64_t *pops, uint32_t *result,
                     uint32_t *states, void *stream, bool decay = false, const dpemu_qsim_decay_args *dec = nullptr,
                     uint32_t *counts = nullptr)
{
    if (!ctx) return DPEMU_E_INVALID;
    if (int rc = check_ptrs(ctx, what, {{cfg, "cfg"}, {qs, "qs"}, {summary, "summary"}, {events, "events"},
                                        {pops, "pops"}, {result, "result"}, {states, meas ? "states" : nullptr}}))
        return rc;
    if (reinterpret_cast<uintptr_t>(pops) % 8 || reinterpret_cast<uintptr_t>(result) % 16 ||
        reinterpret_cast<uintptr_t>(events) % 16)
        return fail(ctx, DPEMU_E_INVALID, "%s: pops must be 8-byte, events and result 16-byte aligned", what);
    const QsimPlan pl = plan_qsim(cfg, qs, meas);
    if (!pl.err.empty()) return fail(ctx, DPEMU_E_INVALID, "%s: %s", what, pl.err.c_str());
    QsimDecayPlan dpl;
    if (decay) {
        dpl = plan_qsim_decay(cfg, dec);
        if (!dpl.err.empty()) return fail(ctx, DPEMU_E_INVALID, "%s: %s", what, dpl.err.c_str());
        if (reinterpret_cast<uintptr_t>(counts) % 16)
            return fail(ctx, DPEMU_E_INVALID, "%s: counts must be 16-byte aligned", what);
    }
    if (qs->n_shots == 0) return DPEMU_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(ctx, order_begin(ctx, s));
    HIPCHK(ctx, ctx->qsim_tab.upload(pl.tab, s));       // changes with the gate set, not from call to call
    if (decay) HIPCHK(ctx, ctx->qsim_decay_tab.upload(dpl.tab, s));
    QsimParams p{};
    p.summary = summary;
    p.events = reinterpret_cast<const uint4 *>(events);
    p.tab = ctx->qsim_tab.as<const uint32_t>();
    p.pops = reinterpret_cast<unsigned long long *>(pops);
    p.result = reinterpret_cast<uint4 *>(result);
    p.seed = cfg->seed; p.shot_begin = qs->shot_begin;
    p.n_regs = qs->n_regs; p.n_shots = (uint32_t)qs->n_shots; p.n_rows = (uint32_t)(qs->n_regs * qs->n_shots);
    p.n_lanes = qs->n_lanes; p.event_cap = qs->event_cap; p.C = cfg->cores_per_shot;
    p.shot_major = cfg->lane_order == DPEMU_LANES_SHOT_MAJOR; p.drv_elem = qs->drv_elem;
    fast_div_init(p.n_shots, p.ns_div);
    p.off_reg = pl.off_reg; p.off_slot = pl.off_slot; p.off_det = pl.off_det; p.off_dict = pl.off_dict;
    p.lds_bytes = pl.lds_bytes;
    if (meas) {                                 // states is assigned: zero (lanes of no register stay so), then the rows store
        p.meas = 1u; p.meas_elem = cfg->meas_elem; p.states = states;
        HIPCHK(ctx, hipMemsetAsync(states, 0, (size_t)qs->n_lanes * sizeof(uint32_t), s));
    }
    if (decay) {
        p.decay = ctx->qsim_decay_tab.as<const uint32_t>(); p.counts = counts; p.t_final = dec->t_final;
    }
    HIPCHK(ctx, timed(ctx, s, [&] { return launch_qsim(p, s); }));
    ctx->last_kernel = decay ? (meas ? "qsim_kernel<meas,decay>" : "qsim_kernel<decay>")
                             : (meas ? "qsim_kernel<meas>" : "qsim_kernel");
    HIPCHK(ctx, order_end(ctx, s));
    return DPEMU_OK;
}

extern "C" int dpemu_qsim(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_qsim_args *qs, const uint32_t *summary,
                          const uint32_t *events, uint64_t *pops, uint32_t *result, void *stream)
{
    return qsim_impl(ctx, "dpemu_qsim", false, cfg, qs, summary, events, pops, result, nullptr, stream);
}

extern "C" int dpemu_qsim_meas(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_qsim_args *qs,
                               const uint32_t *summary, const uint32_t *events, uint64_t *pops, uint32_t *result,
                               uint32_t *states, void *stream)
{
    return qsim_impl(ctx, "dpemu_qsim_meas", true, cfg, qs, summary, events, pops, result, states, stream);
}

extern "C" int dpemu_qsim_decay(dpemu_ctx *ctx, const dpemu_config *cfg, const dpemu_qsim_args *qs,
                                const dpemu_qsim_decay_args *dec, const uint32_t *summary, const uint32_t *events,
                                uint64_t *pops, uint32_t *result, uint32_t *states, uint32_t *counts, void *stream)
{
    return qsim_impl(ctx, "dpemu_qsim_decay", states != nullptr, cfg, qs, summary, events, pops, result, states, stream,
                     true, dec, counts);
}
