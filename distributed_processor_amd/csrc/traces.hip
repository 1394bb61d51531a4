// traces.hip -- averaged readout traces of the shared feedline (gfx950).
//
// Spec: include/dpemu.h dpemu_feedline_traces, DESIGN.md §2 "Averaged traces
// and matched filter" and §4.12; CPU restatement tests/traces_ref.py
// (bit-exact).  One streaming pass over the windows of every kept readout: the
// line's ADC row and the pair's LO row, spc_lo * 4 B of each per window clock
// (feedline_demod_kernel's stream; the window: readout_rules.h ro_window), reduced to a [S][C][2][n_bins][4] int64
// table.  Integer arithmetic and integer atomics only: the result does not
// depend on the grid or on the order anything arrives in.
//
// feedline_trace_kernel, grid (sample tiles, chunks, S): S = 1, or with by_slot
// one grid layer per slot.  A chunk is a run of pairs of one core and one
// spc_lo (the host sorts the pair table by both: launch_plan.h plan_traces),
// so the class rows and the bin of every sample are fixed for the workgroup.
// Thread r of the tile row owns the 4 LO samples 4 r .. 4 r + 3 COUNTED FROM
// THE WINDOW START of whatever readout it is at: a bin is a distance from the
// strobe, so the thread's four bins never change, and consecutive threads read
// consecutive 16-byte groups.  The workgroup first stages its pairs' windows
// {ADC row, LO row, first sample, length, state} in LDS, one thread per pair,
// compacted by a block scan: the chain of dependent loads behind a window
// (sorted index -> pair -> readout record) is then paid once for all pairs at a
// time, not once per window of the sweep, and the sweep loads the next
// window's rows while it sums this one's.  Pair, readout and prepared state
// are wave-uniform: the state picks one of two register sets by a uniform
// branch (a dynamically indexed register array would live in scratch,
// iq_stats.hip).
// A window start t_lo spc_lo that is no multiple of 4 (spc_lo 1, 2) takes the
// same samples in 4-byte loads -- a uniform branch too.  At the end a thread
// merges those of its four samples that share a bin and adds the nonzero
// words to `traces` with 64-bit global atomics; when a bin is longer than 4
// samples several threads add to it.  The host zeroes `traces` before the
// launch and sizes the chunks so that this traffic stays small beside the
// stream and the grid within what the device holds at once.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"
#include "q15.h"

namespace dpemu {

// one prepared state's sums of a thread, per owned sample
struct TrSet {
    uint32_t n0[4], n1[4];                              // readouts that open a bin at the sample / samples
    long long si[4], sq[4];
};

__device__ __forceinline__ void tr_zero(TrSet &a)
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        a.n0[s] = a.n1[s] = 0;
        a.si[s] = a.sq[s] = 0;
    }
}

// the first `rem` of the thread's 4 samples are inside the window (0: the thread adds nothing)
__device__ __forceinline__ void tr_add(TrSet &a, const u32x4 aw, const u32x4 lw, uint32_t rem, const uint32_t opens[4])
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t ok = (uint32_t)s < rem ? 1u : 0u;
        const int2 P = mix_conj_m1(aw[s], ok ? lw[s] : 0u);   // {P_I - 1, P_Q}; a masked sample gives {-1, 0}
        a.si[s] += (long long)P.x + 1;
        a.sq[s] += P.y;
        a.n1[s] += ok;
        a.n0[s] += ok & opens[s];
    }
}

// samples of one bin are neighbours: carry a sample's sums into the next while the bin stays, add at its last
__device__ __forceinline__ void tr_flush(TrSet &a, const uint32_t bin[4], unsigned long long *row, uint32_t n_bins)
{
#pragma unroll
    for (int s = 0; s < 4; s++) {
        if (s < 3 && bin[s] == bin[s < 3 ? s + 1 : s]) {
            a.n0[s < 3 ? s + 1 : s] += a.n0[s];
            a.n1[s < 3 ? s + 1 : s] += a.n1[s];
            a.si[s < 3 ? s + 1 : s] += a.si[s];
            a.sq[s < 3 ? s + 1 : s] += a.sq[s];
        } else if (a.n1[s] && bin[s] < n_bins) {
            unsigned long long *w = row + (uint64_t)bin[s] * DPEMU_TRACE_WORDS;
            if (a.n0[s]) atomicAdd(&w[0], (unsigned long long)a.n0[s]);
            atomicAdd(&w[1], (unsigned long long)a.n1[s]);
            if (a.si[s]) atomicAdd(&w[2], (unsigned long long)a.si[s]);
            if (a.sq[s]) atomicAdd(&w[3], (unsigned long long)a.sq[s]);
        }
    }
}

// the first rem of the thread's 4 samples of a staged window, from both rows (zeros for a thread past the window)
__device__ __forceinline__ void tr_fetch(const FeedlineParams &p, const uint4 *s_item, uint32_t i, uint32_t i0,
                                         u32x4 &aw, u32x4 &lw, uint32_t &rem, uint32_t &state)
{
    const uint4 it = s_item[i];                         // one address for the whole wave
    const uint32_t *__restrict__ adc_row = p.adc + (uint64_t)__builtin_amdgcn_readfirstlane(it.x) * p.n_samples_lo;
    const uint32_t *__restrict__ lo_row = p.iq_lo + (uint64_t)__builtin_amdgcn_readfirstlane(it.y) * p.n_samples_lo;
    const uint32_t j0 = __builtin_amdgcn_readfirstlane(it.z), w = __builtin_amdgcn_readfirstlane(it.w);
    const uint32_t len = w & 0x7FFFFFFFu;
    state = w >> 31;
    rem = len > i0 ? len - i0 : 0u;
    aw = lw = u32x4{0u, 0u, 0u, 0u};
    if ((j0 & 3u) == 0u) {                              // (uniform) n_samples_lo is a multiple of 4: the whole group is inside
        if (rem) {
            aw = *reinterpret_cast<const u32x4 *>(adc_row + j0 + i0);
            lw = *reinterpret_cast<const u32x4 *>(lo_row + j0 + i0);
        }
    } else {
#pragma unroll
        for (int s = 0; s < 4; s++)
            if ((uint32_t)s < rem) {
                aw[s] = adc_row[j0 + i0 + s];
                lw[s] = lo_row[j0 + i0 + s];
            }
    }
}

__global__ void __launch_bounds__(BLOCK) feedline_trace_kernel(const TraceParams q)
{
    __shared__ uint4 s_item[TRACE_ITEMS];               // staged windows {ADC row, LO row, j0, len | state << 31}
    __shared__ uint32_t s_tmp[BLOCK / 64];
    const FeedlineParams &p = q.f;
    const uint32_t tid = threadIdx.x;
    const uint4 ch = q.chunks[blockIdx.y];
    const uint32_t core = __builtin_amdgcn_readfirstlane(ch.x), sh_lo = __builtin_amdgcn_readfirstlane(ch.y);
    const uint32_t k0 = __builtin_amdgcn_readfirstlane(ch.z), k1 = __builtin_amdgcn_readfirstlane(ch.w);
    const uint32_t m0 = q.by_slot ? blockIdx.z : 0u, m1 = q.by_slot ? m0 + 1u : p.meas_cap;

    // the thread's 4 samples, counted from a window's start: their bins, and whether a sample opens its bin
    const uint32_t i0 = 4u * (blockIdx.x * BLOCK + tid);    // < 2^21: the host bounds the tiles
    uint32_t bin[4], opens[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t i = i0 + s, clk = i >> sh_lo;
        bin[s] = clk / q.bin_clocks;
        opens[s] = ((i & ((1u << sh_lo) - 1u)) == 0u && clk == bin[s] * q.bin_clocks) ? 1u : 0u;
    }

    TrSet a0, a1;                                       // prepared state 0 / 1
    tr_zero(a0);
    tr_zero(a1);
    // the chunk's pairs in runs whose readouts fit the staging table (>= 32 pairs: meas_cap <= 32)
    const uint32_t run = min(TRACE_ITEMS / (m1 - m0), BLOCK);
    for (uint32_t kb = k0; kb < k1; kb += run) {
        // ---- stage: thread t lists the windows of pair kb + t, compacted by a scan.  Every dependent
        // load of the pair's metadata happens here, once and for all pairs at a time; the sweep
        // below waits for nothing but its two row loads ----
        const uint32_t k = kb + tid;
        uint32_t pr = 0, count = 0, bits = 0, lo_r = 0, adc_r = 0, valid = 0;
        if (tid < run && k < k1) {
            pr = q.perm[k];
            const uint2 h = p.hdr[pr];
            count = min(h.x, m1);
            bits = h.y;
            lo_r = p.pairs[DEMOD_PAIR_WORDS * pr + PAIR_LO_ROW];
            adc_r = p.line_of[pr];
        }
        uint4 first = make_uint4(0u, 0u, 0u, 0u);       // (most pairs have one window: kept from the first pass)
        for (uint32_t m = m0; m < count; m++) {
            const uint2 rd = p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + m];
            const RoWindow w = ro_window(rd.x, rd.y, sh_lo, p.ro_cpw, p.n_samples_lo);
            if (w.j0 >= w.j1) continue;                 // nothing of the window is inside the rows
            if (!valid) first = make_uint4(adc_r, lo_r, w.j0, (w.j1 - w.j0) | (((bits >> m) & 1u) << 31));
            valid |= 1u << (m - m0);
        }
        uint32_t total;
        uint32_t at = block_exclusive_scan((uint32_t)__popc(valid), s_tmp, &total);
        if (valid) s_item[at++] = first;
        valid &= valid - 1u;
        while (valid) {                                 // the rarer further windows: their records again
            const uint32_t m = m0 + (uint32_t)__ffs(valid) - 1u;
            valid &= valid - 1u;
            const uint2 rd = p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + m];
            const RoWindow w = ro_window(rd.x, rd.y, sh_lo, p.ro_cpw, p.n_samples_lo);
            s_item[at++] = make_uint4(adc_r, lo_r, w.j0, (w.j1 - w.j0) | (((bits >> m) & 1u) << 31));
        }
        __syncthreads();

        // ---- sweep: the next window's rows are in flight while this one's are summed ----
        u32x4 aw = {0u, 0u, 0u, 0u}, lw = {0u, 0u, 0u, 0u};
        uint32_t rem = 0, state = 0;
        if (total) tr_fetch(p, s_item, 0, i0, aw, lw, rem, state);
        for (uint32_t i = 0; i < total; i++) {
            u32x4 aw2 = {0u, 0u, 0u, 0u}, lw2 = {0u, 0u, 0u, 0u};
            uint32_t rem2 = 0, state2 = 0;
            if (i + 1u < total) tr_fetch(p, s_item, i + 1u, i0, aw2, lw2, rem2, state2);
            if (state)                                  // (uniform) the readout's prepared state
                tr_add(a1, aw, lw, rem, opens);
            else
                tr_add(a0, aw, lw, rem, opens);
            aw = aw2; lw = lw2; rem = rem2; state = state2;
        }
        __syncthreads();                                // the table is rewritten by the next run
    }

    // ---- the thread's sums -> traces[slot][core][state] ----
    const uint64_t row_words = (uint64_t)q.n_bins * DPEMU_TRACE_WORDS;
    unsigned long long *out = q.traces + ((uint64_t)(q.by_slot ? blockIdx.z : 0u) * q.C + core) * 2u * row_words;
    tr_flush(a0, bin, out, q.n_bins);
    tr_flush(a1, bin, out + row_words, q.n_bins);
}

// workgroups of feedline_trace_kernel a compute unit holds at once; 0 when the runtime cannot say
uint32_t trace_wgs_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, feedline_trace_kernel, BLOCK, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n > 0 ? (uint32_t)n : 0u;
}

hipError_t launch_feedline_trace(const TraceParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(feedline_trace_kernel, dim3(p.tiles, p.n_chunks, p.by_slot ? p.f.meas_cap : 1u), dim3(BLOCK), 0,
                       stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
