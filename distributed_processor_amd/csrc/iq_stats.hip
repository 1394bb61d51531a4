// iq_stats.hip -- readout IQ statistics of an accumulator buffer (gfx950).
//
// Spec: include/dpemu.h dpemu_iq_stats, DESIGN.md §2 "Readout statistics" and
// §4.9; CPU restatement tests/iq_stats_ref.py (bit-exact).  One streaming pass
// over acc [meas_cap][n_cols][2] (slot-major: consecutive columns are
// consecutive 8-byte loads), 8 B per readout in, a [S][C][2][16] int64 table
// out.  Integer arithmetic and integer atomics only: the result does not
// depend on the grid or on the order anything arrives in.
//
// iq_stats_kernel, grid (gx, S): S = 1, or with by_slot one grid row per slot.
// A thread takes columns gx * BLOCK apart.  Per readout it redraws the prepared
// state (lane.h philox3 and readout_rules.h ro_state, the draw of meas_bit /
// demod_readout / demod_iq.hip; dpemu_iq_stats_st: bit m of the column's
// `states` word in its place), re-discriminates {I, Q} (demod_decide) and adds the 13 words of the readout to two register
// sets: every readout's, and by select (0 for state 0) state 1's -- state 0 is
// their difference; a dynamically indexed register array would live in
// scratch.  The sets belong to one core: when a thread's
// next column is another core's (core-major lanes, explicit columns) it first
// adds them to the workgroup's table in LDS.  At the end a wave whose lanes
// hold `red_c` cores in the pattern lane & (red_c - 1) -- shot-major lanes,
// C <= 64, or one core for the whole wave -- reduces by __shfl_xor (offsets 32
// down to red_c) and red_c lanes add to LDS; any other wave (one that
// straddles a core boundary, explicit cores) adds lane by lane.  The
// workgroup then adds the table's nonzero words to `stats` with 64-bit global
// atomics; the host caps the grid at the workgroups the device holds at once
// and at a size where this traffic stays small beside the stream (launch_plan.h),
// and zeroes `stats` before the launch.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"

namespace dpemu {

constexpr int IQ_SUMS = 11;                             // words 2..12 (int64); words 0, 1 are counters

// one state's sums of a thread
struct IqSet {
    uint32_t n, n1;
    long long s[IQ_SUMS];
};

__device__ __forceinline__ void iq_zero(IqSet &a)
{
    a.n = a.n1 = 0;
#pragma unroll
    for (int k = 0; k < IQ_SUMS; k++) a.s[k] = 0;
}

__device__ __forceinline__ IqSet iq_sub(const IqSet &a, const IqSet &b)
{
    IqSet d;
    d.n = a.n - b.n;
    d.n1 = a.n1 - b.n1;
#pragma unroll
    for (int k = 0; k < IQ_SUMS; k++) d.s[k] = a.s[k] - b.s[k];
    return d;
}

// add a set to the workgroup table's class row (16 words) in LDS
__device__ __forceinline__ void iq_to_lds(unsigned long long *row, const IqSet &a)
{
    if (!a.n) return;                                   // every word of a readout-less set is zero
    atomicAdd(&row[0], (unsigned long long)a.n);
    if (a.n1) atomicAdd(&row[1], (unsigned long long)a.n1);
#pragma unroll
    for (int k = 0; k < IQ_SUMS; k++)
        if (a.s[k]) atomicAdd(&row[2 + k], (unsigned long long)a.s[k]);
}

__device__ __forceinline__ void iq_wave_reduce(IqSet &a, uint32_t red_c)
{
    for (uint32_t o = 32; o >= red_c; o >>= 1) {
        a.n += __shfl_xor(a.n, o, 64);
        a.n1 += __shfl_xor(a.n1, o, 64);
#pragma unroll
        for (int k = 0; k < IQ_SUMS; k++) a.s[k] += __shfl_xor(a.s[k], o, 64);
    }
}

__global__ void __launch_bounds__(BLOCK) iq_stats_kernel(const IqStatsParams p)
{
    __shared__ unsigned long long s_tab[DPEMU_MAX_CORES * 2 * DPEMU_IQ_STAT_WORDS];
    __shared__ uint32_t s_p1[DPEMU_MAX_CORES], s_axis[DPEMU_MAX_CORES];
    __shared__ int32_t s_thr[DPEMU_MAX_CORES];
    const uint32_t tid = threadIdx.x, wl = tid & 63u;
    const uint32_t rows = p.C * 2u * DPEMU_IQ_STAT_WORDS;
    for (uint32_t i = tid; i < rows; i += BLOCK) s_tab[i] = 0ull;
    if (tid < DPEMU_MAX_CORES) {
        s_p1[tid] = p.p1[tid];
        s_axis[tid] = p.axis[tid];
        s_thr[tid] = p.thr[tid];
    }
    __syncthreads();

    // slots of this grid row: all (one class set), or the row's own (by_slot)
    const uint32_t m0 = p.by_slot ? blockIdx.y : 0u, m1 = p.by_slot ? m0 + 1u : p.meas_cap;
    // bits[col] holds every slot's outcome: with by_slot grid row 0 sweeps them all
    const bool do_bits = p.bits && blockIdx.y == 0u;
    const uint32_t b1 = do_bits ? p.meas_cap : m1;      // slots [m0, b1) are discriminated, [m0, m1) counted

    IqSet at, a1;                                       // every readout / those of prepared state 1, core `cur`
    iq_zero(at);
    iq_zero(a1);
    uint32_t cur = ~0u;                                 // no column yet
    const uint32_t stride = gridDim.x * BLOCK;
    for (uint32_t col = blockIdx.x * BLOCK + tid; col < p.n_cols; col += stride) {
        uint32_t core;
        uint64_t shot;
        if (p.x_core) {
            core = p.x_core[col];
            shot = p.x_shot[col];
        } else if (p.shot_major) {
            core = col & (p.C - 1u);
            shot = p.shot_begin + (col >> p.log2C);
        } else {
            core = fast_div(col, p.ns_div);
            shot = p.shot_begin + (col - core * p.n_shots);
        }
        if (core != cur) {                              // the sets are one core's
            if (cur != ~0u) {
                iq_to_lds(&s_tab[(cur * 2u) * DPEMU_IQ_STAT_WORDS], iq_sub(at, a1));
                iq_to_lds(&s_tab[(cur * 2u + 1u) * DPEMU_IQ_STAT_WORDS], a1);
                iq_zero(at);
                iq_zero(a1);
            }
            cur = core;
        }
        const uint32_t count = min(p.counts[(uint64_t)col * p.count_stride], p.meas_cap);
        const uint32_t thr_p1 = s_p1[core], ax = s_axis[core];
        const int32_t thr = s_thr[core];
        const uint32_t st_word = p.states ? p.states[col] : 0u;
        uint32_t bits = 0;
        for (uint32_t m = m0; m < b1; m++) {
            if (m >= count) break;
            const int2 v = p.acc[(uint64_t)m * p.n_cols + col];
            const uint32_t o = demod_decide(v.x, v.y, ax, thr);
            bits |= o << m;
            if (m >= m1) continue;                      // (by_slot, row 0) the other rows count this slot
            bool st;
            if (p.states) {                             // dpemu_iq_stats_st: the column's injected bits
                st = (st_word >> m) & 1u;
            } else {
                const uint3 r = philox3(p.seed, shot, core, m);
                st = ro_state(r.x, thr_p1);
            }
            // X = 65536 a + b: a in [-2^15, 2^15), b in [0, 2^16)
            const int32_t ai = v.x >> 16, aq = v.y >> 16;
            const int32_t bi = v.x & 0xFFFF, bq = v.y & 0xFFFF;
            long long t[IQ_SUMS];
            t[0] = v.x;
            t[1] = v.y;
            t[2] = ai * ai;                             // <= 2^30
            t[3] = ai * bi;                             // |.| < 2^31
            t[4] = (long long)((uint32_t)bi * (uint32_t)bi);
            t[5] = aq * aq;
            t[6] = aq * bq;
            t[7] = (long long)((uint32_t)bq * (uint32_t)bq);
            t[8] = ai * aq;
            t[9] = (long long)(ai * bq) + (long long)(bi * aq);
            t[10] = (long long)((uint32_t)bi * (uint32_t)bq);
            at.n += 1u;
            a1.n += st ? 1u : 0u;
            at.n1 += o;
            a1.n1 += st ? o : 0u;
#pragma unroll
            for (int k = 0; k < IQ_SUMS; k++) {
                at.s[k] += t[k];
                a1.s[k] += st ? t[k] : 0ll;
            }
        }
        if (do_bits) p.bits[col] = bits;
    }

    // ---- the thread's sets -> the workgroup table ----
    // lanes 0..k of a wave have columns (they are consecutive), so lane
    // wl & (red_c - 1) has one whenever lane wl does
    const uint32_t ref = __shfl(cur, wl & (p.red_c - 1u), 64);
    if (__all(cur == ~0u || cur == ref)) {
        iq_wave_reduce(at, p.red_c);
        iq_wave_reduce(a1, p.red_c);
        if (wl >= p.red_c) cur = ~0u;
    }
    if (cur != ~0u) {
        iq_to_lds(&s_tab[(cur * 2u) * DPEMU_IQ_STAT_WORDS], iq_sub(at, a1));
        iq_to_lds(&s_tab[(cur * 2u + 1u) * DPEMU_IQ_STAT_WORDS], a1);
    }
    __syncthreads();

    // ---- the workgroup table -> stats[slot row] ----
    unsigned long long *out = p.stats + (uint64_t)blockIdx.y * rows;
    for (uint32_t i = tid; i < rows; i += BLOCK) {
        const unsigned long long v = s_tab[i];
        if (v) atomicAdd(&out[i], v);
    }
}

// workgroups of iq_stats_kernel a compute unit holds at once (its registers and
// LDS decide); 0 when the runtime cannot say
uint32_t iq_stats_wgs_per_cu()
{
    int n = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, iq_stats_kernel, BLOCK, 0) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n > 0 ? (uint32_t)n : 0u;
}

hipError_t launch_iq_stats(const IqStatsParams &p, uint32_t gx, hipStream_t stream)
{
    hipLaunchKernelGGL(iq_stats_kernel, dim3(gx, p.by_slot ? p.meas_cap : 1u), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
