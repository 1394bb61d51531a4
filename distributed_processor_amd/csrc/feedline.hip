// feedline.hip -- multiplexed readout: the shared-feedline ADC trace and its
// demodulation (gfx950).
//
// Spec: include/dpemu.h dpemu_feedline_adc / dpemu_demod_feedline, DESIGN.md §2
// "Multiplexed readout" and §4.10; CPU restatement tests/feedline_ref.py
// (bit-exact).  A feedline sums the rotated, scaled drive returns of up to
// DPEMU_FEEDLINE_MAX pairs into one ADC row; every member's LO then
// demodulates that row.
//
// Launches:
//   * feedline_index_kernel, one workgroup per pair (both calls): the pair's
//     kept readout strobes {t_lo, env word} in event order, their count and
//     the prepared state of each, found once (readout_dev.h scan_readouts).
//     Neither hot kernel reads an event record.
//   * feedline_adc_kernel, grid (sample tiles, lines): the workgroup stages
//     its members' readout times, state bits and drive rows in LDS; a lane
//     takes 4 consecutive LO samples, gathers each member's 4 drive samples
//     (one index for all members: a line has one rate pair), picks the
//     member's state at the sample's clock, rotates and scales on the packed
//     int16 helpers, sums in int32, saturates and stores 16 bytes.
//   * feedline_demod_kernel, grid (meas_cap, pairs), one workgroup per
//     readout: two contiguous rows (the line's ADC row and the pair's LO row)
//     in 16-B loads, P = adc conj(lo) on v_dot2_i32_i16, int64 sums, reduced
//     by readout_dev.h block_sum2; thread 0 scales, adds the noise and stores.
//     demod_iq.hip's readout_result_kernel then packs the outcome bits.
// Integer sums throughout: the result is the same for every grid.  The rules
// -- state, window, ADC sample, return, m_p(n), noise -- are readout_rules.h's.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"
#include "q15.h"
#include "readout_dev.h"

namespace dpemu {

__global__ void __launch_bounds__(BLOCK) feedline_index_kernel(const FeedlineParams p)
{
    constexpr int K = SCAN_K;
    __shared__ uint32_t s_cnt[SCAN_K * SCAN_W];         // readout strobes per chunk
    __shared__ uint2 s_rd[FEEDLINE_RD_SLOTS];           // the kept readouts {t, env word}
    const uint32_t tid = threadIdx.x, wl = tid & 63u, wv = tid >> 6;
    const uint32_t pr = blockIdx.x;
    const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
    const uint32_t lane = d[PAIR_LANE], core = d[PAIR_CORE], thr = d[PAIR_P1_THR];
    const uint64_t shot = pair_shot(d);

    if (tid < FEEDLINE_RD_SLOTS) s_rd[tid] = make_uint2(0xFFFFFFFFu, 0u);   // unused slot: a time no clock reaches
    const uint64_t below = wl ? (~0ull >> (64 - wl)) : 0ull;
    ReadoutScan sc;
    scan_readouts(p.summary, p.events, p.n_lanes, p.event_cap, p.meas_elem, lane, s_cnt, sc);
    const uint32_t total = sc.total;
    const uint32_t count = min(total, p.meas_cap);      // meas_cap <= FEEDLINE_RD_SLOTS
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t idx = sc.before[k] + (uint32_t)__popcll(sc.hit[k] & below);
        if (((sc.hit[k] >> wl) & 1ull) && idx < count) s_rd[idx] = make_uint2(sc.ev[k].x, sc.ev[k].y);
    }
    __syncthreads();
    if (wv != 0) return;
    // the prepared state of every kept readout; a pair without one uses draw 0
    const uint32_t draws = max(count, 1u);
    uint64_t st;
    if (p.states) {                                     // the *_st calls: the lane's injected bits, not the draw
        st = p.states[lane] & (0xFFFFFFFFu >> (32u - draws));   // draws in 1..32
    } else {
        const uint3 r = philox3(p.seed, shot, core, wl);
        st = __ballot(wl < draws && ro_state(r.x, thr));
    }
    if (wl < FEEDLINE_RD_SLOTS) p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + wl] = s_rd[wl];
    if (wl == 0) p.hdr[pr] = make_uint2(count, (uint32_t)st);
}

__global__ void __launch_bounds__(BLOCK) feedline_adc_kernel(const FeedlineParams p)
{
    __shared__ uint32_t s_t[DPEMU_FEEDLINE_MAX][FEEDLINE_RD_SLOTS];   // readout times (unused: 0xFFFFFFFF)
    __shared__ uint32_t s_cnt[DPEMU_FEEDLINE_MAX], s_bits[DPEMU_FEEDLINE_MAX], s_row[DPEMU_FEEDLINE_MAX];
    const uint32_t tid = threadIdx.x, line = blockIdx.y;
    const uint32_t first = p.line_first[line];
    const uint32_t n_mem = min(p.line_first[line + 1] - first, (uint32_t)DPEMU_FEEDLINE_MAX);
    for (uint32_t i = tid; i < n_mem * FEEDLINE_RD_SLOTS; i += BLOCK) {
        const uint32_t pr = p.member[first + i / FEEDLINE_RD_SLOTS];
        s_t[i / FEEDLINE_RD_SLOTS][i % FEEDLINE_RD_SLOTS] = p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + i % FEEDLINE_RD_SLOTS].x;
    }
    if (tid < n_mem) {
        const uint32_t pr = p.member[first + tid];
        const uint2 h = p.hdr[pr];
        s_cnt[tid] = h.x;
        s_bits[tid] = h.y;
        s_row[tid] = p.pairs[DEMOD_PAIR_WORDS * pr + PAIR_DRV_ROW];
    }
    __syncthreads();
    const uint32_t g = blockIdx.x * BLOCK + tid;        // the lane's group of 4 LO samples
    if (g >= p.n_samples_lo / 4u) return;

    // the two states' return rotation and gain: one set for the whole feedline
    const ReturnRot rot0 = return_rot(p.sin_lut, p.ro_theta0), rot1 = return_rot(p.sin_lut, p.ro_theta1);
    const int32_t gain0 = (int32_t)p.ro_gain0, gain1 = (int32_t)p.ro_gain1;

    // the members of a line share spc_drv and spc_lo: one drive index per sample for all of them
    const uint32_t *__restrict__ d0 = p.pairs + DEMOD_PAIR_WORDS * p.member[first];
    const uint32_t spc_drv = d0[PAIR_SPC_DRV], spc_lo = d0[PAIR_SPC_LO];
    const uint32_t sh_lo = __ffs(spc_lo) - 1;
    uint32_t clk[4];
    uint64_t di[4];
    bool ok[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const AdcIndex a = adc_index(4u * g + s, spc_drv, spc_lo, p.ro_delay, p.n_samples_drv);
        clk[s] = (4u * g + s) >> sh_lo;
        ok[s] = a.ok;
        di[s] = a.ok ? a.i : 0ull;
    }
    int32_t sum_i[4] = {0, 0, 0, 0}, sum_q[4] = {0, 0, 0, 0};
    for (uint32_t mem = 0; mem < n_mem; mem++) {
        const uint32_t cnt = __builtin_amdgcn_readfirstlane(s_cnt[mem]);
        const uint32_t bits = __builtin_amdgcn_readfirstlane(s_bits[mem]);
        const uint32_t *__restrict__ row = p.iq_drv + (uint64_t)__builtin_amdgcn_readfirstlane(s_row[mem]) * p.n_samples_drv;
        uint32_t dw[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t v = row[di[s]];
            dw[s] = ok[s] ? v : 0u;
        }
        uint32_t seen[4] = {0, 0, 0, 0};                // kept readouts with t_lo <= the sample's clock
        for (uint32_t r = 0; r < cnt; r++) {
            const uint32_t t = s_t[mem][r];
#pragma unroll
            for (int s = 0; s < 4; s++) seen[s] += t <= clk[s] ? 1u : 0u;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const bool st = ro_member_state(bits, seen[s]);
            const int32_t gn = st ? gain1 : gain0;
            // the return r, then g = (r gain + 2^15) >> 16 per component
            const uint32_t rw = rotate_return(dw[s], st ? rot1 : rot0);
            sum_i[s] += ((int32_t)(int16_t)(rw & 0xFFFFu) * gn + (1 << 15)) >> 16;
            sum_q[s] += (((int32_t)rw >> 16) * gn + (1 << 15)) >> 16;
        }
    }
    u32x4 out;
#pragma unroll
    for (int s = 0; s < 4; s++)                         // the converter clips: symmetric, never -32768
        out[s] = pack16(min(max(sum_i[s], -32767), 32767), min(max(sum_q[s], -32767), 32767));
    *reinterpret_cast<u32x4 *>(p.adc + (uint64_t)line * p.n_samples_lo + 4ull * g) = out;
}

__global__ void __launch_bounds__(BLOCK) feedline_demod_kernel(const FeedlineParams p)
{
    __shared__ long long s_sum[SCAN_W][2];
    const uint32_t tid = threadIdx.x;
    const uint32_t m = blockIdx.x, pr = blockIdx.y;
    const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
    const uint32_t core = d[PAIR_CORE], spc_lo = d[PAIR_SPC_LO];
    const uint64_t shot = pair_shot(d);
    const uint32_t count = p.hdr[pr].x;
    if (m == 0 && tid == 0) p.result[pr].x = count;
    if (m >= count) {                                   // (workgroup-uniform) an unused slot reads zero
        if (tid == 0) p.acc[(uint64_t)m * p.n_pairs + pr] = make_int2(0, 0);
        return;
    }
    const uint2 rd = p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + m];

    // ---- sweep: LO samples [j0, j1) of the LO row and the line's ADC row, 4 per lane per step ----
    const uint32_t sh_lo = __ffs(spc_lo) - 1;
    const RoWindow w = ro_window(rd.x, rd.y, sh_lo, p.ro_cpw, p.n_samples_lo);
    const uint32_t j0 = w.j0, j1 = w.j1;
    const uint32_t *__restrict__ lo_row = p.iq_lo + (uint64_t)d[PAIR_LO_ROW] * p.n_samples_lo;
    const uint32_t *__restrict__ adc_row = p.adc + (uint64_t)p.line_of[pr] * p.n_samples_lo;
    long long sum_i = 0, sum_q = 0;
    const uint32_t g_end = (j1 + 3u) >> 2;              // n_samples_lo is a multiple of 4: whole groups are inside
    for (uint32_t g = (j0 >> 2) + tid; g < g_end && j0 < j1; g += BLOCK) {
        const u32x4 lw = *reinterpret_cast<const u32x4 *>(lo_row + 4ull * g);
        const u32x4 aw = *reinterpret_cast<const u32x4 *>(adc_row + 4ull * g);
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t j = 4u * g + s;
            const uint32_t lo = (j >= j0 && j < j1) ? lw[s] : 0u;
            // P = a conj(lo), exact for every int16 half (q15.h mix_conj_m1: {P_I - 1, P_Q}); the 1 of each of
            // the group's four samples goes back in below (a masked sample gives -1 + 1 too)
            const int2 P = mix_conj_m1(aw[s], lo);
            sum_i += P.x;
            sum_q += P.y;
        }
        sum_i += 4;
    }

    // ---- reduce, then thread 0: scale (the gain is in the ADC), noise, store ----
    long long S[2];
    if (!block_sum2(sum_i, sum_q, s_sum, S)) return;
    p.acc[(uint64_t)m * p.n_pairs + pr] = demod_acc<false>(S, sh_lo, 0, philox3(p.seed, shot, core, m), p.ro_sigma);
}

hipError_t launch_feedline_index(const FeedlineParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(feedline_index_kernel, dim3(p.n_pairs), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_feedline_adc(const FeedlineParams &p, hipStream_t stream)
{
    const uint32_t groups = p.n_samples_lo / 4u;
    hipLaunchKernelGGL(feedline_adc_kernel, dim3((groups + BLOCK - 1) / BLOCK, p.n_lines), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_feedline_demod(const FeedlineParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(feedline_demod_kernel, dim3(p.meas_cap, p.n_pairs), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
