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
//     the prepared state of each, found once with demod_iq_kernel's scan
//     (readout_scan.h).  Neither hot kernel reads an event record.
//   * feedline_adc_kernel, grid (sample tiles, lines): the workgroup stages
//     its members' readout times, state bits and drive rows in LDS; a lane
//     takes 4 consecutive LO samples, gathers each member's 4 drive samples
//     (one index for all members: a line has one rate pair), picks the
//     member's state at the sample's clock, rotates and scales on the packed
//     int16 helpers, sums in int32, saturates and stores 16 bytes.
//   * feedline_demod_kernel, grid (meas_cap, pairs), one workgroup per
//     readout: two contiguous rows (the line's ADC row and the pair's LO row)
//     in 16-B loads, P = adc conj(lo) on v_dot2_i32_i16, int64 sums, wave
//     shuffles and LDS as demod_iq_kernel; thread 0 scales, adds the noise and
//     stores.  feedline_result_kernel, one thread per pair, packs the outcome
//     bits.
// Integer sums throughout: the result is the same for every grid.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"
#include "q15.h"
#include "readout_scan.h"

namespace dpemu {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(BLOCK) feedline_index_kernel(const FeedlineParams p)
{
    constexpr int K = SCAN_K;
    __shared__ uint32_t s_cnt[SCAN_K * SCAN_W];         // readout strobes per chunk
    __shared__ uint2 s_rd[FEEDLINE_RD_SLOTS];           // the kept readouts {t, env word}
    const uint32_t tid = threadIdx.x, wl = tid & 63u, wv = tid >> 6;
    const uint32_t pr = blockIdx.x;
    const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
    const uint32_t lane = d[0], core = d[1], thr = d[8];
    const uint64_t shot = (uint64_t)d[2] | ((uint64_t)d[3] << 32);

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
        st = __ballot(wl < draws && ((thr == 0xFFFFFFFFu) || (r.x < thr)));
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
        s_row[tid] = p.pairs[DEMOD_PAIR_WORDS * pr + 4];
    }
    __syncthreads();
    const uint32_t g = blockIdx.x * BLOCK + tid;        // the lane's group of 4 LO samples
    if (g >= p.n_samples_lo / 4u) return;

    // the two states' return rotation (c, s_) and gain: one set for the whole feedline
    uint32_t rot_i[2], rot_q[2];
#pragma unroll
    for (int s = 0; s < 2; s++) {
        const uint32_t ti = (((s ? p.ro_theta1 : p.ro_theta0) + (1u << 19)) >> 20) & 4095u;
        const int32_t rc = p.sin_lut[(ti + 1024u) & 4095u], rs = p.sin_lut[ti];
        rot_i[s] = pack16(rc, -rs);
        rot_q[s] = pack16(rs, rc);
    }
    const int32_t gain0 = (int32_t)p.ro_gain0, gain1 = (int32_t)p.ro_gain1;

    // the members of a line share spc_drv and spc_lo: one drive index per sample for all of them
    const uint32_t *__restrict__ d0 = p.pairs + DEMOD_PAIR_WORDS * p.member[first];
    const uint32_t spc_drv = d0[6], spc_lo = d0[7];
    const uint32_t sh_lo = __ffs(spc_lo) - 1, ratio = spc_drv / spc_lo;
    uint32_t clk[4];
    uint64_t di[4];
    bool ok[4];
#pragma unroll
    for (int s = 0; s < 4; s++) {
        const uint32_t j = 4u * g + s, k = j & (spc_lo - 1u);
        clk[s] = j >> sh_lo;
        const uint64_t i = (uint64_t)(clk[s] - p.ro_delay) * spc_drv + k * ratio;
        ok[s] = clk[s] >= p.ro_delay && i < p.n_samples_drv;
        di[s] = ok[s] ? i : 0ull;
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
            const bool st = (bits >> (max(seen[s], 1u) - 1u)) & 1u;
            const uint32_t ri = st ? rot_i[1] : rot_i[0], rq = st ? rot_q[1] : rot_q[0];
            const int32_t gn = st ? gain1 : gain0;
            // r = symsat((d (x) (c, s_) + 2^14) >> 15), then g = (r gain + 2^15) >> 16 per component
            const uint32_t rw = pk_symfloor(pk_sat(dot2(dw[s], ri, 1 << 14), dot2(dw[s], rq, 1 << 14)));
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
    constexpr int W = BLOCK / 64;
    __shared__ long long s_sum[W][2];
    const uint32_t tid = threadIdx.x, wl = tid & 63u, wv = tid >> 6;
    const uint32_t m = blockIdx.x, pr = blockIdx.y;
    const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
    const uint32_t core = d[1], spc_lo = d[7];
    const uint64_t shot = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
    const uint32_t count = p.hdr[pr].x;
    if (m == 0 && tid == 0) p.result[pr].x = count;
    if (m >= count) {                                   // (workgroup-uniform) an unused slot reads zero
        if (tid == 0) p.acc[(uint64_t)m * p.n_pairs + pr] = make_int2(0, 0);
        return;
    }
    const uint2 rd = p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + m];
    const uint32_t t_lo = rd.x, pe = rd.y;

    // ---- sweep: LO samples [j0, j1) of the LO row and the line's ADC row, 4 per lane per step ----
    const uint32_t sh_lo = __ffs(spc_lo) - 1;
    const uint64_t w0 = (uint64_t)t_lo << sh_lo;
    const uint64_t w1 = w0 + ((uint64_t)(ro_words(pe) * p.ro_cpw) << sh_lo);
    const uint32_t j0 = (uint32_t)min(w0, (uint64_t)p.n_samples_lo), j1 = (uint32_t)min(w1, (uint64_t)p.n_samples_lo);
    const uint32_t *__restrict__ lo_row = p.iq_lo + (uint64_t)d[5] * p.n_samples_lo;
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

    // ---- reduce: wave by shuffles, workgroup through LDS ----
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        sum_i += __shfl_xor(sum_i, o, 64);
        sum_q += __shfl_xor(sum_q, o, 64);
    }
    if (wl == 0) { s_sum[wv][0] = sum_i; s_sum[wv][1] = sum_q; }
    __syncthreads();
    if (tid != 0) return;
    long long S[2] = {0, 0};
#pragma unroll
    for (int w = 0; w < W; w++) { S[0] += s_sum[w][0]; S[1] += s_sum[w][1]; }

    // ---- scale (the gain is in the ADC), noise, store ----
    const uint32_t h = 15u + sh_lo;
    int64_t sig[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int64_t T = (S[c] + (1ll << (h - 1))) >> h;
        sig[c] = min(max(T, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
    }
    const uint3 r = philox3(p.seed, shot, core, m);
    const int32_t u0 = (int32_t)(r.y & 0xFFFFu), u1 = (int32_t)(r.y >> 16);
    const int32_t u2 = (int32_t)(r.z & 0xFFFFu), u3 = (int32_t)(r.z >> 16);
    const int64_t zi = u0 + u1 - u2 - u3, zq = u0 - u1 + u2 - u3;
    int2 acc;
    acc.x = (int32_t)(sig[0] + ((zi * (int64_t)p.ro_sigma) >> 16));
    acc.y = (int32_t)(sig[1] + ((zq * (int64_t)p.ro_sigma) >> 16));
    p.acc[(uint64_t)m * p.n_pairs + pr] = acc;
}

// outcome bit m of pair pr = the discriminator on acc[m][pr], m < count
__global__ void __launch_bounds__(BLOCK) feedline_result_kernel(const FeedlineParams p)
{
    const uint32_t pr = blockIdx.x * BLOCK + threadIdx.x;
    if (pr >= p.n_pairs) return;
    const uint32_t axis = p.pairs[DEMOD_PAIR_WORDS * pr + 9];
    const uint32_t count = p.result[pr].x;
    uint32_t bits = 0;
    for (uint32_t m = 0; m < count; m++)
        bits |= demod_decide(p.acc[(uint64_t)m * p.n_pairs + pr], axis, p.ro_thr) << m;
    p.result[pr].y = bits;
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

hipError_t launch_feedline_result(const FeedlineParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(feedline_result_kernel, dim3((p.n_pairs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
