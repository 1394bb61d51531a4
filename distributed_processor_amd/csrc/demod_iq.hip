// demod_iq.hip -- readout demodulation from the synthesised waveforms (gfx950).
//
// Spec: include/dpemu.h dpemu_demod_iq, DESIGN.md §2 "Waveform demodulation"
// and §4.8; CPU restatement tests/demod_iq_ref.py (bit-exact).  A pair is one
// lane's readout-drive channel and LO channel, both written by dpemu_dds.
// Read-bound: per readout the LO window (4 B per sample) and the drive
// samples under it come in, 8 B of {I, Q} go out.  The rules -- state, window,
// ADC sample, return, noise, discriminator -- are readout_rules.h's, their
// packed and workgroup-wide forms readout_dev.h's.
//
// Two launches per call:
//   * demod_iq_kernel, grid (meas_cap, pairs), one workgroup per readout.
//     The workgroup finds its m-th readout strobe in the lane's slot-major
//     event records (scan_readouts), draws the prepared state, then
//     sweeps the window: a lane takes 4 consecutive LO samples per step (one
//     16-B load), gathers their drive samples, rotates them by the state's
//     return phase and mixes them with conj(LO) on v_dot2_i32_i16, summing
//     in int64.  No LDS traffic and no divergent branch in the loop: samples
//     outside the window or the buffers are masked by select.  Waves reduce
//     by __shfl_xor, the workgroup through LDS, thread 0 scales, adds the
//     noise and stores.  Integer sums: the result does not depend on the
//     order, so it is bit-exact for any grid.
//   * readout_result_kernel, one thread per pair (dpemu_demod_feedline's
//     too): the outcome bits of the pair's readouts from their stored {I, Q}
//     (a workgroup of the first launch knows only its own readout, and there
//     are no atomics).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"
#include "q15.h"
#include "readout_dev.h"

namespace dpemu {

__global__ void __launch_bounds__(BLOCK) demod_iq_kernel(const DemodParams p)
{
    constexpr int W = SCAN_W, K = SCAN_K;
    __shared__ uint32_t s_cnt[K * W];                   // readout strobes per chunk
    __shared__ uint2 s_hit;                             // the m-th readout strobe {t, env word}
    __shared__ long long s_sum[W][2];
    const uint32_t tid = threadIdx.x, wl = tid & 63u;
    const uint32_t m = blockIdx.x, pr = blockIdx.y;
    const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
    const uint32_t lane = d[PAIR_LANE], core = d[PAIR_CORE];
    const uint64_t shot = pair_shot(d);
    const uint32_t spc_drv = d[PAIR_SPC_DRV], spc_lo = d[PAIR_SPC_LO], thr = d[PAIR_P1_THR];

    // ---- the lane's m-th readout strobe ----
    const uint64_t below = wl ? (~0ull >> (64 - wl)) : 0ull;
    ReadoutScan sc;
    scan_readouts(p.summary, p.events, p.n_lanes, p.event_cap, p.meas_elem, lane, s_cnt, sc);
    const uint32_t total = sc.total;
    const uint32_t count = min(total, p.meas_cap);
    if (m == 0 && tid == 0) p.result[pr].x = count;
    if (m >= count) {                                   // (workgroup-uniform) an unused slot reads zero
        if (tid == 0) p.acc[(uint64_t)m * p.n_pairs + pr] = make_int2(0, 0);
        return;
    }
#pragma unroll
    for (int k = 0; k < K; k++)
        if (((sc.hit[k] >> wl) & 1ull) && sc.before[k] + (uint32_t)__popcll(sc.hit[k] & below) == m)
            s_hit = make_uint2(sc.ev[k].x, sc.ev[k].y);
    __syncthreads();
    const uint32_t t_lo = s_hit.x, pe = s_hit.y;

    // ---- prepared state and its return rotation ----
    const uint3 r = philox3(p.seed, shot, core, m);
    const uint32_t st = ro_state(r.x, thr);
    const ReturnRot rot = return_rot(p.sin_lut, st ? p.ro_theta1 : p.ro_theta0);

    // ---- sweep: LO samples [j0, j1), 4 per lane per step ----
    const uint32_t sh_lo = __ffs(spc_lo) - 1;
    const RoWindow w = ro_window(t_lo, pe, sh_lo, p.ro_cpw, p.n_samples_lo);
    const uint32_t j0 = w.j0, j1 = w.j1;
    const uint32_t *__restrict__ lo_row = p.iq_lo + (uint64_t)d[PAIR_LO_ROW] * p.n_samples_lo;
    const uint32_t *__restrict__ drv_row = p.iq_drv + (uint64_t)d[PAIR_DRV_ROW] * p.n_samples_drv;
    long long sum_i = 0, sum_q = 0;
    const uint32_t g_end = (j1 + 3u) >> 2;              // n_samples_lo is a multiple of 4: whole groups are inside
    for (uint32_t g = (j0 >> 2) + tid; g < g_end && j0 < j1; g += BLOCK) {
        const u32x4 lw = *reinterpret_cast<const u32x4 *>(lo_row + 4ull * g);
        uint32_t dw[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const AdcIndex a = adc_index(4u * g + s, spc_drv, spc_lo, p.ro_delay, p.n_samples_drv);
            const uint32_t v = drv_row[a.ok ? a.i : 0ull];
            dw[s] = a.ok ? v : 0u;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t j = 4u * g + s;
            const uint32_t lo = (j >= j0 && j < j1) ? lw[s] : 0u;
            const uint32_t rw = rotate_return(dw[s], rot);
            // P = r conj(lo): P_I = r_I lo_I + r_Q lo_Q, P_Q = r_Q lo_I - r_I lo_Q
            sum_i += dot2(rw, lo, 0);
            sum_q += dot2(neg_swap(rw), lo, 0);
        }
    }

    // ---- reduce, then thread 0: scale, noise, store ----
    long long S[2];
    if (!block_sum2(sum_i, sum_q, s_sum, S)) return;
    p.acc[(uint64_t)m * p.n_pairs + pr] = demod_acc<true>(S, sh_lo, st ? p.ro_gain1 : p.ro_gain0, r, p.ro_sigma);
}

// outcome bit m of pair pr = the discriminator on acc[m][pr], m < count = result[pr].x
__global__ void __launch_bounds__(BLOCK) readout_result_kernel(const uint32_t *pairs, const int2 *acc, uint2 *result,
                                                               uint32_t n_pairs, int32_t ro_thr)
{
    const uint32_t pr = blockIdx.x * BLOCK + threadIdx.x;
    if (pr >= n_pairs) return;
    const uint32_t axis = pairs[DEMOD_PAIR_WORDS * pr + PAIR_AXIS];
    const uint32_t count = result[pr].x;
    uint32_t bits = 0;
    for (uint32_t m = 0; m < count; m++) {
        const int2 a = acc[(uint64_t)m * n_pairs + pr];
        bits |= demod_decide(a.x, a.y, axis, ro_thr) << m;
    }
    result[pr].y = bits;
}

hipError_t launch_demod_iq(const DemodParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(demod_iq_kernel, dim3(p.meas_cap, p.n_pairs), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_readout_result(const uint32_t *pairs, const int2 *acc, uint2 *result, uint32_t n_pairs, int32_t ro_thr,
                                 hipStream_t stream)
{
    hipLaunchKernelGGL(readout_result_kernel, dim3((n_pairs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, pairs, acc,
                       result, n_pairs, ro_thr);
    return hipGetLastError();
}

}  // namespace dpemu
