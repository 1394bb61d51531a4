// demod_iq.hip -- readout demodulation from the synthesised waveforms (gfx950).
//
// Spec: include/dpemu.h dpemu_demod_iq, DESIGN.md §2 "Waveform demodulation"
// and §4.8; CPU restatement tests/demod_iq_ref.py (bit-exact).  A pair is one
// lane's readout-drive channel and LO channel, both written by dpemu_dds.
// Read-bound: per readout the LO window (4 B per sample) and the drive
// samples under it come in, 8 B of {I, Q} go out.
//
// Two launches per call:
//   * demod_iq_kernel, grid (meas_cap, pairs), one workgroup per readout.
//     The workgroup finds its m-th readout strobe in the lane's slot-major
//     event records (readout_scan.h), draws the prepared state, then
//     sweeps the window: a lane takes 4 consecutive LO samples per step (one
//     16-B load), gathers their drive samples, rotates them by the state's
//     return phase and mixes them with conj(LO) on v_dot2_i32_i16, summing
//     in int64.  No LDS traffic and no divergent branch in the loop: samples
//     outside the window or the buffers are masked by select.  Waves reduce
//     by __shfl_xor, the workgroup through LDS, thread 0 scales, adds the
//     noise and stores.  Integer sums: the result does not depend on the
//     order, so it is bit-exact for any grid.
//   * demod_iq_result_kernel, one thread per pair: the outcome bits of the
//     pair's readouts from their stored {I, Q} (a workgroup of the first
//     launch knows only its own readout, and there are no atomics).

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"
#include "q15.h"
#include "readout_scan.h"

namespace dpemu {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__global__ void __launch_bounds__(BLOCK) demod_iq_kernel(const DemodParams p)
{
    constexpr int W = SCAN_W, K = SCAN_K;
    __shared__ uint32_t s_cnt[K * W];                   // readout strobes per chunk
    __shared__ uint2 s_hit;                             // the m-th readout strobe {t, env word}
    __shared__ long long s_sum[W][2];
    const uint32_t tid = threadIdx.x, wl = tid & 63u, wv = tid >> 6;
    const uint32_t m = blockIdx.x, pr = blockIdx.y;
    const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
    const uint32_t lane = d[0], core = d[1];
    const uint64_t shot = (uint64_t)d[2] | ((uint64_t)d[3] << 32);
    const uint32_t spc_drv = d[6], spc_lo = d[7], thr = d[8];

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

    // ---- prepared state and its return rotation (c, s_) ----
    const uint3 r = philox3(p.seed, shot, core, m);
    const uint32_t st = (thr == 0xFFFFFFFFu) || (r.x < thr);
    const uint32_t ti = (((st ? p.ro_theta1 : p.ro_theta0) + (1u << 19)) >> 20) & 4095u;
    const int32_t rc = p.sin_lut[(ti + 1024u) & 4095u], rs = p.sin_lut[ti];
    const uint32_t rot_i = pack16(rc, -rs), rot_q = pack16(rs, rc);   // d = {I low, Q high}

    // ---- sweep: LO samples [j0, j1), 4 per lane per step ----
    const uint32_t sh_lo = __ffs(spc_lo) - 1, ratio = spc_drv / spc_lo;
    const uint64_t w0 = (uint64_t)t_lo << sh_lo;
    const uint64_t w1 = w0 + ((uint64_t)(ro_words(pe) * p.ro_cpw) << sh_lo);
    const uint32_t j0 = (uint32_t)min(w0, (uint64_t)p.n_samples_lo), j1 = (uint32_t)min(w1, (uint64_t)p.n_samples_lo);
    const uint32_t *__restrict__ lo_row = p.iq_lo + (uint64_t)d[5] * p.n_samples_lo;
    const uint32_t *__restrict__ drv_row = p.iq_drv + (uint64_t)d[4] * p.n_samples_drv;
    long long sum_i = 0, sum_q = 0;
    const uint32_t g_end = (j1 + 3u) >> 2;              // n_samples_lo is a multiple of 4: whole groups are inside
    for (uint32_t g = (j0 >> 2) + tid; g < g_end && j0 < j1; g += BLOCK) {
        const u32x4 lw = *reinterpret_cast<const u32x4 *>(lo_row + 4ull * g);
        uint32_t dw[4];
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t j = 4u * g + s, n = j >> sh_lo, k = j & (spc_lo - 1u);
            const uint64_t di = (uint64_t)(n - p.ro_delay) * spc_drv + k * ratio;
            const bool ok = n >= p.ro_delay && di < p.n_samples_drv;
            const uint32_t v = drv_row[ok ? di : 0ull];
            dw[s] = ok ? v : 0u;
        }
#pragma unroll
        for (int s = 0; s < 4; s++) {
            const uint32_t j = 4u * g + s;
            const uint32_t lo = (j >= j0 && j < j1) ? lw[s] : 0u;
            // r = symsat((d (x) (c, s_) + 2^14) >> 15), {I low, Q high}
            const uint32_t rw = pk_symfloor(pk_sat(dot2(dw[s], rot_i, 1 << 14), dot2(dw[s], rot_q, 1 << 14)));
            // P = r conj(lo): P_I = r_I lo_I + r_Q lo_Q, P_Q = r_Q lo_I - r_I lo_Q
            sum_i += dot2(rw, lo, 0);
            sum_q += dot2(neg_swap(rw), lo, 0);
        }
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

    // ---- scale, noise, store ----
    const uint32_t h = 15u + sh_lo;
    const int64_t gain = st ? p.ro_gain1 : p.ro_gain0;
    int64_t sig[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int64_t T = (S[c] + (1ll << (h - 1))) >> h;
        const int64_t v = (T * gain + (1ll << 15)) >> 16;
        sig[c] = min(max(v, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
    }
    const int32_t u0 = (int32_t)(r.y & 0xFFFFu), u1 = (int32_t)(r.y >> 16);
    const int32_t u2 = (int32_t)(r.z & 0xFFFFu), u3 = (int32_t)(r.z >> 16);
    const int64_t zi = u0 + u1 - u2 - u3, zq = u0 - u1 + u2 - u3;
    int2 acc;
    acc.x = (int32_t)(sig[0] + ((zi * (int64_t)p.ro_sigma) >> 16));
    acc.y = (int32_t)(sig[1] + ((zq * (int64_t)p.ro_sigma) >> 16));
    p.acc[(uint64_t)m * p.n_pairs + pr] = acc;
}

// outcome bit m of pair pr = the discriminator on acc[m][pr], m < count
__global__ void __launch_bounds__(BLOCK) demod_iq_result_kernel(const DemodParams p)
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

hipError_t launch_demod_iq(const DemodParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(demod_iq_kernel, dim3(p.meas_cap, p.n_pairs), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_demod_iq_result(const DemodParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(demod_iq_result_kernel, dim3((p.n_pairs + BLOCK - 1) / BLOCK), dim3(BLOCK), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
