// readout_dev.h -- the device-only pieces the readout stages share (demod_iq.hip, feedline.hip): a lane's
// readout strobes found among its event records by a whole workgroup (4 records per thread, ballot + popcount
// per wave, the 16 chunk counts scanned from LDS), the packed return rotation, the workgroup sum of a
// demodulator's two int64 sums and its scale-noise tail.  The integer rules under them: readout_rules.h.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "q15.h"
#include "readout_rules.h"

namespace dpemu {

constexpr int SCAN_W = BLOCK / 64;                  // waves per workgroup
constexpr int SCAN_K = DDS_MAX_EVENTS / BLOCK;      // event chunks (64 records) per wave

// Chunk k * SCAN_W + wave of the lane's first min(n_events, event_cap) records:
// ev[k] this thread's record {t, env | cfg | kind}, hit[k] the wave's readout
// strobes (strobes of element meas_elem), before[k] the readout strobes in
// the chunks before it, total the lane's readout strobes.  The strobe of a
// thread whose bit is set in hit[k] is readout before[k] + popcount(hit[k] &
// the lanes below it), in event order.
struct ReadoutScan {
    uint2 ev[SCAN_K];
    uint64_t hit[SCAN_K];
    uint32_t before[SCAN_K], total;
};

// s_cnt: SCAN_K * SCAN_W words of LDS.  Every thread of the workgroup calls it
// (it holds a barrier).
__device__ __forceinline__ void scan_readouts(const uint32_t *summary, const uint4 *events, uint32_t n_lanes,
                                              uint32_t event_cap, uint32_t meas_elem, uint32_t lane, uint32_t *s_cnt,
                                              ReadoutScan &r)
{
    constexpr int W = SCAN_W, K = SCAN_K;
    const uint32_t tid = threadIdx.x, wl = tid & 63u, wv = tid >> 6;
    const uint32_t n_ev = min(summary[8ull * lane + 2], event_cap);
#pragma unroll
    for (int k = 0; k < K; k++) {                       // chunk k * W + wv: records t and env | cfg | kind
        const uint32_t e = (k * W + wv) * 64u + wl;
        r.ev[k] = e < n_ev ? *reinterpret_cast<const uint2 *>(events + ((uint64_t)e * n_lanes + lane))
                           : make_uint2(0u, 0u);
    }
#pragma unroll
    for (int k = 0; k < K; k++) {
        const uint32_t e = (k * W + wv) * 64u + wl;
        r.hit[k] = __ballot(e < n_ev && strobe_of(r.ev[k].y, meas_elem));
        if (wl == 0) s_cnt[k * W + wv] = (uint32_t)__popcll(r.hit[k]);
    }
    __syncthreads();
    r.total = 0;
#pragma unroll
    for (int k = 0; k < K; k++) r.before[k] = 0;
#pragma unroll
    for (int q = 0; q < K * W; q++) {
        const uint32_t c = s_cnt[q];
#pragma unroll
        for (int k = 0; k < K; k++) r.before[k] += (uint32_t)q < (uint32_t)k * W + wv ? c : 0u;
        r.total += c;
    }
}

// The return rotation (c, s_) of a phase ro_theta, packed for dot2 on a drive word d = {I low, Q high}, and
// r = symsat((d (x) (c, s_) + 2^14) >> 15), {I low, Q high}
struct ReturnRot {
    uint32_t i, q;
};
__device__ __forceinline__ ReturnRot return_rot(const int16_t *sin_lut, uint32_t theta)
{
    const uint32_t ti = ro_theta_index(theta);
    const int32_t rc = sin_lut[(ti + 1024u) & 4095u], rs = sin_lut[ti];
    return ReturnRot{pack16(rc, -rs), pack16(rs, rc)};
}
__device__ __forceinline__ uint32_t rotate_return(uint32_t d, const ReturnRot rot)
{
    return pk_symfloor(pk_sat(dot2(d, rot.i, 1 << 14), dot2(d, rot.q, 1 << 14)));
}

// The workgroup's sums of every thread's (a, b): waves by shuffles, the workgroup through s_sum.  True for
// thread 0 alone, whose S holds them.  Every thread of the workgroup calls it (it holds a barrier).
__device__ __forceinline__ bool block_sum2(long long a, long long b, long long (*s_sum)[2], long long S[2])
{
    const uint32_t tid = threadIdx.x, wl = tid & 63u, wv = tid >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        a += __shfl_xor(a, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (wl == 0) { s_sum[wv][0] = a; s_sum[wv][1] = b; }
    __syncthreads();
    if (tid != 0) return false;
    S[0] = S[1] = 0;
#pragma unroll
    for (int w = 0; w < SCAN_W; w++) { S[0] += s_sum[w][0]; S[1] += s_sum[w][1]; }
    return true;
}

// A demodulator's accumulator from its window sums S ("scale", "noise"): T = (S + 2^(h-1)) >> h, h = 15 +
// log2 spc_lo; GAIN: sig = (T gain + 2^15) >> 16 (else the gain is in the ADC: sig = T); saturated to int32,
// plus the readout noise of the Philox draw r
template <bool GAIN>
__device__ __forceinline__ int2 demod_acc(const long long S[2], uint32_t sh_lo, int64_t gain, const uint3 r, uint32_t sigma)
{
    const uint32_t h = 15u + sh_lo;
    int64_t sig[2];
#pragma unroll
    for (int c = 0; c < 2; c++) {
        const int64_t T = (S[c] + (1ll << (h - 1))) >> h;
        const int64_t v = GAIN ? (T * gain + (1ll << 15)) >> 16 : T;
        sig[c] = min(max(v, (int64_t)INT32_MIN), (int64_t)INT32_MAX);
    }
    const RoNoise z = ro_noise_pair(r.y, r.z);
    return make_int2((int32_t)(sig[0] + ro_noise(z.zi, sigma)), (int32_t)(sig[1] + ro_noise(z.zq, sigma)));
}

}  // namespace dpemu
