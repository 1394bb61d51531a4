// readout_scan.h -- a lane's readout strobes among its event records, found by
// a whole workgroup (demod_iq.hip, feedline.hip): 4 records per thread, ballot
// + popcount per wave, the 16 chunk counts scanned from LDS.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

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
        r.hit[k] = __ballot(e < n_ev && (r.ev[k].y >> 28) == DPEMU_EV_STROBE && ((r.ev[k].y >> 24) & 3u) == meas_elem);
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

}  // namespace dpemu
