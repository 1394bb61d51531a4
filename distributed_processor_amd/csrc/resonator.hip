// resonator.hip -- readout resonator response and per-sample converter noise
// on the shared feedline (gfx950).
//
// Spec: include/dpemu.h dpemu_feedline_adc_res (normative), DESIGN.md §2
// "Resonator response" and §4.11; CPU restatement tests/resonator_ref.py
// (bit-exact).  Every member of a line passes its delayed drive through a
// one-pole complex recurrence y' = x + a y whose pole a and coupling c follow
// the member's prepared state; the line's ADC sample is the clipped sum of the
// members' returns c y' and one noise draw.
//
// The recurrence is sequential in time and exact, so the parallelism is over
// members: feedline_res_kernel runs one single-wave workgroup per run of whole
// lines with at most RES_MEMBERS = 16 members (the host packs them: wg_first;
// 64, 32 and 16 members measured 1.55 / 1.04 / 0.85 ms at 8,192 members and
// 2.14 / 1.71 / 1.78 ms at 65,520, DESIGN.md §4.11: a wave's time is its own
// serial walk plus the gather and sum of all its members, so fewer members
// per wave -- idle lanes in the walk -- are faster until the device is full).
// Time goes in tiles of RES_TILE LO samples, three phases per tile:
//   gather  lane = sample, loop over members: the strided drive gather of
//           the "ADC" rule (readout_rules.h adc_index), RES_TILE words per member, held in registers
//           -- issued for tile k + 1 before tile k is computed -- and then
//           written to LDS rows of pitch RES_TILE + 1 words
//   walk    lane = member: RES_TILE steps down the member's own row (the odd
//           pitch puts the 32 lanes of a half wave on 32 banks), y and the
//           current coefficients in registers, eight v_mad_i64_i32 per step;
//           the return g overwrites the drive word in place
//   sum     lane = sample, loop over the workgroup's lines: the members' g
//           summed in int32, one Philox draw per (line, sample), clamp, pack
//           to an LDS row; then 16-byte stores of the ADC tile
// The member's state at a clock is found from the index pass's rd / hdr rows
// by the m_p(n) counting rule: a member holds the count of kept readouts at or
// before the clock and the next readout time after it, and recounts (over its
// unsorted times) only when the clock reaches that time -- at most count + 1
// times per trace.  A tile in which no member's count changes (most) walks
// without the per-step test, unrolled by four.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"
#include "q15.h"

namespace dpemu {

constexpr uint32_t RES_PITCH = RES_TILE + 1;
static_assert(RES_TILE == RES_WAVE && RES_MEMBERS <= RES_WAVE && RES_MEMBERS >= DPEMU_FEEDLINE_MAX,
              "one wave: a lane is a sample in the gather and the sum, a member in the walk; a line fits a workgroup");

// (a b + c d + 2^29) >> 30 on int64 products (two v_mad_i64_i32); the callers' bounds keep it within int32
__device__ __forceinline__ int32_t cmad_q30(int32_t a, int32_t b, int32_t c, int32_t d)
{
    return (int32_t)(((int64_t)a * b + ((int64_t)c * d + (1ll << 29))) >> 30);
}

__global__ void __launch_bounds__(RES_WAVE) feedline_res_kernel(const ResonatorParams q)
{
    const FeedlineParams &p = q.f;
    __shared__ uint32_t s_d[RES_MEMBERS * RES_PITCH];                   // drive words, then the returns g, per member
    __shared__ __attribute__((aligned(16))) uint32_t s_out[RES_MEMBERS * RES_TILE];   // the ADC tile, per line
    const uint32_t l = threadIdx.x;
    const uint32_t line0 = q.wg_first[blockIdx.x];
    const uint32_t n_lines = min(q.wg_first[blockIdx.x + 1] - line0, RES_MEMBERS);
    const uint32_t mem0 = p.line_first[line0];
    const uint32_t n_mem = min(p.line_first[line0 + n_lines] - mem0, RES_MEMBERS);
    const uint32_t n_lo = p.n_samples_lo;

    // ---- lane = member: its rates, readout index header and the two coefficient sets ----
    uint32_t pr = 0, cnt = 0, bits = 0, sh_lo = 0, row_m = 0, spc_m = 0;
    int4 k0 = make_int4(0, 0, 0, 0), k1 = k0;
    if (l < n_mem) {
        pr = p.member[mem0 + l];
        const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * pr;
        sh_lo = __ffs(d[PAIR_SPC_LO]) - 1;
        row_m = d[PAIR_DRV_ROW];
        spc_m = d[PAIR_SPC_DRV];
        const uint2 h = p.hdr[pr];
        cnt = min(h.x, FEEDLINE_RD_SLOTS);
        bits = h.y;
        k0 = q.coef[2ull * pr];
        k1 = q.coef[2ull * pr + 1];
    }

    // the drive words of tile `tile`, sample l of every member (0 outside the drive row or the trace).
    // Member m's row and rates are read from lane m's registers (spc_drv 0: no member); the empty asm
    // redefines them per tile, so the members' scalars are not all hoisted out of the tile loop and held
    // in SGPRs across it.  A sample that reads 0 loads the zero word behind the coefficient table:
    // nothing then depends on a load before the tile is written to LDS, so a lane's RES_MEMBERS loads
    // are all in flight
    uint32_t v[RES_MEMBERS];
    const uint32_t *__restrict__ zero = reinterpret_cast<const uint32_t *>(q.coef + 2ull * p.n_pairs);
    auto gather = [&](uint32_t tile) {
        const uint32_t j = tile * RES_TILE + l;
        uint32_t row_v = row_m, spc_v = spc_m, sh_v = sh_lo;
        asm volatile("" : "+v"(row_v), "+v"(spc_v), "+v"(sh_v));
#pragma unroll
        for (uint32_t m = 0; m < RES_MEMBERS; m++) {
            const uint32_t spc_drv = __builtin_amdgcn_readlane(spc_v, m);
            const uint32_t sh = __builtin_amdgcn_readlane(sh_v, m);
            const uint32_t *__restrict__ row = p.iq_drv + (uint64_t)__builtin_amdgcn_readlane(row_v, m) * p.n_samples_drv;
            // readout_rules.h adc_index, rearranged: with j = n spc_lo + k and ratio = spc_drv >> sh, its index
            // (n - ro_delay) spc_drv + k ratio = (n spc_lo + k) ratio - ro_delay spc_drv = j ratio - ro_delay spc_drv
            // (one 64-bit product per member instead of the split of j), and its n >= ro_delay is the test below
            const uint64_t i = (uint64_t)j * (spc_drv >> sh) - (uint64_t)p.ro_delay * spc_drv;
            const bool ok = spc_drv != 0u && j < n_lo && (j >> sh) >= p.ro_delay && i < p.n_samples_drv;
            v[m] = *(ok ? row + i : zero);
        }
    };

    int32_t y_i = 0, y_q = 0;
    int4 k = k0;                                        // the current state's {pole, coupling}
    int32_t na_im = -k.y, nc_im = -k.w;
    uint32_t nxt = l < n_mem ? 0u : 0xFFFFFFFFu;        // the first clock at which the readout count changes
    const uint32_t n_tiles = (n_lo + RES_TILE - 1) / RES_TILE;
    gather(0);
    for (uint32_t tile = 0; tile < n_tiles; tile++) {
        const uint32_t t0 = tile * RES_TILE, len = min(RES_TILE, n_lo - t0);
#pragma unroll
        for (uint32_t m = 0; m < RES_MEMBERS; m++) s_d[m * RES_PITCH + l] = v[m];
        __syncthreads();
        if (tile + 1 < n_tiles) gather(tile + 1);       // in flight during the walk

        // ---- walk: lane = member ----
        // one step: x from the member's row, y' = x + a y, the return c y' in place of x
        auto step = [&](uint32_t t) {
            const uint32_t x = s_d[l * RES_PITCH + t];
            const int32_t x_i = (int32_t)(int16_t)(x & 0xFFFFu), x_q = (int32_t)x >> 16;
            const int32_t n_i = x_i + cmad_q30(k.x, y_i, na_im, y_q);
            const int32_t n_q = x_q + cmad_q30(k.x, y_q, k.y, y_i);
            y_i = n_i; y_q = n_q;
            const int32_t g_i = cmad_q30(k.z, y_i, nc_im, y_q), g_q = cmad_q30(k.z, y_q, k.w, y_i);
            s_d[l * RES_PITCH + t] = pack16(min(max(g_i, -32767), 32767), min(max(g_q, -32767), 32767));
        };
        if (l < RES_MEMBERS) {                          // (lanes past the rows stay out of LDS)
            // no member's readout count changes inside most tiles: those walk without the per-step test,
            // four steps unrolled so that the next reads of x are issued under the current products
            const bool quiet = len == RES_TILE && __ballot(nxt <= ((t0 + RES_TILE - 1u) >> sh_lo)) == 0ull;
            if (quiet) {
#pragma unroll 4
                for (uint32_t t = 0; t < RES_TILE; t++) step(t);
            } else {
                for (uint32_t t = 0; t < len; t++) {
                    const uint32_t n = (t0 + t) >> sh_lo;
                    if (n >= nxt) {                     // the m_p(n) rule, recounted where it can change
                        uint32_t seen = 0;
                        nxt = 0xFFFFFFFFu;
                        for (uint32_t r = 0; r < cnt; r++) {
                            const uint32_t tr = p.rd[(uint64_t)pr * FEEDLINE_RD_SLOTS + r].x;
                            seen += tr <= n ? 1u : 0u;
                            nxt = tr > n ? min(nxt, tr) : nxt;
                        }
                        k = ro_member_state(bits, seen) ? k1 : k0;
                        na_im = -k.y; nc_im = -k.w;
                    }
                    step(t);
                }
            }
        }
        __syncthreads();

        // ---- sum: lane = sample, line by line ----
        for (uint32_t li = 0; li < n_lines; li++) {
            const uint32_t a = p.line_first[line0 + li] - mem0;
            const uint32_t b = min(p.line_first[line0 + li + 1] - mem0, n_mem);
            int32_t sum_i = 0, sum_q = 0;
            for (uint32_t m = a; m < b; m++) {
                const uint32_t w = s_d[m * RES_PITCH + l];
                sum_i += (int32_t)(int16_t)(w & 0xFFFFu);
                sum_q += (int32_t)w >> 16;
            }
            int64_t tot_i = sum_i, tot_q = sum_q;
            if (q.adc_sigma) {                          // the converter's noise: one draw per line and sample
                const uint32_t *__restrict__ d = p.pairs + DEMOD_PAIR_WORDS * p.member[mem0 + a];
                const uint3 r = philox3(p.seed, pair_shot(d), 0x80000000u | d[PAIR_CORE], t0 + l);
                const RoNoise z = ro_noise_pair(r.y, r.z);
                tot_i += ro_noise(z.zi, q.adc_sigma);
                tot_q += ro_noise(z.zq, q.adc_sigma);
            }
            const int32_t o_i = (int32_t)min(max(tot_i, (int64_t)-32767), (int64_t)32767);
            const int32_t o_q = (int32_t)min(max(tot_q, (int64_t)-32767), (int64_t)32767);
            s_out[li * RES_TILE + l] = pack16(o_i, o_q);
        }
        __syncthreads();

        // ---- store: 16 bytes per lane (n_samples_lo is a multiple of 4: a group is inside or outside) ----
        for (uint32_t g = l; g < n_lines * (RES_TILE / 4u); g += RES_WAVE) {
            const uint32_t li = g / (RES_TILE / 4u), j = t0 + 4u * (g % (RES_TILE / 4u));
            if (j < n_lo)
                *reinterpret_cast<u32x4 *>(p.adc + (uint64_t)(line0 + li) * n_lo + j) =
                    *reinterpret_cast<const u32x4 *>(&s_out[li * RES_TILE + 4u * (g % (RES_TILE / 4u))]);
        }
        // (the next tile's writes to s_d follow this tile's sum by the barrier above; its writes to s_out
        // follow these reads by the barriers of its own gather and walk)
    }
}

hipError_t launch_feedline_res(const ResonatorParams &p, hipStream_t stream)
{
    hipLaunchKernelGGL(feedline_res_kernel, dim3(p.n_wgs), dim3(RES_WAVE), 0, stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
