// qsim.hip -- qubit state from the emulated drive pulses (gfx950).
//
// Spec: include/dpemu.h dpemu_qsim / dpemu_qsim_meas, DESIGN.md §2 "Qubit state
// from the drive pulses" and §4.13; CPU restatements tests/qsim_ref.py and
// tests/qsim_meas_ref.py (bit-exact).  Integer arithmetic only: Q30 amplitudes,
// int64 products (resonator.hip's cmad_q30 shape), so the result does not
// depend on the grid.
//
// qsim_kernel, one thread per (register, shot) row, rows register-major: with
// core-major lanes adjacent threads read adjacent 16-byte event records of a
// slot (shot-major lanes: a stride of C records).  The workgroup stages the
// 6 KB phase table and the dictionary slots of the registers its rows belong
// to in dynamic LDS (the host sizes it: launch_plan.h plan_qsim).  A thread
// keeps the 4 amplitudes in registers and walks the two lanes' records with a
// one-record look-ahead each: a step refills the heads that are empty (one
// load each, skipping what is no drive strobe), and once both are settled
// takes the earlier one, looks its key up in the core's slot and applies the
// gate.  The acted qubit's amplitude pairs are picked by selects (x1 and x2
// trade places around a gate on the first core's qubit): no indexed register
// array.  qsim_kernel<true, *> (dpemu_qsim_meas) keeps the readout strobes in the
// same heads; a taken one measures its core's qubit on the four amplitudes
// (measure() below), counts the lane's readouts and packs their bits.  Waves
// diverge -- a wave of config 4 holds about six different pulse programs --
// and loop to their longest merged stream.
//
// qsim_kernel<MEAS, true> (dpemu_qsim_decay) adds the qubit clocks tl0 / tl1 and
// advance() below: before a readout or a matched gate acts, the acted qubit
// (for a controlled gate the control, then the target) decays over the clocks
// since its last advance.  The span factors come from the core's 64-word table
// in global memory, one entry per set bit of dt.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"
#include "lane.h"

namespace dpemu {

struct C32 { int32_t re, im; };
struct C64 { long long re, im; };

// (p x + 2^29) >> 30 per component, the two products summed before the one floor shift
__device__ __forceinline__ C64 cmulr64(const C32 p, const C32 x)
{
    const long long re = (long long)p.re * x.re - (long long)p.im * x.im + (1ll << 29);
    const long long im = (long long)p.re * x.im + (long long)p.im * x.re + (1ll << 29);
    return C64{re >> 30, im >> 30};
}

// ... of operands whose product fits: a phase factor times a phase factor or a matrix component
__device__ __forceinline__ C32 cmulr(const C32 p, const C32 x)
{
    const C64 r = cmulr64(p, x);
    return C32{(int32_t)r.re, (int32_t)r.im};
}

__device__ __forceinline__ int32_t clamp31(long long v)
{
    return (int32_t)min(max(v, -2147483647ll), 2147483647ll);
}

struct Gate2 { C32 a, b, c, d; };

// [[a, b], [c, d]] on the pair (x0, x1)
__device__ __forceinline__ void apply(const Gate2 &g, C32 &x0, C32 &x1)
{
    const C64 p = cmulr64(g.a, x0), q = cmulr64(g.b, x1), r = cmulr64(g.c, x0), s = cmulr64(g.d, x1);
    x0 = C32{clamp31(p.re + q.re), clamp31(p.im + q.im)};
    x1 = C32{clamp31(r.re + s.re), clamp31(r.im + s.im)};
}

// Pauli `code` (0 I, 1 X, 2 Y, 3 Z) on the pair (x0, x1): exact
__device__ __forceinline__ void pauli(uint32_t code, C32 &x0, C32 &x1)
{
    const C32 a = x0, b = x1;
    if (code == 1u) {
        x0 = b;
        x1 = a;
    } else if (code == 2u) {
        x0 = C32{b.im, -b.re};
        x1 = C32{-a.im, a.re};
    } else if (code == 3u) {
        x1 = C32{-b.re, -b.im};
    }
}

__device__ __forceinline__ unsigned long long pop(const C32 x)
{
    return (unsigned long long)((long long)x.re * x.re + (long long)x.im * x.im);
}

__device__ __forceinline__ C32 shl(const C32 x, uint32_t s)
{
    return C32{(int32_t)((uint32_t)x.re << s), (int32_t)((uint32_t)x.im << s)};
}

// Projective readout of qubit q (0: the first core's, 1: the second's) with the
// draw u (include/dpemu.h dpemu_qsim_meas "Readout m of a lane"): the outcome b
// with P(1) = A / T, the amplitudes of the other value zeroed, the rest shifted
// left so that their populations sum to [2^58, 2^60).  Returns b.
__device__ __forceinline__ uint32_t measure(uint32_t q, unsigned long long u, C32 &x0, C32 &x1, C32 &x2, C32 &x3)
{
    const unsigned long long P0 = pop(x0), P1 = pop(x1), P2 = pop(x2), P3 = pop(x3);
    const unsigned long long T = P0 + P1 + P2 + P3;
    const unsigned long long A = (q ? P1 : P2) + P3;
    const unsigned long long v = u * (T >> 32) + ((u * (T & 0xFFFFFFFFull)) >> 32);
    const bool b = T - A <= v;
    const unsigned long long Tc = b ? A : T - A;        // the sum of the populations that stay
    const int hi = 63 - __clzll((long long)Tc);         // msb (Tc != 0)
    const uint32_t s = (Tc == 0ull || hi >= 58) ? 0u : (uint32_t)(59 - hi) >> 1;
    // x0 holds this qubit's bit 0 and x3 its bit 1 whichever qubit it is; x1 and x2 trade places
    const bool z1 = q ? !b : b, z2 = q ? b : !b;
    const C32 zero = {0, 0};
    x0 = b ? zero : shl(x0, s);
    x1 = z1 ? zero : shl(x1, s);
    x2 = z2 ? zero : shl(x2, s);
    x3 = b ? shl(x3, s) : zero;
    return b ? 1u : 0u;
}

// Counter tags of the decay draws (include/dpemu.h dpemu_qsim_decay "draws"): | core
constexpr uint32_t DECAY_OWN = 0x08000000u, DECAY_TARGET = 0x04000000u, DECAY_FINAL = 0x02000000u;

// (g x + 2^29) >> 30 per component, g a Q30 factor in [0, 2^30]
__device__ __forceinline__ C32 scaled(uint32_t g, const C32 x)
{
    return C32{(int32_t)(((long long)g * x.re + (1ll << 29)) >> 30), (int32_t)(((long long)g * x.im + (1ll << 29)) >> 30)};
}

__device__ __forceinline__ C32 neg(const C32 x)      // modulo 2^32, as shl
{
    return C32{(int32_t)(0u - (uint32_t)x.re), (int32_t)(0u - (uint32_t)x.im)};
}

// Advance qubit q (0: the first core's, 1: the second's; `core` its core) to the clock t (include/dpemu.h
// dpemu_qsim_decay "Damping step" / "Dephasing step"): the span factors G and E over dt = t - tl from the core's
// table, one draw on (tag | core, n); the no-jump decay of the |1> amplitudes or the jump to |0>, the
// renormalising shift, then the sampled Z flip.  Returns (jumped ? 1 : 0) | (flipped ? 2 : 0)
__device__ __forceinline__ uint32_t advance(const QsimParams &p, uint64_t shot, uint32_t q, uint32_t core, uint32_t t,
                                            uint32_t tag, uint32_t n, uint32_t &tl0, uint32_t &tl1, C32 &x0, C32 &x1,
                                            C32 &x2, C32 &x3)
{
    const uint32_t tl = q ? tl1 : tl0;
    if (t <= tl) return 0u;
    tl0 = q ? tl0 : t;
    tl1 = q ? t : tl1;
    const uint32_t *__restrict__ tab = p.decay + core * QSIM_DECAY_WORDS;
    uint32_t G = 1u << 30, E = 1u << 30;
    for (uint32_t m = t - tl; m; m &= m - 1u) {         // the set bits of dt, ascending
        const uint32_t i = (uint32_t)__ffs((int)m) - 1u;
        G = (uint32_t)(((uint64_t)G * tab[i] + (1u << 29)) >> 30);
        E = (uint32_t)(((uint64_t)E * tab[32u + i] + (1u << 29)) >> 30);
    }
    if (G == (1u << 30) && E == (1u << 30)) return 0u;  // nothing can happen: the draw is not observable
    const uint3 rr = philox3(p.seed, shot, tag | core, n);
    // the qubit's pairs are (x0, t1), (t2, x3): the first core's qubit trades x1 and x2
    C32 t1 = q ? x1 : x2, t2 = q ? x2 : x1;
    const C32 zero = {0, 0};
    uint32_t did = 0u;
    if (G < (1u << 30)) {
        const unsigned long long A = pop(t1) + pop(x3), T = pop(x0) + pop(t2) + A;
        const C32 y1 = scaled(G, t1), y3 = scaled(G, x3);
        const unsigned long long A2 = pop(y1) + pop(y3);
        const unsigned long long u = rr.x, v = u * (T >> 32) + ((u * (T & 0xFFFFFFFFull)) >> 32);
        const bool jump = v < A - A2;
        const unsigned long long Tn = jump ? A : T - A + A2;    // the sum of the new populations
        const int hi = 63 - __clzll((long long)Tn);
        const uint32_t s = (Tn == 0ull || hi >= 58) ? 0u : (uint32_t)(59 - hi) >> 1;
        x0 = shl(jump ? t1 : x0, s);
        t2 = shl(jump ? x3 : t2, s);
        t1 = jump ? zero : shl(y1, s);
        x3 = jump ? zero : shl(y3, s);
        did = jump ? 1u : 0u;
    }
    if (rr.y < ((1u << 30) - E) << 1) {
        t1 = neg(t1);
        x3 = neg(x3);
        did |= 2u;
    }
    x1 = q ? t1 : t2;
    x2 = q ? t2 : t1;
    return did;
}

template <bool MEAS, bool DECAY> __global__ void __launch_bounds__(BLOCK) qsim_kernel(const QsimParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t s_mem[];   // phase table, then the dictionary slots
    const uint32_t tid = threadIdx.x;
    const uint32_t row0 = blockIdx.x * BLOCK, row_last = min(row0 + BLOCK, p.n_rows) - 1u;
    // the registers of the workgroup's rows and their dictionary slots
    const uint32_t r_lo = fast_div(row0, p.ns_div), r_hi = fast_div(row_last, p.ns_div);
    const uint32_t sl_lo = p.tab[p.off_slot + r_lo], sl_hi = p.tab[p.off_slot + r_hi + 1u];
    for (uint32_t i = tid; i < QSIM_LUT_WORDS; i += BLOCK) s_mem[i] = p.tab[i];
    const uint32_t *__restrict__ dict = p.tab + p.off_dict + sl_lo * QSIM_SLOT_WORDS;
    const uint32_t n_dict = (sl_hi - sl_lo) * QSIM_SLOT_WORDS;
    for (uint32_t i = tid; i < n_dict; i += BLOCK) s_mem[QSIM_LUT_WORDS + i] = dict[i];
    __syncthreads();

    const uint32_t row = row0 + tid;
    if (row >= p.n_rows) return;
    const uint32_t r = fast_div(row, p.ns_div), sl = row - r * p.n_shots;
    const uint64_t shot = p.shot_begin + sl;
    const uint32_t c0 = p.tab[p.off_reg + 2u * r], c1 = p.tab[p.off_reg + 2u * r + 1u];
    const bool two = c1 != 0xFFFFFFFFu;
    const uint32_t slot0 = QSIM_LUT_WORDS + (p.tab[p.off_slot + r] - sl_lo) * QSIM_SLOT_WORDS;   // the first core's, in s_mem
    const uint32_t lane0 = p.shot_major ? sl * p.C + c0 : c0 * p.n_shots + sl;
    const uint32_t lane1 = !two ? lane0 : p.shot_major ? sl * p.C + c1 : c1 * p.n_shots + sl;
    const uint32_t ne0 = p.summary[(uint64_t)lane0 * 8u + 2u], ne1 = two ? p.summary[(uint64_t)lane1 * 8u + 2u] : 0u;
    const uint32_t n0 = min(ne0, p.event_cap), n1 = min(ne1, p.event_cap);
    const uint32_t det0 = p.tab[p.off_det + c0], det1 = two ? p.tab[p.off_det + c1] : 0u;

    C32 x0 = {1 << 30, 0}, x1 = {0, 0}, x2 = {0, 0}, x3 = {0, 0};
    uint32_t n_gates = 0, n_unmatched = 0, n_errors = 0;
    uint32_t nm0 = 0, nm1 = 0, st0 = 0, st1 = 0;        // MEAS: the lanes' readouts so far and their state bits
    uint32_t tl0 = 0, tl1 = 0, nj0 = 0, nf0 = 0, nj1 = 0, nf1 = 0;   // DECAY: the qubits' clocks, their jumps and flips
    auto tally = [&](uint32_t q, uint32_t did) {        // what an advance of qubit q did
        nj0 += q ? 0u : did & 1u;
        nf0 += q ? 0u : did >> 1;
        nj1 += q ? did & 1u : 0u;
        nf1 += q ? did >> 1 : 0u;
    };
    uint32_t k0 = 0, k1 = 0, hk0 = 0, hk1 = 0;          // the next record to look at / the head's slot
    uint4 h0 = make_uint4(0u, 0u, 0u, 0u), h1 = h0;     // the lanes' next drive strobes, when v0 / v1
    bool v0 = false, v1 = false;
    for (;;) {
        if (!v0 && k0 < n0) {
            h0 = p.events[(uint64_t)k0 * p.n_lanes + lane0];
            hk0 = k0++;
            v0 = strobe_of(h0.y, p.drv_elem) || (MEAS && strobe_of(h0.y, p.meas_elem));
        }
        if (!v1 && k1 < n1) {
            h1 = p.events[(uint64_t)k1 * p.n_lanes + lane1];
            hk1 = k1++;
            v1 = strobe_of(h1.y, p.drv_elem) || (MEAS && strobe_of(h1.y, p.meas_elem));
        }
        if ((!v0 && k0 < n0) || (!v1 && k1 < n1)) continue;   // a lane is still looking for its next kept strobe
        if (!v0 && !v1) break;
        const bool take0 = v0 && (!v1 || h0.x <= h1.x);
        const uint4 e = take0 ? h0 : h1;
        const uint32_t k = take0 ? hk0 : hk1, q = take0 ? 0u : 1u, core = take0 ? c0 : c1;
        v0 = take0 ? false : v0;
        v1 = take0 ? v1 : false;

        // ---- a readout strobe (element meas_elem; != drv_elem, the host checks) measures this core's qubit:
        // no lookup, no error draw ----
        if (MEAS && strobe_of(e.y, p.meas_elem)) {
            if constexpr (DECAY) tally(q, advance(p, shot, q, core, e.x, DECAY_OWN, k, tl0, tl1, x0, x1, x2, x3));
            const uint32_t m = q ? nm1 : nm0;
            const uint32_t b = measure(q, philox3(p.seed, shot, 0x10000000u | core, m).x, x0, x1, x2, x3);
            const uint32_t bit = m < 32u ? b << (m & 31u) : 0u;
            st0 |= q ? 0u : bit;
            st1 |= q ? bit : 0u;
            nm0 += 1u - q;
            nm1 += q;
            continue;
        }

        // ---- lookup in the emitting core's slot ----
        const uint32_t slot = slot0 + q * QSIM_SLOT_WORDS;
        const uint32_t freq = e.z >> 17, env = e.y & 0xFFFFFFu, amp = e.w & 0xFFFFu;
        uint32_t hit = DPEMU_QSIM_GATES_MAX;
#pragma unroll
        for (uint32_t i = 0; i < DPEMU_QSIM_GATES_MAX; i++) {
            const uint32_t g = slot + i * QSIM_GATE_WORDS;
            hit = (s_mem[g + 1u] == freq && s_mem[g + 2u] == env && s_mem[g + 3u] == amp) ? i : hit;
        }
        if (hit == DPEMU_QSIM_GATES_MAX) {
            n_unmatched++;
            continue;
        }
        n_gates++;
        const uint32_t g = slot + hit * QSIM_GATE_WORDS;
        const uint32_t kind = s_mem[g + 4u], err_thr = s_mem[g + 5u];
        if constexpr (DECAY) {                          // the emitting core's qubit (kind 1: the control), then the target
            tally(q, advance(p, shot, q, core, e.x, DECAY_OWN, k, tl0, tl1, x0, x1, x2, x3));
            if (kind) tally(1u, advance(p, shot, 1u, c1, e.x, DECAY_TARGET, k, tl0, tl1, x0, x1, x2, x3));
        }

        // ---- phase: the emitting core's frame, or for a controlled gate the target's ----
        const uint32_t det = (kind | q) ? det1 : det0;
        const uint32_t phi = ((e.z & 0x1FFFFu) + (uint32_t)(((uint64_t)det * e.x) >> 15)) & 0x1FFFFu;
        const uint32_t ic = 2u * (phi >> 8), jf = 2u * (DPEMU_QSIM_LUT_COARSE + (phi & 255u));
        const C32 w = cmulr(C32{(int32_t)s_mem[ic], (int32_t)s_mem[ic + 1u]}, C32{(int32_t)s_mem[jf], (int32_t)s_mem[jf + 1u]});
        const C32 wc = {w.re, -w.im};

        // ---- U(phi) = Rz(phi) M Rz(-phi) for the pair with control bit 0 (or both) / control bit 1 ----
        Gate2 ga, gb;
        {
            const uint32_t m = g + 6u;
            ga.a = C32{(int32_t)s_mem[m], (int32_t)s_mem[m + 1u]};
            ga.b = cmulr(C32{(int32_t)s_mem[m + 2u], (int32_t)s_mem[m + 3u]}, wc);
            ga.c = cmulr(C32{(int32_t)s_mem[m + 4u], (int32_t)s_mem[m + 5u]}, w);
            ga.d = C32{(int32_t)s_mem[m + 6u], (int32_t)s_mem[m + 7u]};
        }
        gb = ga;
        if (kind) {
            const uint32_t m = g + 14u;
            gb.a = C32{(int32_t)s_mem[m], (int32_t)s_mem[m + 1u]};
            gb.b = cmulr(C32{(int32_t)s_mem[m + 2u], (int32_t)s_mem[m + 3u]}, wc);
            gb.c = cmulr(C32{(int32_t)s_mem[m + 4u], (int32_t)s_mem[m + 5u]}, w);
            gb.d = C32{(int32_t)s_mem[m + 6u], (int32_t)s_mem[m + 7u]};
        }
        // the acted qubit's pairs are (x0, t1), (t2, x3): the first core's qubit trades x1 and x2
        const bool first = q == 0u && kind == 0u;
        C32 t1 = first ? x2 : x1, t2 = first ? x1 : x2;
        apply(ga, x0, t1);
        apply(gb, t2, x3);

        // ---- stochastic Pauli error after the gate ----
        if (err_thr) {
            const uint3 rr = philox3(p.seed, shot, 0x40000000u | core, k);
            if (rr.x < err_thr) {
                n_errors++;
                if (kind == 0u) {
                    const uint32_t code = 1u + __umulhi(rr.y, 3u);
                    pauli(code, x0, t1);
                    pauli(code, t2, x3);
                } else {                                // (kind 1: t1 = x1, t2 = x2)
                    const uint32_t idx = 1u + __umulhi(rr.y, 15u);
                    pauli(idx & 3u, x0, t1);            // the target: the second core's qubit
                    pauli(idx & 3u, t2, x3);
                    pauli(idx >> 2, x0, t2);            // the control: the first core's
                    pauli(idx >> 2, t1, x3);
                }
            }
        }
        x1 = first ? t2 : t1;
        x2 = first ? t1 : t2;
    }

    if constexpr (DECAY) {
        if (p.t_final) {
            tally(0u, advance(p, shot, 0u, c0, p.t_final, DECAY_FINAL, 0u, tl0, tl1, x0, x1, x2, x3));
            if (two) tally(1u, advance(p, shot, 1u, c1, p.t_final, DECAY_FINAL, 0u, tl0, tl1, x0, x1, x2, x3));
        }
        if (p.counts) reinterpret_cast<uint4 *>(p.counts)[row] = make_uint4(nj0, nf0, nj1, nf1);
    }

    // ---- populations and the sampled outcome ----
    const unsigned long long P0 = pop(x0), P1 = pop(x1), P2 = pop(x2), P3 = pop(x3);
    const unsigned long long T = P0 + P1 + P2 + P3;
    const unsigned long long u = philox3(p.seed, shot, 0x20000000u | c0, 0u).x;
    const unsigned long long v = u * (T >> 32) + ((u * (T & 0xFFFFFFFFull)) >> 32);
    const uint32_t j = (P0 <= v ? 1u : 0u) + (P0 + P1 <= v ? 1u : 0u) + (P0 + P1 + P2 <= v ? 1u : 0u);
    unsigned long long *out = p.pops + (uint64_t)row * 4u;
    out[0] = P0;
    out[1] = P1;
    out[2] = P2;
    out[3] = P3;
    const uint32_t ovf = (ne0 > p.event_cap || ne1 > p.event_cap) ? 0x80000000u : 0u;
    p.result[row] = make_uint4((j >> 1) | ((j & 1u) << 1), n_gates, n_unmatched, (n_errors & 0xFFFFu) | ovf);
    if (MEAS) {
        p.states[lane0] = st0;
        if (two) p.states[lane1] = st1;
    }
}

hipError_t launch_qsim(const QsimParams &p, hipStream_t stream)
{
    const dim3 grid((p.n_rows + BLOCK - 1u) / BLOCK);
    if (p.decay && p.meas)
        hipLaunchKernelGGL((qsim_kernel<true, true>), grid, dim3(BLOCK), p.lds_bytes, stream, p);
    else if (p.decay)
        hipLaunchKernelGGL((qsim_kernel<false, true>), grid, dim3(BLOCK), p.lds_bytes, stream, p);
    else if (p.meas)
        hipLaunchKernelGGL((qsim_kernel<true, false>), grid, dim3(BLOCK), p.lds_bytes, stream, p);
    else
        hipLaunchKernelGGL((qsim_kernel<false, false>), grid, dim3(BLOCK), p.lds_bytes, stream, p);
    return hipGetLastError();
}

}  // namespace dpemu
