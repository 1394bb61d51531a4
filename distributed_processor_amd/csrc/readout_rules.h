// readout_rules.h -- the integer rules of the readout model, once each, for host and device: include/dpemu.h
// states them (dpemu_config's DEMOD model, dpemu_demod_iq, dpemu_feedline_adc; that text is normative), the
// interpreters' readout models (lane.h), the readout stages (demod_iq.hip, feedline.hip, resonator.hip,
// traces.hip, iq_stats.hip) and qsim.hip evaluate them through these functions.  Plain integer arithmetic over
// uop.h: nothing from HIP and no device intrinsic, only the compilers' __builtin_ctz
// (tests/readout_rules_test.cpp builds it with g++).
#pragma once

#include <stdint.h>

#include "../../include/dpemu.h"
#include "uop.h"

// always inlined, as the kernels' own __forceinline__ helpers are
#define RO_RULE DPEMU_HD inline __attribute__((always_inline))

namespace dpemu {

// a strobe event of element `elem`, from the record's word 1 (env[23:0] cfg[27:24] kind[31:28])
RO_RULE bool strobe_of(uint32_t word1, uint32_t elem)
{
    return (word1 >> 28) == DPEMU_EV_STROBE && ((word1 >> 24) & 3u) == elem;
}

// "state": the prepared state from Philox word 0 and the core's p1 threshold
RO_RULE bool ro_state(uint32_t word0, uint32_t thr) { return (thr == 0xFFFFFFFFu) || (word0 < thr); }

// env length field (bits 23:12) in env words, 0 (a CW envelope) = 4096
RO_RULE uint32_t ro_words(uint32_t env) { const uint32_t L = (env >> 12) & 0xFFFu; return L ? L : 4096u; }

// "window": the LO samples [j0, j1) of a readout strobe at clock t_lo with env word pe on a row of
// n_samples_lo samples, sh_lo = log2 spc_lo; j0 == j1: nothing of the window is inside the row
struct RoWindow {
    uint32_t j0, j1;
};
RO_RULE RoWindow ro_window(uint32_t t_lo, uint32_t pe, uint32_t sh_lo, uint32_t ro_cpw, uint32_t n_samples_lo)
{
    const uint64_t w0 = (uint64_t)t_lo << sh_lo;
    const uint64_t w1 = w0 + ((uint64_t)(ro_words(pe) * ro_cpw) << sh_lo);
    const uint64_t n = n_samples_lo;
    return RoWindow{(uint32_t)(w0 < n ? w0 : n), (uint32_t)(w1 < n ? w1 : n)};
}

// "ADC": the drive-row sample under LO sample j = n spc_lo + k, (n - ro_delay) spc_drv + k (spc_drv / spc_lo);
// !ok (the sample reads 0) when n < ro_delay or the index is past the row.  spc_lo is a power of two and
// spc_drv a multiple of it (stage_plan.h describe_pairs)
struct AdcIndex {
    uint64_t i;
    bool ok;
};
RO_RULE AdcIndex adc_index(uint32_t j, uint32_t spc_drv, uint32_t spc_lo, uint32_t ro_delay, uint32_t n_samples_drv)
{
    const uint32_t n = j >> __builtin_ctz(spc_lo), k = j & (spc_lo - 1u);
    const uint64_t i = (uint64_t)(n - ro_delay) * spc_drv + k * (spc_drv / spc_lo);
    return AdcIndex{i, n >= ro_delay && i < n_samples_drv};
}

// "noise": z_I, z_Q, the Hadamard pairs of the 16-bit halves of Philox words 1 and 2 (each in [-131070,
// 131070]), and a component's share (z sigma) >> 16 (a floor shift)
struct RoNoise {
    int64_t zi, zq;
};
RO_RULE RoNoise ro_noise_pair(uint32_t word1, uint32_t word2)
{
    const int32_t u0 = (int32_t)(word1 & 0xFFFFu), u1 = (int32_t)(word1 >> 16);
    const int32_t u2 = (int32_t)(word2 & 0xFFFFu), u3 = (int32_t)(word2 >> 16);
    return RoNoise{u0 + u1 - u2 - u3, u0 - u1 + u2 - u3};
}
RO_RULE int64_t ro_noise(int64_t z, uint32_t sigma) { return (z * (int64_t)sigma) >> 16; }

// "return": the Q15 sine table's entry i of a return phase ro_theta; (c, s_) = (lut[(i + 1024) & 4095], lut[i])
RO_RULE uint32_t ro_theta_index(uint32_t theta) { return ((theta + (1u << 19)) >> 20) & 4095u; }

// "m_p(n)": the state of a feedline member at a clock by which `seen` of its kept readouts have begun, from
// its state bits (readout m's in bit m; a member without a readout uses draw 0)
RO_RULE uint32_t ro_member_state(uint32_t bits, uint32_t seen) { return (bits >> ((seen > 1u ? seen : 1u) - 1u)) & 1u; }

// the discriminator on an accumulated {I, Q}: x = (acc_I axis_I + acc_Q axis_Q) >> 15 > thr, ax = the
// core's Q15 axis I | Q << 16
RO_RULE uint32_t demod_decide(int32_t acc_i, int32_t acc_q, uint32_t ax, int32_t thr)
{
    const int64_t x = ((int64_t)acc_i * (int16_t)(ax & 0xFFFFu) + (int64_t)acc_q * (int16_t)(ax >> 16)) >> 15;
    return x > (int64_t)thr;
}

}  // namespace dpemu

#undef RO_RULE
