// CPU driver of the readout model's integer rules (csrc/readout_rules.h) and of the pair descriptor's word
// names (csrc/uop.h), built and run by tests/test_readout_rules.py with g++.  Every expected value is worked
// out by hand from the text of include/dpemu.h (dpemu_config's DEMOD model, dpemu_demod_iq,
// dpemu_feedline_adc) and written out here; none comes from the functions under test.  Prints
// "ok <checks>" and returns 0, or the first failed check.
#include <cstdint>
#include <cstdio>

#include "../distributed_processor_amd/csrc/readout_rules.h"

using namespace dpemu;

static int n_checks = 0;
#define CHECK(...)                                                         \
    do {                                                                   \
        n_checks++;                                                        \
        if (!(__VA_ARGS__)) { std::printf("line %d: %s\n", __LINE__, #__VA_ARGS__); return 1; } \
    } while (0)

static bool window_is(uint32_t t_lo, uint32_t pe, uint32_t sh_lo, uint32_t ro_cpw, uint32_t n_lo, uint32_t j0, uint32_t j1)
{
    const RoWindow w = ro_window(t_lo, pe, sh_lo, ro_cpw, n_lo);
    if (w.j0 != j0 || w.j1 != j1) std::printf("window [%u, %u), expected [%u, %u)\n", w.j0, w.j1, j0, j1);
    return w.j0 == j0 && w.j1 == j1;
}

// the sample reads drive index i
static bool adc_is(uint32_t j, uint32_t spc_drv, uint32_t spc_lo, uint32_t ro_delay, uint32_t n_drv, uint64_t i)
{
    const AdcIndex a = adc_index(j, spc_drv, spc_lo, ro_delay, n_drv);
    if (!a.ok || a.i != i) std::printf("adc index %llu ok %d, expected %llu\n", (unsigned long long)a.i, (int)a.ok, (unsigned long long)i);
    return a.ok && a.i == i;
}
// the sample reads 0
static bool adc_zero(uint32_t j, uint32_t spc_drv, uint32_t spc_lo, uint32_t ro_delay, uint32_t n_drv)
{
    return !adc_index(j, spc_drv, spc_lo, ro_delay, n_drv).ok;
}

static bool noise_is(uint32_t word1, uint32_t word2, int64_t zi, int64_t zq)
{
    const RoNoise z = ro_noise_pair(word1, word2);
    if (z.zi != zi || z.zq != zq) std::printf("z = (%lld, %lld), expected (%lld, %lld)\n", (long long)z.zi, (long long)z.zq, (long long)zi, (long long)zq);
    return z.zi == zi && z.zq == zq;
}

int main()
{
    // ---- the pair descriptor: lane, core, shot (low, high), drv_row, lo_row, spc_drv, spc_lo, p1 threshold, axis ----
    {
        const uint32_t d[DEMOD_PAIR_WORDS] = {100, 101, 0x89ABCDEFu, 0x01234567u, 104, 105, 106, 107, 108, 109};
        CHECK(DEMOD_PAIR_WORDS == 10);
        CHECK(d[PAIR_LANE] == 100 && d[PAIR_CORE] == 101 && d[PAIR_SHOT_LO] == 0x89ABCDEFu && d[PAIR_SHOT_HI] == 0x01234567u);
        CHECK(d[PAIR_DRV_ROW] == 104 && d[PAIR_LO_ROW] == 105 && d[PAIR_SPC_DRV] == 106 && d[PAIR_SPC_LO] == 107);
        CHECK(d[PAIR_P1_THR] == 108 && d[PAIR_AXIS] == 109);
        CHECK(pair_shot(d) == 0x0123456789ABCDEFull);
    }

    // ---- a strobe of an element: kind (bits 31:28) STROBE = 0 and cfg (bits 27:24) & 3 == elem ----
    CHECK(strobe_of(0x06123456u, 2));                   // cfg 6: element 2
    CHECK(!strobe_of(0x06123456u, 1) && !strobe_of(0x06123456u, 0) && !strobe_of(0x06123456u, 3));
    CHECK(!strobe_of(0x16123456u, 2));                  // a pulse_reset record
    CHECK(strobe_of(0x00FFFFFFu, 0) && strobe_of(0x0FFFFFFFu, 3) && !strobe_of(0xF3000000u, 3));

    // ---- W = env bits 23:12, 0 = 4096 ----
    CHECK(ro_words(0x00000ABCu) == 4096);               // field 0 (the low 12 bits are not the field)
    CHECK(ro_words(0x00000000u) == 4096);
    CHECK(ro_words(0x00FFF000u) == 4095);
    CHECK(ro_words(0xFF001FFFu) == 1);                  // bits above 23 are not the field either
    CHECK(ro_words(0x003E8000u) == 1000);

    // ---- window: clocks [t_lo, t_lo + W ro_cpw), LO samples n spc_lo + k of them, clipped to n_samples_lo ----
    // W = 3, ro_cpw = 4: clocks [10, 22)
    const uint32_t pe3 = 3u << 12;
    CHECK(window_is(10, pe3, 0, 4, 64, 10, 22));        // spc_lo 1: inside the row
    CHECK(window_is(10, pe3, 0, 4, 16, 10, 16));        //   clipped
    CHECK(window_is(16, pe3, 0, 4, 16, 16, 16));        //   begins at the row's end: empty
    CHECK(window_is(100, pe3, 0, 4, 16, 16, 16));       //   begins past it: empty
    CHECK(window_is(10, pe3, 2, 4, 128, 40, 88));       // spc_lo 4
    CHECK(window_is(10, pe3, 2, 4, 64, 40, 64));
    CHECK(window_is(16, pe3, 2, 4, 64, 64, 64));
    CHECK(window_is(17, pe3, 2, 4, 64, 64, 64));
    CHECK(window_is(10, pe3, 4, 4, 512, 160, 352));     // spc_lo 16
    CHECK(window_is(10, pe3, 4, 4, 256, 160, 256));
    CHECK(window_is(16, pe3, 4, 4, 256, 256, 256));
    CHECK(window_is(4000, pe3, 4, 4, 256, 256, 256));
    CHECK(window_is(10, pe3, 4, 4, 352, 160, 352));     // ends exactly at the row's end
    CHECK(window_is(0, 0x00000123u, 0, 1, 8192, 0, 4096));   // a CW envelope: 4096 words
    CHECK(window_is(0, 0x00FFF000u, 0, 31, 200000, 0, 126945));   // 4095 words of 31 clocks
    // t_lo << sh past 2^32: the window lies past any row, it does not wrap to the row's start
    CHECK(window_is(0x40000000u, pe3, 2, 4, 0xFFFFFFFCu, 0xFFFFFFFCu, 0xFFFFFFFCu));
    CHECK(window_is(0xFFFFFFFFu, pe3, 4, 4, 1024, 1024, 1024));
    CHECK(window_is(0x80000001u, pe3, 1, 4, 64, 64, 64));
    // the window's end past 2^32 alone: [2^32 - 16, 2^32 - 16 + 4096 * 4) clipped
    CHECK(window_is(0xFFFFFFF0u, 0, 0, 4, 0xFFFFFFFCu, 0xFFFFFFF0u, 0xFFFFFFFCu));

    // ---- ADC: LO sample j = n spc_lo + k reads drive index (n - ro_delay) spc_drv + k (spc_drv / spc_lo),
    // or 0 when n < ro_delay or the index is >= n_samples_drv ----
    // 16 : 4, ro_delay 3, a row of 64
    CHECK(adc_zero(0, 16, 4, 3, 64) && adc_zero(11, 16, 4, 3, 64));     // clocks 0 and 2
    CHECK(adc_is(12, 16, 4, 3, 64, 0));                 // n == ro_delay, k = 0
    CHECK(adc_is(13, 16, 4, 3, 64, 4) && adc_is(15, 16, 4, 3, 64, 12));
    CHECK(adc_is(22, 16, 4, 3, 64, 40));                // n = 5, k = 2
    CHECK(adc_is(27, 16, 4, 3, 64, 60));                // n = 6, k = 3: the last index the gather reaches
    CHECK(adc_zero(28, 16, 4, 3, 64));                  // index 64
    CHECK(adc_is(27, 16, 4, 3, 61, 60) && adc_zero(27, 16, 4, 3, 60));
    // 4 : 4, ro_delay 2, a row of 10
    CHECK(adc_zero(7, 4, 4, 2, 10));
    CHECK(adc_is(8, 4, 4, 2, 10, 0) && adc_is(11, 4, 4, 2, 10, 3));
    CHECK(adc_is(17, 4, 4, 2, 10, 9));                  // n = 4, k = 1
    CHECK(adc_zero(18, 4, 4, 2, 10));
    // 1 : 1, ro_delay 5, a row of 7
    CHECK(adc_zero(4, 1, 1, 5, 7));
    CHECK(adc_is(5, 1, 1, 5, 7, 0) && adc_is(11, 1, 1, 5, 7, 6));
    CHECK(adc_zero(12, 1, 1, 5, 7));
    CHECK(adc_is(0, 1, 1, 0, 7, 0));                    // no delay: sample 0 reads index 0
    // 16 : 2 and 8 : 8
    CHECK(adc_is(9, 16, 2, 1, 1000, 56));               // n = 4, k = 1: 3 * 16 + 8
    CHECK(adc_is(21, 8, 8, 0, 1000, 21));
    // the index is 64-bit: 2^29 clocks of 16 samples
    CHECK(adc_index(0x20000000u, 16, 1, 0, 0xFFFFFFFFu).i == 0x200000000ull && adc_zero(0x20000000u, 16, 1, 0, 0xFFFFFFFFu));

    // ---- state: Philox word 0 < p1_threshold, or a threshold of 0xFFFFFFFF ----
    CHECK(!ro_state(0, 0) && !ro_state(5, 0) && !ro_state(0xFFFFFFFFu, 0));             // thr 0: never
    CHECK(ro_state(0, 0xFFFFFFFFu) && ro_state(0xFFFFFFFFu, 0xFFFFFFFFu));              // thr 2^32 - 1: always
    CHECK(ro_state(99, 100) && !ro_state(100, 100) && !ro_state(101, 100));             // word0 == thr: 0
    CHECK(ro_state(0xFFFFFFFDu, 0xFFFFFFFEu) && !ro_state(0xFFFFFFFEu, 0xFFFFFFFEu) && !ro_state(0xFFFFFFFFu, 0xFFFFFFFEu));

    // ---- noise: halves u0 u1 of word 1 and u2 u3 of word 2 (low half first); z_I = u0 + u1 - u2 - u3,
    // z_Q = u0 - u1 + u2 - u3; a component's share floor(z sigma / 2^16) ----
    CHECK(noise_is(0xFFFFFFFFu, 0x00000000u, 131070, 0));
    CHECK(noise_is(0x00000000u, 0xFFFFFFFFu, -131070, 0));
    CHECK(noise_is(0x0000FFFFu, 0x0000FFFFu, 0, 131070));
    CHECK(noise_is(0xFFFF0000u, 0xFFFF0000u, 0, -131070));
    CHECK(noise_is(0x00030001u, 0x00100007u, -19, -11));   // 1 + 3 - 7 - 16, 1 - 3 + 7 - 16
    CHECK(noise_is(0u, 0u, 0, 0) && noise_is(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0));
    CHECK(ro_noise(19, 32768) == 9 && ro_noise(-19, 32768) == -10);     // +-9.5: the floor, not toward zero
    CHECK(ro_noise(-1, 1) == -1 && ro_noise(1, 1) == 0 && ro_noise(-1, 0) == 0);
    CHECK(ro_noise(-19, 65536) == -19 && ro_noise(131070, 65536) == 131070);
    // the largest magnitudes: -131070 (2^32 - 1) = -131070 2^32 + 131070 -> -131070 2^16 + 1
    CHECK(ro_noise(-131070, 0xFFFFFFFFu) == -8589803519ll && ro_noise(131070, 0xFFFFFFFFu) == 8589803518ll);

    // ---- return: sine-table entry ((ro_theta + 2^19) >> 20) & 4095 ----
    CHECK(ro_theta_index(0) == 0 && ro_theta_index(1u << 20) == 1 && ro_theta_index(0x40000000u) == 1024);
    CHECK(ro_theta_index((1u << 19) - 1) == 0 && ro_theta_index(1u << 19) == 1);       // rounds to nearest
    CHECK(ro_theta_index(0xFFF7FFFFu) == 4095 && ro_theta_index(0xFFF80000u) == 0);    // and wraps
    CHECK(ro_theta_index(0xFFFFFFFFu) == 0 && ro_theta_index(0x80000000u) == 2048);

    // ---- m_p(n) = max(#kept readouts at or before the clock, 1) - 1 picks the state bit ----
    CHECK(ro_member_state(0x5u, 0) == 1 && ro_member_state(0x5u, 1) == 1);             // none yet: draw 0, as the first
    CHECK(ro_member_state(0x5u, 2) == 0 && ro_member_state(0x5u, 3) == 1 && ro_member_state(0x5u, 4) == 0);
    CHECK(ro_member_state(0xFFFFFFFEu, 0) == 0 && ro_member_state(0xFFFFFFFEu, 1) == 0 && ro_member_state(0xFFFFFFFEu, 2) == 1);
    CHECK(ro_member_state(0x80000000u, 32) == 1 && ro_member_state(0x80000000u, 31) == 0);
    CHECK(ro_member_state(0x7FFFFFFFu, 32) == 0 && ro_member_state(0x7FFFFFFFu, 31) == 1);

    // ---- discriminator: x = (acc_I axis_I + acc_Q axis_Q) >> 15 > ro_thr, axis halves signed Q15 ----
    // axis (-32768, 0): x = -acc_I = 7
    CHECK(demod_decide(-7, 123, 0x00008000u, 7) == 0);  // x == thr
    CHECK(demod_decide(-7, 123, 0x00008000u, 6) == 1);  // x == thr + 1
    CHECK(demod_decide(-7, 123, 0x00008000u, 8) == 0);
    // axis (16384, -16384): (10 * 16384 - 4 * 16384) >> 15 = 3
    CHECK(demod_decide(10, 4, 0xC0004000u, 3) == 0 && demod_decide(10, 4, 0xC0004000u, 2) == 1);
    // axis (0, -1): (-(5) ) >> 15 = -1 (floor), so -1 > -2 only
    CHECK(demod_decide(99, 5, 0xFFFF0000u, -1) == 0 && demod_decide(99, 5, 0xFFFF0000u, -2) == 1);
    // 64-bit: -2^31 * -32768 >> 15 = 2^31 exceeds every int32 threshold
    CHECK(demod_decide(INT32_MIN, 0, 0x00008000u, INT32_MAX) == 1);
    CHECK(demod_decide(INT32_MAX, 0, 0x00008000u, INT32_MIN) == 1 && demod_decide(INT32_MIN, 0, 0x00007FFFu, INT32_MIN) == 1);
    CHECK(demod_decide(0, 0, 0x7FFF7FFFu, 0) == 0 && demod_decide(0, 0, 0x7FFF7FFFu, -1) == 1);

    std::printf("ok %d\n", n_checks);
    return 0;
}
