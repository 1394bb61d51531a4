// q15.h -- packed int16 arithmetic shared by the sample-level kernels
// (dds.hip, demod_iq.hip, feedline.hip, resonator.hip, traces.hip): complex Q15 products as
// v_dot2_i32_i16 pairs, and the 16-byte group of four sample words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dpemu {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));   // four I16|Q16 words: one 16-B load or store

// a.lo * b.lo + a.hi * b.hi + c on packed int16 pairs: one VOP3P
// v_dot2_i32_i16 with the rounding constant in an SGPR
__device__ __forceinline__ int32_t dot2(uint32_t a, uint32_t b, int32_t c)
{
    int32_t r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(c));
    return r;
}

// the same with a per-lane addend (a VGPR); the sum is taken mod 2^32
__device__ __forceinline__ int32_t dot2v(uint32_t a, uint32_t b, int32_t c)
{
    int32_t r;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// P = a conj(lo) of two I16|Q16 words (feedline_demod_kernel, feedline_trace_kernel): {P_I - 1, P_Q} with
// P_I = a_I lo_I + a_Q lo_Q, P_Q = a_Q lo_I - a_I lo_Q, for EVERY int16 half: a caller's trace and an LO row may
// hold -32768, which a 16-bit negation (neg_swap) does not survive.
//   P_I reaches 2^31 at four halves of -32768; P_I - 1 lies in [-2^31 + 65535, 2^31 - 1], so the addend is -1
//     and the caller puts the 1 back into its 64-bit sum (a masked sample, lo = 0, gives -1 + 1 too)
//   P_Q = a_Q lo_I + a_I ~lo_Q + a_I, as ~x = -x - 1 has no exception; taken mod 2^32 the sum is P_Q itself,
//     which fits int32 (|P_Q| <= 2^31 - 32768); a masked lo gives -a_I + a_I
__device__ __forceinline__ int2 mix_conj_m1(uint32_t a, uint32_t lo)
{
    return make_int2(dot2(a, lo, -1),
                     dot2v(__builtin_amdgcn_alignbit(a, a, 16), lo ^ 0xFFFF0000u, (int32_t)(int16_t)(a & 0xFFFFu)));
}

// {lo[15:0], hi[15:0]} in one v_perm_b32
__device__ __forceinline__ uint32_t pack16(int32_t lo, int32_t hi)
{
    return __builtin_amdgcn_perm((uint32_t)hi, (uint32_t)lo, 0x05040100u);
}

typedef short short2v __attribute__((ext_vector_type(2)));

// {lo: hi, hi: -lo} of an I16|Q16 word
__device__ __forceinline__ uint32_t neg_swap(uint32_t w) { return (w >> 16) | (((0u - w) & 0xFFFFu) << 16); }

// dot2 results (+2^14) >> 15 of two components -> {lo, hi} saturated to int16
__device__ __forceinline__ uint32_t pk_sat(int32_t lo, int32_t hi)
{
    return __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_pk_i16(lo >> 15, hi >> 15));
}

// each half of a packed int16 pair raised to at least -32767 (symsat after pk_sat)
__device__ __forceinline__ uint32_t pk_symfloor(uint32_t w)
{
    const short2v lo = {-32767, -32767};
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(short2v, w), lo));
}

}  // namespace dpemu
