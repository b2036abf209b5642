// qmm_q8x_split.h — the integer helper of the Q8-exact prefill mode (QMM_PREC_Q8_EXACT, qmm_mfma_q8x.hiph): a K-quant weight q times its
// integer sub-block scale sc, v = sc * q, is cut into two int8 planes v = 128 * hi + lo with lo in [0, 127] (floor division), so that
// two int8 MFMA accumulations over a whole 256-element superblock give sum(v * q8) = (hi_acc << 7) + lo_acc with no rescale in between.
//   Q4_K  sc 0..63,     q 0..15     v 0..945         hi 0..7
//   Q5_K  sc 0..63,     q 0..31     v 0..1953        hi 0..15
//   Q6_K  sc -128..127, q -32..31   v -4064..4096    hi -32..32
//   Q3_K  sc -32..31,   q -4..3     v -124..128      hi -1..1
//   IQ4_XS sc -32..31,  q -127..113 v -3937..4064    hi -31..31     (q = kvalues_iq4nl[index])
//   Q2_K  sc 0..15,     q 0..3      v 0..45          one plane, no split (q8x_plane1)
// |v| <= 4096 for all of them, so a superblock's sum over 256 products with |q8| <= 127 stays below 2^27.
// Plain C++ on gcc / clang vector extensions (two 16-bit lanes in a register: v_pk_mul_lo_u16 / v_pk_ashrrev_i16 on gfx950), so that a
// host compiler alone can enumerate every (sc, q) pair (tests/test_q8_exact_host.py, tests/test_q8_exact_more_host.py).
#pragma once

#include "qmm_types.h"

namespace qmm {

typedef short q8x_s2 __attribute__((vector_size(4)));      // two int16

QMM_HD inline q8x_s2 q8x_as_s2(uint32_t u) { q8x_s2 v; __builtin_memcpy(&v, &u, 4); return v; }
QMM_HD inline uint32_t q8x_as_u32(q8x_s2 v) { uint32_t u; __builtin_memcpy(&u, &v, 4); return u; }

// two products: hi = floor(v / 128), lo = v - 128 * hi
QMM_HD inline void q8x_split(q8x_s2 q, short sc, q8x_s2 & hi, q8x_s2 & lo) {
    const q8x_s2 v = q * sc;
    hi = v >> 7;
    lo = v & (short) 127;
}

// Four weights as the bytes of `q` (unsigned, byte j = weight j; the format's offset `bias` is taken off here: 32 for Q6_K, else 0) times
// one scale: byte j of `hi` / `lo` = the int8 halves of sc * (q_j - bias), in the same byte order.
QMM_HD inline void q8x_planes(uint32_t q, short bias, short sc, uint32_t & hi, uint32_t & lo) {
    const q8x_s2 e = q8x_as_s2(q & 0x00FF00FFu) - bias, o = q8x_as_s2((q >> 8) & 0x00FF00FFu) - bias;      // weights 0, 2 and 1, 3
    q8x_s2 he, le, ho, lo2;
    q8x_split(e, sc, he, le);
    q8x_split(o, sc, ho, lo2);
    lo = q8x_as_u32(le) | (q8x_as_u32(lo2) << 8);                                                            // lo < 128: nothing to mask
    hi = (q8x_as_u32(he) & 0x00FF00FFu) | ((q8x_as_u32(ho) & 0x00FF00FFu) << 8);
}

// ... four weights that already are signed bytes (IQ4_XS: the bytes of kvalues_iq4nl)
QMM_HD inline void q8x_planes_s8(uint32_t q, short sc, uint32_t & hi, uint32_t & lo) { q8x_planes(q ^ 0x80808080u, 128, sc, hi, lo); }

// Four weights of 0..3 (Q2_K) times one scale of 0..15: byte j = sc * q_j <= 45, one int8 plane as it is
QMM_HD inline uint32_t q8x_plane1(uint32_t q, uint32_t sc) { return q * sc; }

} // namespace qmm
