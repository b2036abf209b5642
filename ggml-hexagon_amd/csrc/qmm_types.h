// qmm_types.h — the weight type ids and the run-time views of the type table.  Plain C++ (no HIP): qmm_device.hiph includes it for
// the kernels, qmm_prefill_plan.h and qmm_matvec_plan.h for the host-side launch plans, and a host compiler alone can read both.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define QMM_HD __host__ __device__
#else
#define QMM_HD
#endif

namespace qmm {

enum : int { T_Q4_0 = 2, T_Q4_1 = 3, T_Q5_0 = 6, T_Q5_1 = 7, T_Q8_0 = 8, T_Q8_1 = 9, T_Q2_K = 10, T_Q3_K = 11, T_Q4_K = 12, T_Q5_K = 13,
             T_Q6_K = 14, T_Q8_K = 15, T_IQ4_NL = 20, T_IQ4_XS = 23,
             // the 3-bit i-quants: their grids are not in this source; qmm_set_codebook hands them to a context at run time
             T_IQ3_XXS = 18, T_IQ3_S = 21,
             // the 2-bit i-quants with two scales per 32 weights: eight weights per grid entry, the same run-time codebooks
             T_IQ2_XS = 17, T_IQ2_S = 22,
             // the 1-bit i-quants: eight ternary weights per index into one grid both formats share, handed over the same way
             T_IQ1_S = 19, T_IQ1_M = 29,
             // the ternary formats of BitNet / TriLM files: no table, TQ1_0 five trits per byte (decoded by a multiply), TQ2_0 two bits per weight
             T_TQ1_0 = 34, T_TQ2_0 = 35,
             // the same blocks with every row re-laid as aligned planes (qmm_repack_rows; the bytes of a row stay in the row):
             //   Q4_0P  [d: nb x 2 B][qs: nb x 16 B]           K % 256 == 0  (the d plane is a multiple of 16 bytes)
             //   Q8_0P  [d: nb x 2 B][qs: nb x 32 B]           K % 256 == 0
             //   Q6_KP  [ql: nb x 128][qh: nb x 64][scales: nb x 16][d: nb x 2]     K % 2048 == 0 (row stride a multiple of 16)
             // so that a lane's 16-byte loads are 16-byte aligned (18-, 34- and 210-byte blocks put them at 2-byte alignment)
             T_Q4_0P = 102, T_Q8_0P = 108, T_Q6_KP = 114 };
QMM_HD constexpr int type_base(int t) { return t >= 100 ? t - 100 : t; }
QMM_HD inline bool type_planar(int t) { return t >= 100; }

// run-time views of the type table (host and device)
QMM_HD inline bool type_known(int t) {
    if (t == T_Q4_0P || t == T_Q8_0P || t == T_Q6_KP) return true;
    return t == T_Q4_0 || t == T_Q4_1 || t == T_Q5_0 || t == T_Q5_1 || t == T_Q8_0 || t == T_Q2_K || t == T_Q3_K || t == T_Q4_K || t == T_Q5_K ||
           t == T_Q6_K || t == T_IQ4_NL || t == T_IQ4_XS || t == T_IQ3_XXS || t == T_IQ3_S || t == T_IQ2_XS || t == T_IQ2_S || t == T_IQ1_S || t == T_IQ1_M ||
           t == T_TQ1_0 || t == T_TQ2_0;
}
// types whose values come out of a codebook set per context: 32-bit words of the table, 0 for every other type (IQ3: one word = one
// entry of four magnitudes; IQ2: words 2e and 2e + 1 = entry e of eight; IQ1_S and IQ1_M: one table of 2048 such word pairs, int8 -1 / 0 / +1)
QMM_HD constexpr int type_codebook(int t) { return t == T_IQ3_XXS ? 256 : t == T_IQ3_S ? 512 : t == T_IQ2_XS ? 1024 : t == T_IQ2_S ? 2048 : (t == T_IQ1_S || t == T_IQ1_M) ? 4096 : 0; }
QMM_HD constexpr bool type_ternary(int t) { return t == T_IQ1_S || t == T_IQ1_M; }
// IQ1_M's 56-byte blocks hold four u16 of scales that a lane reads as one 8-byte word (block_iq1_m is 8-byte aligned in ggml too):
// the base address and every stride between rows (and experts) must be multiples of 8
QMM_HD inline bool iq1m_misaligned(int t, const void * w, int64_t row_bytes, int64_t plane_bytes = 0) {
    return t == T_IQ1_M && ((uintptr_t) w % 8 || row_bytes % 8 || plane_bytes % 8);
}
QMM_HD constexpr int type_blck(int t) { t = type_base(t); return (t == T_Q2_K || t == T_Q3_K || t == T_Q4_K || t == T_Q5_K || t == T_Q6_K || t == T_IQ4_XS || t == T_IQ3_XXS || t == T_IQ3_S || t == T_IQ2_XS || t == T_IQ2_S || t == T_IQ1_S || t == T_IQ1_M || t == T_TQ1_0 || t == T_TQ2_0) ? 256 : 32; }
QMM_HD inline int type_tsize(int t) {
    switch (type_base(t)) {
        case T_Q4_0: return 18; case T_Q4_1: return 20; case T_Q5_0: return 22; case T_Q5_1: return 24; case T_Q8_0: return 34; case T_IQ4_NL: return 18;
        case T_IQ4_XS: return 136; case T_IQ3_XXS: return 98; case T_IQ3_S: return 110; case T_IQ2_XS: return 74; case T_IQ2_S: return 82; case T_IQ1_S: return 50; case T_IQ1_M: return 56; case T_TQ1_0: return 54; case T_TQ2_0: return 66; case T_Q2_K: return 84; case T_Q3_K: return 110; case T_Q4_K: return 144; case T_Q5_K: return 176; case T_Q6_K: return 210; default: return 0;
    }
}
// activation format the CPU backend dots the type against (type_traits_cpu[].vec_dot_type, ggml-cpu.c:256-...)
QMM_HD constexpr int type_act(int t) { t = type_base(t); return type_blck(t) == 256 ? T_Q8_K : (t == T_Q4_1 || t == T_Q5_1) ? T_Q8_1 : T_Q8_0; }

} // namespace qmm
