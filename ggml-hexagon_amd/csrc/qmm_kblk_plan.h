// qmm_kblk_plan.h — the launch plan of what a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 adds (qmm_kblk.hiph; llama.cpp's -ctk q4_0 / q4_1 / q5_0 /
// q5_1 without flash attention): which operands the entry points take with a tensor of one of these types among them (CPY f32 -> type,
// CPY type -> f32 / f16, qmm_attn_decode / qmm_attn_prefill with k in the type), and for operands they take which kernel runs with which
// grid, block and LDS bytes, under which trace label.  Plain C++ (no HIP, no ggml; a host compiler alone reads it), built on
// qmm_kcache_plan.h: the attention limits, the cut of a long cache, the static LDS budget and the scratch cap are the Q8_0 K cache's, and
// that header's tables stay as they are.  The kernels take their constants from here; the host side in qmm_kblk.hiph executes a plan and
// decides nothing.
// V stays the transposed F16 cache; a quantized V, IQ4_NL (whose quantizer is a search) and D = 256 are outside this surface.
#pragma once

#include "qmm_kcache_plan.h"

namespace qmm {

enum : int { G_Q4_0 = 2, G_Q4_1 = 3, G_Q5_0 = 6, G_Q5_1 = 7 };
constexpr int KBLK_QK = 32;                      // values per block of all four types

// block_q4_0 / q4_1 / q5_0 / q5_1 (ggml-common.h): f16 d, [f16 m], [4 bytes qh], 16 bytes of nibbles (byte j: element j low, j + 16 high)
constexpr bool kblk_code(int type) { return type == G_Q4_0 || type == G_Q4_1 || type == G_Q5_0 || type == G_Q5_1; }
constexpr bool kblk_has_m(int type) { return type == G_Q4_1 || type == G_Q5_1; }
constexpr bool kblk_has_qh(int type) { return type == G_Q5_0 || type == G_Q5_1; }
constexpr int  kblk_qh_off(int type) { return kblk_has_m(type) ? 4 : 2; }
constexpr int  kblk_qs_off(int type) { return kblk_qh_off(type) + (kblk_has_qh(type) ? 4 : 0); }
constexpr int  kblk_block(int type) { return kblk_qs_off(type) + 16; }                     // 18 / 20 / 22 / 24
inline const char * kblk_name(int type) { return type == G_Q4_0 ? "q4_0" : type == G_Q4_1 ? "q4_1" : type == G_Q5_0 ? "q5_0" : type == G_Q5_1 ? "q5_1" : "?"; }

// ---------------------------------------------------------------------------------------------- operands

inline bool kblk_type(const qmm_tensor * t) { return t && kblk_code(t->type); }
// whole blocks, dense in a row; rows, planes and batches anywhere on 2-byte boundaries (d, m, qh and the nibbles are read at 2-byte alignment)
inline bool kblk_rows(const qmm_tensor * t) {
    return kblk_type(t) && t->ne[0] > 0 && t->ne[0] % KBLK_QK == 0 && t->nb[0] == kblk_block(t->type) && t->nb[1] % 2 == 0 && t->nb[2] % 2 == 0 &&
           t->nb[3] % 2 == 0;
}
inline bool kblk_contiguous(const qmm_tensor * t) {
    if (!kblk_type(t) || t->ne[0] % KBLK_QK || t->nb[0] != kblk_block(t->type)) return false;
    int64_t nb = t->ne[0] / KBLK_QK * kblk_block(t->type);
    for (int i = 1; i < 4; ++i) {
        if (t->ne[i] != 1 && t->nb[i] != nb) return false;
        nb *= t->ne[i];
    }
    return true;
}

// QMM_OP_CPY with a tensor of one of the four types on either side is decided here, in front of sup_cpy (and behind kq8_cpy_case)
inline bool kblk_cpy_case(const qmm_tensor * a, const qmm_tensor * d) { return kblk_type(a) || kblk_type(d); }
// f32 -> type: src rows of whole blocks with any 4-byte strides, dst contiguous; element i of src in src's index order is element i of dst
inline bool kblk_takes_quantize(const qmm_tensor * a, const qmm_tensor * d) {
    if (!a || !d || a->type != G_F32 || !kblk_contiguous(d)) return false;
    if (a->ne[0] % KBLK_QK || a->nb[0] != 4 || !strides_aligned(a, 4)) return false;
    return nelements(a) == nelements(d) && fits_u32(a);
}
// type -> f32 / f16: dst contiguous, values as dequantize_row_*, rounded once more for f16
inline bool kblk_takes_unpack(const qmm_tensor * a, const qmm_tensor * d) {
    if (!a || !d || !kblk_rows(a) || (d->type != G_F32 && d->type != G_F16) || !contiguous(d)) return false;
    return nelements(a) == nelements(d) && fits_u32(a);
}
inline bool kblk_takes_cpy(const qmm_tensor * a, const qmm_tensor * d) { return kblk_takes_quantize(a, d) || kblk_takes_unpack(a, d); }

// the attention entry points with k in one of the four types: every rule of the Q8_0 form (kq8_attn_operands_ok, its limits and its
// scratch cap) with this type's block size in nb[0]
inline bool kblk_attn_operands_ok(const AttnLimits & lim, int q_align, const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                                  const qmm_tensor * dst) {
    if (!kblk_rows(k)) return false;
    qmm_tensor k8 = *k;                              // the same rows as that predicate reads them: shape and the strides of dims 1-3
    k8.type = G_Q8_0;  k8.nb[0] = KQ8_BLOCK;
    return kq8_attn_operands_ok(lim, q_align, q, &k8, v, mask, dst);
}
inline bool kblk_takes_attn_decode(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask, const qmm_tensor * dst) {
    return kblk_attn_operands_ok(ATTN_KQ8_DECODE_LIMITS, 4, q, k, v, mask, dst);
}
inline bool kblk_takes_attn_prefill(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask, const qmm_tensor * dst) {
    return kblk_attn_operands_ok(ATTN_KQ8_PREFILL_LIMITS, 16, q, k, v, mask, dst) && kq8_unpack_bytes(k->ne[0], k->ne[1], k->ne[2]) <= KQ8_UNPACK_CAP;
}

// ---------------------------------------------------------------------------------------------- one launch

enum KblkKernel { KBLK_NONE,
                  KBLK_QUANTIZE,      // cpy_kblk_quantize_kernel<T>: one thread per block, the reference's loops as they stand
                  KBLK_UNPACK,        // cpy_kblk_unpack_kernel<T, TD>: 4 lanes per block, 8 values each
                  KBLK_DECODE };      // attn_kblk_decode_kernel<T, D>; a cut cache also runs attn_combine_kernel

struct KblkCpyPlan {
    int      kernel;              // KBLK_QUANTIZE / KBLK_UNPACK; KBLK_NONE: nothing to copy
    int      type;                // the block type: dst's (KBLK_QUANTIZE) or src's (KBLK_UNPACK)
    int      dst_type;            // KBLK_UNPACK: G_F32 or G_F16
    bool     vec;                 // KBLK_UNPACK: dst is 16-byte aligned, a thread stores its 8 values as 16-byte words
    unsigned grid, block, threads;
    char     label[40];
};

inline void kblk_unpack_label(KblkCpyPlan & p) { snprintf(p.label, sizeof(p.label), "cpy_%s_unpack_kernel<%s>", kblk_name(p.type), p.dst_type == G_F16 ? "f16" : "f32"); }

inline KblkCpyPlan kblk_cpy_plan(const qmm_tensor * a, const qmm_tensor * d) {
    KblkCpyPlan p = {};
    const uint32_t n = (uint32_t) nelements(a);
    if (n == 0) return p;
    p.block = 256;
    if (kblk_type(d)) {
        p.kernel = KBLK_QUANTIZE;  p.type = p.dst_type = d->type;  p.threads = n / KBLK_QK;
        snprintf(p.label, sizeof(p.label), "cpy_%s_quantize_kernel", kblk_name(p.type));
    } else {
        p.kernel = KBLK_UNPACK;  p.type = a->type;  p.dst_type = d->type;  p.threads = n / 8;  p.vec = data_aligned(d, 16);
        kblk_unpack_label(p);
    }
    p.grid = (p.threads + p.block - 1) / p.block;
    return p;
}

// N <= 8 tokens of H heads on a K cache of n_kv rows in `type`: kq8_decode_plan's grid, pieces, LDS and merge launch (one workgroup of 16
// waves per (head, token, piece), cut from 1024 rows on, GGML_MI355X_ATTN_SPLIT=0 keeps one piece) under this kernel's label.  Static LDS:
// the quantized q row with d and, for Q4_1 / Q5_1, s per block, and the reduction slots: within KQ8_STATIC_LDS
inline AttnPlan kblk_decode_plan(const AttnRules & r, int type, int D, int Dv, int n_kv, int N, int H) {
    AttnPlan p = kq8_decode_plan(r, D, Dv, n_kv, N, H);
    p.kernel = KBLK_DECODE;
    snprintf(p.label, sizeof(p.label), "attn_kblk_decode_kernel<%s,%d>", kblk_name(type), D);
    return p;
}

// a prompt batch: the unpack launch into the workspace ([D, n_kv, Hk] contiguous f16: rows of D halves, 16-byte aligned), then
// attn_prefill_plan's launch on that image, unchanged
struct KblkPrefillPlan {
    KblkCpyPlan unpack;
    size_t      ws_bytes;
    int64_t     k_nb1, k_nb2;     // strides of the f16 image
    AttnPlan    attn;
};
inline KblkPrefillPlan kblk_prefill_plan(int type, int D, int n_kv, int N, int H, int Hk) {
    KblkPrefillPlan p = {};
    p.ws_bytes = kq8_unpack_bytes(D, n_kv, Hk);
    p.k_nb1 = (int64_t) D * 2;  p.k_nb2 = p.k_nb1 * n_kv;
    p.unpack.kernel = KBLK_UNPACK;  p.unpack.type = type;  p.unpack.dst_type = G_F16;  p.unpack.vec = true;  p.unpack.block = 256;
    p.unpack.threads = (unsigned) ((size_t) D * n_kv * Hk / 8);
    p.unpack.grid = (p.unpack.threads + 255) / 256;
    kblk_unpack_label(p.unpack);
    p.attn = attn_prefill_plan(D, n_kv, N, H);
    return p;
}

} // namespace qmm
