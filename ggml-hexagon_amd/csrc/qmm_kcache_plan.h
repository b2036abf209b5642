// qmm_kcache_plan.h — the launch plan of everything a Q8_0 K cache adds (qmm_kcache.hiph): which operands the entry points take with a
// Q8_0 tensor among them (CPY f32 -> Q8_0, CPY Q8_0 -> f32 / f16, qmm_attn_decode / qmm_attn_prefill with k in Q8_0), and for operands
// they take which kernel runs with which grid, block and LDS bytes, under which trace label, how a long cache is cut into pieces, and
// how much scratch the prompt form may use.  Plain C++ (no HIP, no ggml; a host compiler alone reads it, like qmm_attn_plan.h and
// qmm_glue_plan.h, whose helpers it uses and whose tables it leaves alone).  The kernels take their constants from here; the host side
// in qmm_kcache.hiph executes a plan and decides nothing.
// V stays the transposed F16 cache; a quantized V, other K types and D = 256 are outside this surface (the plugin runs the unfused nodes).
#pragma once

#include "qmm_attn_plan.h"
#include "qmm_glue_plan.h"

namespace qmm {

enum : int { G_Q8_0 = 8 };
constexpr int KQ8_QK = 32, KQ8_BLOCK = 34;       // block_q8_0 (ggml-common.h): one f16 d, then 32 int8; the int8 run sits 2 bytes into the block

// ---------------------------------------------------------------------------------------------- operands

inline bool kq8_type(const qmm_tensor * t) { return t && t->type == G_Q8_0; }
// whole blocks, dense in a row; rows, planes and batches anywhere on 2-byte boundaries (the f16 d is read as one value)
inline bool kq8_rows(const qmm_tensor * t) {
    return kq8_type(t) && t->ne[0] > 0 && t->ne[0] % KQ8_QK == 0 && t->nb[0] == KQ8_BLOCK && t->nb[1] % 2 == 0 && t->nb[2] % 2 == 0 && t->nb[3] % 2 == 0;
}
inline bool kq8_contiguous(const qmm_tensor * t) {
    if (!kq8_type(t) || t->ne[0] % KQ8_QK || t->nb[0] != KQ8_BLOCK) return false;
    int64_t nb = t->ne[0] / KQ8_QK * KQ8_BLOCK;
    for (int i = 1; i < 4; ++i) {
        if (t->ne[i] != 1 && t->nb[i] != nb) return false;
        nb *= t->ne[i];
    }
    return true;
}

// QMM_OP_CPY with a Q8_0 tensor on either side is decided here, in front of sup_cpy (which refuses every quantized type)
inline bool kq8_cpy_case(const qmm_tensor * a, const qmm_tensor * d) { return kq8_type(a) || kq8_type(d); }
// f32 -> Q8_0: src rows of whole blocks with any 4-byte strides, dst contiguous; element i of src in src's index order is element i of dst
inline bool kq8_takes_quantize(const qmm_tensor * a, const qmm_tensor * d) {
    if (!a || !d || a->type != G_F32 || !kq8_contiguous(d)) return false;
    if (a->ne[0] % KQ8_QK || a->nb[0] != 4 || !strides_aligned(a, 4)) return false;
    return nelements(a) == nelements(d) && fits_u32(a);
}
// Q8_0 -> f32 / f16: dst contiguous, value = f32(d) * q, rounded once for f16
inline bool kq8_takes_unpack(const qmm_tensor * a, const qmm_tensor * d) {
    if (!a || !d || !kq8_rows(a) || (d->type != G_F32 && d->type != G_F16) || !contiguous(d)) return false;
    return nelements(a) == nelements(d) && fits_u32(a);
}
inline bool kq8_takes_cpy(const qmm_tensor * a, const qmm_tensor * d) { return kq8_takes_quantize(a, d) || kq8_takes_unpack(a, d); }

// the attention entry points with k in Q8_0: few tokens D in {64, 128}, Dv <= 128, n_kv in whole llama.cpp paddings (32) up to 16384, N <= 8;
// a prompt batch D = Dv in {64, 128}, n_kv a multiple of 32
constexpr AttnLimits ATTN_KQ8_DECODE_LIMITS  = { 32, 128, 128, 16384, 8 };
constexpr AttnLimits ATTN_KQ8_PREFILL_LIMITS = { 32, 128, 0, 1 << 20, 1 << 20 };
// the prompt form unpacks the n_kv x H_kv K rows the batch reads into the context's workspace as f16 and runs attn_prefill_kernel on that
// image: at most this many bytes of it (llama3-8b's 8 kv heads of 128 at 32768 cache rows); past it the predicate answers 0
constexpr size_t KQ8_UNPACK_CAP = (size_t) 64 << 20;
inline size_t kq8_unpack_bytes(int64_t D, int64_t n_kv, int64_t Hk) { return (size_t) D * (size_t) n_kv * (size_t) Hk * 2; }

// attn_operands_ok of qmm_attn.hiph with the K rows in Q8_0: q f32 [D, N, H], k Q8_0 [D, n_kv, Hk], v f16 [n_kv, Dv, Hk] (the transposed
// cache, flags 0), mask f32 [n_kv, >= N], dst f32 [Dv * H, N]
inline bool kq8_attn_operands_ok(const AttnLimits & lim, int q_align, const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                                 const qmm_tensor * dst) {
    if (!q || !k || !v || !mask || !dst || v->flags != 0) return false;
    if (q->type != G_F32 || !kq8_rows(k) || v->type != G_F16 || mask->type != G_F32 || dst->type != G_F32) return false;
    const int64_t D = k->ne[0], n_kv = k->ne[1], Hk = k->ne[2], N = q->ne[1], H = q->ne[2], Dv = v->ne[1];
    if (!attn_shape_ok(lim, D, Dv, n_kv, N, H, Hk)) return false;
    if (q->ne[0] != D || v->ne[0] != n_kv || v->ne[2] != Hk || q->ne[3] != 1 || k->ne[3] != 1 || v->ne[3] != 1) return false;
    if (q->nb[0] != 4 || v->nb[0] != 2 || mask->nb[0] != 4 || dst->nb[0] != 4) return false;
    if (mask->ne[0] != n_kv || mask->ne[1] < N || dst->ne[0] != Dv * H || dst->ne[1] != N || dst->ne[2] != 1 || dst->ne[3] != 1) return false;
    return !(q->nb[1] % q_align || q->nb[2] % q_align || v->nb[1] % 16 || v->nb[2] % 16 || mask->nb[1] % 4 || dst->nb[1] % 4);
}
inline bool kq8_takes_attn_decode(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask, const qmm_tensor * dst) {
    return kq8_attn_operands_ok(ATTN_KQ8_DECODE_LIMITS, 4, q, k, v, mask, dst);
}
inline bool kq8_takes_attn_prefill(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask, const qmm_tensor * dst) {
    return kq8_attn_operands_ok(ATTN_KQ8_PREFILL_LIMITS, 16, q, k, v, mask, dst) && kq8_unpack_bytes(k->ne[0], k->ne[1], k->ne[2]) <= KQ8_UNPACK_CAP;
}

// ---------------------------------------------------------------------------------------------- one launch

enum Kq8Kernel { KQ8_NONE,
                 KQ8_QUANTIZE,       // cpy_q8_0_quantize_kernel: 8 lanes per block, 4 values each
                 KQ8_UNPACK,         // cpy_q8_0_unpack_kernel<TD>: 4 lanes per block, 8 values each
                 KQ8_DECODE };       // attn_kq8_decode_kernel<D>; a cut cache also runs attn_combine_kernel

struct Kq8CpyPlan {
    int      kernel;              // KQ8_QUANTIZE / KQ8_UNPACK; KQ8_NONE: nothing to copy
    int      dst_type;            // KQ8_UNPACK: G_F32 or G_F16
    bool     vec;                 // KQ8_UNPACK: dst is 16-byte aligned, a thread stores its 8 values as 16-byte words
    unsigned grid, block, threads;
    char     label[40];
};

inline Kq8CpyPlan kq8_cpy_plan(const qmm_tensor * a, const qmm_tensor * d) {
    Kq8CpyPlan p = {};
    const uint32_t n = (uint32_t) nelements(a);
    if (n == 0) return p;
    p.block = 256;
    if (kq8_type(d)) {
        p.kernel = KQ8_QUANTIZE;  p.dst_type = G_Q8_0;  p.threads = n / 4;
        snprintf(p.label, sizeof(p.label), "cpy_q8_0_quantize_kernel");
    } else {
        p.kernel = KQ8_UNPACK;  p.dst_type = d->type;  p.threads = n / 8;  p.vec = data_aligned(d, 16);
        snprintf(p.label, sizeof(p.label), "cpy_q8_0_unpack_kernel<%s>", d->type == G_F16 ? "f16" : "f32");
    }
    p.grid = (p.threads + p.block - 1) / p.block;
    return p;
}

// N <= 8 tokens of H heads on a Q8_0 K cache of n_kv rows: one workgroup of 16 waves per (head, token) and, from 1024 cache rows on (the
// cut of attn_decode_plan), per piece of the cache, merged by attn_combine_kernel.  Dynamic LDS: the piece's scores; the quantized q
// row and the reduction slots are static (at most KQ8_STATIC_LDS bytes: they count against the 64 KiB a kernel may use unasked).
// GGML_MI355X_ATTN_SPLIT=0 keeps one piece
constexpr size_t KQ8_STATIC_LDS = 256;
inline AttnPlan kq8_decode_plan(const AttnRules & r, int D, int Dv, int n_kv, int N, int H) {
    AttnPlan p = {};
    p.kernel = KQ8_DECODE;  p.D = D;  p.N = N;
    p.grid[0] = (unsigned) H;  p.grid[1] = (unsigned) N;  p.grid[2] = 1;  p.block = 1024;
    p.chunk = n_kv;
    if (r.split_on && n_kv >= 1024) {
        p.S = n_kv / 256 < 16 ? n_kv / 256 : 16;
        p.chunk = ((n_kv + p.S - 1) / p.S + 7) / 8 * 8;
        p.ws_bytes = (size_t) H * N * p.S * (Dv + 2) * sizeof(float);
        p.grid[2] = (unsigned) p.S;
        p.grid2[0] = (unsigned) H;  p.grid2[1] = (unsigned) N;  p.block2 = 256;
        snprintf(p.label2, sizeof(p.label2), "attn_combine_kernel");
    }
    p.lds = (size_t) p.chunk * 4;
    p.lds_attr = p.lds + KQ8_STATIC_LDS > 64 * 1024;
    snprintf(p.label, sizeof(p.label), "attn_kq8_decode_kernel<%d>", D);
    return p;
}

// a prompt batch: the unpack launch into the workspace ([D, n_kv, Hk] contiguous f16: rows of D halves, 16-byte aligned), then
// attn_prefill_plan's launch on that image, unchanged
struct Kq8PrefillPlan {
    Kq8CpyPlan unpack;
    size_t     ws_bytes;
    int64_t    k_nb1, k_nb2;      // strides of the f16 image
    AttnPlan   attn;
};
inline Kq8PrefillPlan kq8_prefill_plan(int D, int n_kv, int N, int H, int Hk) {
    Kq8PrefillPlan p = {};
    p.ws_bytes = kq8_unpack_bytes(D, n_kv, Hk);
    p.k_nb1 = (int64_t) D * 2;  p.k_nb2 = p.k_nb1 * n_kv;
    p.unpack.kernel = KQ8_UNPACK;  p.unpack.dst_type = G_F16;  p.unpack.vec = true;  p.unpack.block = 256;
    p.unpack.threads = (unsigned) ((size_t) D * n_kv * Hk / 8);
    p.unpack.grid = (p.unpack.threads + 255) / 256;
    snprintf(p.unpack.label, sizeof(p.unpack.label), "cpy_q8_0_unpack_kernel<f16>");
    p.attn = attn_prefill_plan(D, n_kv, N, H);
    return p;
}

} // namespace qmm
