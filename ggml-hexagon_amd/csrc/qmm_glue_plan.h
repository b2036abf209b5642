// qmm_glue_plan.h — the one launch plan of the glue ops (qmm_ops.hip): which operands each entry point takes (the sup_* predicates), and
// for operands it takes which kernel runs with which template arguments, grid, block and LDS bytes, under which trace label, or why
// not.  Plain C++ (no HIP, no ggml; a host compiler alone reads it, like qmm_prefill_plan.h, qmm_matvec_plan.h and qmm_attn_plan.h).
// A plan reads types, extents, strides, the op_params that steer a branch (soft-max max_bias; the rope mode in sup_rope) and the low
// bits of the data pointers; it never follows one.  The kernels take their launch constants from here; run_glue executes a plan and
// decides nothing.  Building a plan compares a few integers: no formatting, no allocation (a token is a few hundred of these).
#pragma once

#include "../../include/ggml_mi355x_ops.h"
#include "qmm_types.h"

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <initializer_list>

namespace qmm {

enum : int { G_F32 = 0, G_F16 = 1, G_I32 = 26 };

constexpr int      DOT_T = 128;      // threads per dst element of mul_mat_dot_block_kernel / per expert of moe_router_logits_kernel
constexpr int      MM_T = 64;        // mul_mat_f16_kernel: src0 rows x src1 rows of a workgroup
constexpr uint32_t ROPE_HC = 8;      // rope_store_kernel: heads of one (pair, token) a thread ropes

// ---------------------------------------------------------------------------------------------- operands

inline int64_t nelements(const qmm_tensor * t) { return t->ne[0] * t->ne[1] * t->ne[2] * t->ne[3]; }
inline int64_t nrows(const qmm_tensor * t) { return t->ne[1] * t->ne[2] * t->ne[3]; }
inline int     esize(int type) { return type == G_F32 || type == G_I32 ? 4 : type == G_F16 ? 2 : 0; }
inline bool    same_shape(const qmm_tensor * a, const qmm_tensor * b) {
    return a->ne[0] == b->ne[0] && a->ne[1] == b->ne[1] && a->ne[2] == b->ne[2] && a->ne[3] == b->ne[3];
}
inline bool contiguous(const qmm_tensor * t) {
    const int es = esize(t->type);
    if (!es) return false;
    int64_t nb = es;
    for (int i = 0; i < 4; ++i) {
        if (t->ne[i] != 1 && t->nb[i] != nb) return false;
        nb *= t->ne[i];
    }
    return true;
}
// rows are dense runs of elements (nb[0] == element size); rows themselves may sit anywhere
inline bool dense_rows(const qmm_tensor * t) { return esize(t->type) && (t->nb[0] == esize(t->type) || t->ne[0] == 1); }
inline bool fits_u32(const qmm_tensor * t) { return nelements(t) < ((int64_t) 1 << 31); }
inline bool strides_aligned(const qmm_tensor * t, int a) { return t->nb[1] % a == 0 && t->nb[2] % a == 0 && t->nb[3] % a == 0; }
inline bool data_aligned(const qmm_tensor * t, int a) { return (uintptr_t) t->data % a == 0; }
inline bool aligned_to(const qmm_tensor * t, int a) { return data_aligned(t, a) && strides_aligned(t, a); }
inline bool one_f32_row(const qmm_tensor * w, int64_t ne0) {          // a norm weight: one contiguous f32 row, broadcast over all rows
    return w->type == G_F32 && contiguous(w) && w->ne[0] == ne0 && nelements(w) == w->ne[0];
}
inline float f32_param(const qmm_tensor * d, int i) {
    float v;
    memcpy(&v, &d->op_params[i], sizeof(float));
    return v;
}

// ---------------------------------------------------------------------------------------------- rules more than one kernel follows

// rms_norm_vec_kernel, moe_combine_add_norm_kernel and moe_router_logits_kernel<true> keep a row in registers as float4: four per thread
// of at most 1024 threads ...
inline bool row_norm_in_regs(int64_t ne0) { return ne0 % 4 == 0 && ne0 <= 1024 * 16; }
// ... few rows (token generation) with 1024 threads per row, many rows (prefill) with 256 where the row fits them.  The fused kernels
// take the stand-alone kernel's partition, so that their results are its results bit for bit
inline int row_norm_threads(int64_t rows, int64_t ne0) { return rows < 256 || ne0 > 256 * 16 ? 1024 : 256; }

// a 2-D transpose through 32 x 32 tiles in LDS (cpy_transpose_kernel; the V part of rope_store_kernel<true>): same extents, src dense
// along dim 1, dst dense along dim 0, and large enough for the tiles
inline bool transpose_2d(const qmm_tensor * a, const qmm_tensor * d, int64_t min_ne1) {
    return a->ne[2] == 1 && a->ne[3] == 1 && d->ne[2] == 1 && d->ne[3] == 1 && a->ne[0] == d->ne[0] && a->ne[1] == d->ne[1] &&
           a->nb[1] == esize(a->type) && d->nb[0] == esize(d->type) && a->ne[0] >= 32 && a->ne[1] >= min_ne1;
}

// threads rope_pair_heads wants for a tensor: one per (pair, ROPE_HC heads, token)
inline uint32_t rope_heads_threads(const qmm_tensor * t) {
    return (uint32_t) (t->ne[0] / 2 * ((t->ne[1] + ROPE_HC - 1) / ROPE_HC) * t->ne[2] * t->ne[3]);
}

// ---------------------------------------------------------------------------------------------- what the entry points take

inline bool is_binary(int op) { return op >= QMM_OP_ADD && op <= QMM_OP_DIV; }
inline bool is_unary(int op) { return op >= QMM_OP_SCALE && op <= QMM_OP_EXP; }

inline bool sup_binary(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * d) {
    if (!a || !b || !d || a->type != G_F32 || b->type != G_F32 || d->type != G_F32) return false;
    if (!same_shape(a, d) || !dense_rows(a) || !dense_rows(d) || !fits_u32(d) || nelements(d) == 0) return false;
    for (int i = 0; i < 4; ++i) if (b->ne[i] <= 0 || d->ne[i] % b->ne[i]) return false;       // ggml_can_repeat(b, a)
    return strides_aligned(a, 4) && b->nb[0] % 4 == 0 && strides_aligned(b, 4);
}
inline bool sup_unary(const qmm_tensor * a, const qmm_tensor * d) {
    return a && d && a->type == G_F32 && d->type == G_F32 && same_shape(a, d) && contiguous(a) && contiguous(d) && fits_u32(d);
}
inline bool sup_rms_norm(const qmm_tensor * a, const qmm_tensor * d) {
    return a && d && a->type == G_F32 && d->type == G_F32 && same_shape(a, d) && dense_rows(a) && dense_rows(d) && fits_u32(d) &&
           nelements(d) > 0;
}
inline bool sup_rope(const qmm_tensor * a, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * d) {
    if (!a || !pos || !d || a->type != G_F32 || d->type != G_F32 || pos->type != G_I32 || !same_shape(a, d)) return false;
    if (!dense_rows(a) || !dense_rows(d) || !contiguous(pos) || !fits_u32(d) || nelements(d) == 0 || a->ne[0] % 2) return false;
    const int n_dims = d->op_params[1], mode = d->op_params[2];
    if (mode != 0 && mode != 2) return false;                                     // normal or NEOX; no M-RoPE / vision
    if (n_dims <= 0 || n_dims % 2 || n_dims > a->ne[0] || pos->ne[0] != a->ne[2]) return false;
    if (ff && (ff->type != G_F32 || ff->ne[0] < n_dims / 2 || !contiguous(ff))) return false;
    return true;
}
inline bool sup_soft_max(const qmm_tensor * a, const qmm_tensor * mask, const qmm_tensor * d) {
    if (!a || !d || a->type != G_F32 || d->type != G_F32 || !same_shape(a, d) || !contiguous(a) || !contiguous(d)) return false;
    if (nelements(d) == 0 || nrows(d) >= ((int64_t) 1 << 31)) return false;
    if (mask) {
        if (mask->type != G_F32 && mask->type != G_F16) return false;
        if (!contiguous(mask) || mask->ne[0] != a->ne[0] || mask->ne[1] < a->ne[1] || mask->ne[2] != 1 || mask->ne[3] != 1) return false;
    }
    return true;
}
inline bool sup_cpy(const qmm_tensor * a, const qmm_tensor * d) {
    if (!a || !d || !esize(a->type) || !esize(d->type) || a->type == G_I32 || d->type == G_I32) return false;
    return nelements(a) == nelements(d) && fits_u32(a) && a->nb[0] % esize(a->type) == 0 && d->nb[0] % esize(d->type) == 0;
}
inline bool sup_get_rows(const qmm_tensor * a, const qmm_tensor * ids, const qmm_tensor * d) {
    if (!a || !ids || !d || ids->type != G_I32 || d->type != G_F32 || !dense_rows(d) || nelements(d) == 0) return false;
    if (d->ne[0] != a->ne[0] || d->ne[1] != ids->ne[0] || d->ne[2] != ids->ne[1] || d->ne[3] != ids->ne[2] || ids->ne[3] != 1) return false;
    if (a->ne[2] != ids->ne[1] || a->ne[3] != ids->ne[2] || nrows(d) >= ((int64_t) 1 << 31)) return false;
    if (type_known(a->type)) return a->ne[0] % type_blck(a->type) == 0 && a->nb[1] % 2 == 0 && !iq1m_misaligned(a->type, a->data, a->nb[1], a->nb[2] | a->nb[3]);
    return (a->type == G_F32 || a->type == G_F16) && dense_rows(a);
}
inline bool sup_mul_mat_f(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * d) {
    if (!a || !b || !d || (a->type != G_F16 && a->type != G_F32) || b->type != G_F32 || d->type != G_F32) return false;
    if (a->ne[0] != b->ne[0] || d->ne[0] != a->ne[1] || d->ne[1] != b->ne[1] || d->ne[2] != b->ne[2] || d->ne[3] != b->ne[3]) return false;
    if (a->ne[2] <= 0 || a->ne[3] <= 0 || b->ne[2] % a->ne[2] || b->ne[3] % a->ne[3] || nelements(d) == 0 || a->ne[0] == 0) return false;
    if (a->nb[0] != esize(a->type) || b->nb[0] != 4 || d->nb[0] != 4) return false;         // K dense in both operands
    if (b->ne[2] * b->ne[3] > 65535 || a->ne[1] >= ((int64_t) 1 << 30) || b->ne[1] >= ((int64_t) 1 << 22)) return false;
    return strides_aligned(a, esize(a->type)) && strides_aligned(b, 4) && strides_aligned(d, 4);
}
inline bool sup_argsort(const qmm_tensor * a, const qmm_tensor * d) {
    return a && d && a->type == G_F32 && d->type == G_I32 && same_shape(a, d) && dense_rows(a) && dense_rows(d) && nelements(a) > 0 &&
           a->ne[0] <= 4096 && nrows(a) < ((int64_t) 1 << 31) && (d->op_params[0] == 0 || d->op_params[0] == 1);
}
inline bool sup_sum_rows(const qmm_tensor * a, const qmm_tensor * d) {
    return a && d && a->type == G_F32 && d->type == G_F32 && dense_rows(a) && d->ne[0] == 1 && d->ne[1] == a->ne[1] && d->ne[2] == a->ne[2] &&
           d->ne[3] == a->ne[3] && nelements(a) > 0 && nrows(a) < ((int64_t) 1 << 31);
}

// qmm_op_supported
inline bool sup_op(int op, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * c, const qmm_tensor * d) {
    if (is_binary(op)) return sup_binary(a, b, d);
    if (is_unary(op)) return sup_unary(a, d);
    switch (op) {
        case QMM_OP_RMS_NORM:     return sup_rms_norm(a, d);
        case QMM_OP_NORM:         return sup_rms_norm(a, d);
        case QMM_OP_RMS_NORM_MUL: return sup_rms_norm(a, d) && b && one_f32_row(b, a->ne[0]);
        case QMM_OP_SILU_MUL:     return sup_unary(a, d) && b && sup_unary(b, d);
        case QMM_OP_ROPE:         return sup_rope(a, b, c, d);
        case QMM_OP_SOFT_MAX:     return sup_soft_max(a, b, d);
        case QMM_OP_CPY:          return sup_cpy(a, d);
        case QMM_OP_GET_ROWS:     return sup_get_rows(a, b, d);
        case QMM_OP_MUL_MAT_F:    return sup_mul_mat_f(a, b, d);
        case QMM_OP_ARGSORT:      return sup_argsort(a, d);
        case QMM_OP_SUM_ROWS:     return sup_sum_rows(a, d);
        default:                  return false;
    }
}

// qmm_op_add_rms_norm_supported: everything rms_norm_vec_kernel<.., true, ..> needs but the alignment of the pointers themselves
inline bool sup_add_rms_norm(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * sum, const qmm_tensor * dst) {
    if (!a || !b || !sum || !dst || !sup_rms_norm(sum, dst) || !sup_binary(a, b, sum) || !same_shape(a, b) || !dense_rows(b)) return false;
    if (!row_norm_in_regs(a->ne[0]) || !strides_aligned(a, 16) || !strides_aligned(b, 16) || !strides_aligned(sum, 16) || !strides_aligned(dst, 16)) return false;
    return !w || one_f32_row(w, a->ne[0]);
}

// qmm_rope_kv_store_supported
inline bool sup_rope_kv_store(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst, const qmm_tensor * k,
                              const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst) {
    if (!sup_rope(q, pos, ff, q_dst)) return false;
    if (k) {
        if (!k_dst || k->type != G_F32 || k_dst->type != G_F16 || !same_shape(k, k_dst) || !dense_rows(k) || !dense_rows(k_dst) || !fits_u32(k)) return false;
        if (k->ne[0] != q->ne[0] || k->ne[2] != q->ne[2] || k->ne[3] != q->ne[3] || nelements(k) == 0) return false;
        if (!strides_aligned(k, 4) || !strides_aligned(k_dst, 2)) return false;
    }
    if (v) {
        if (!v_dst || v->type != G_F32 || v_dst->type != G_F16 || nelements(v) != nelements(v_dst) || !fits_u32(v) || nelements(v) == 0) return false;
        if (v->nb[0] % 4 || !strides_aligned(v, 4) || v_dst->nb[0] % 2 || !strides_aligned(v_dst, 2)) return false;
    }
    return nelements(q) / 2 + (k ? nelements(k) / 2 : 0) + (v ? nelements(v) : 0) < ((int64_t) 1 << 31);
}

// qmm_moe_router_supported
inline bool sup_moe_router(const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used) {
    if (!logits || !ids || !weights || logits->type != G_F32 || ids->type != G_I32 || weights->type != G_F32) return false;
    const int64_t E = logits->ne[0], N = logits->ne[1];
    if (E < 1 || E > 64 || n_used < 1 || n_used > E || N < 1 || N >= ((int64_t) 1 << 30)) return false;
    if (logits->ne[2] != 1 || logits->ne[3] != 1 || ids->ne[0] != E || ids->ne[1] != N || ids->ne[2] != 1 || ids->ne[3] != 1) return false;
    if (nelements(weights) != n_used * N) return false;
    return logits->nb[0] == 4 && ids->nb[0] == 4 && weights->nb[0] == 4 && logits->nb[1] % 4 == 0 && ids->nb[1] % 4 == 0;
}
// qmm_moe_router_logits_supported
inline bool sup_moe_router_logits(const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * logits, const qmm_tensor * ids,
                                  const qmm_tensor * weights, int64_t n_used) {
    if (!gate_inp || !x || !sup_moe_router(logits, ids, weights, n_used)) return false;
    if (gate_inp->type != G_F32 || x->type != G_F32) return false;
    const int64_t K = gate_inp->ne[0], E = gate_inp->ne[1], N = x->ne[1];
    // (more tokens: the tiled MUL_MAT + moe_router_kernel; K < 1024: qmm_op(MUL_MAT) takes a wave per element there, another order of additions)
    if (K < 1024 || K >= ((int64_t) 1 << 30) || E != logits->ne[0] || N != logits->ne[1] || N > 8 || x->ne[0] != K) return false;
    if (gate_inp->ne[2] != 1 || gate_inp->ne[3] != 1 || x->ne[2] != 1 || x->ne[3] != 1) return false;
    return gate_inp->nb[0] == 4 && x->nb[0] == 4 && gate_inp->nb[1] % 4 == 0 && x->nb[1] % 4 == 0;
}
// qmm_moe_router_logits_norm_supported
inline bool sup_moe_router_logits_norm(const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * norm_w, const qmm_tensor * normed,
                                       const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used) {
    if (!norm_w || !normed || !sup_moe_router_logits(gate_inp, x, logits, ids, weights, n_used)) return false;
    const int64_t K = x->ne[0];
    if (norm_w->type != G_F32 || normed->type != G_F32 || !row_norm_in_regs(K)) return false;
    if (norm_w->ne[0] != K || norm_w->ne[1] * norm_w->ne[2] * norm_w->ne[3] != 1 || norm_w->nb[0] != 4) return false;
    if (!same_shape(normed, x)) return false;
    if (normed->nb[0] != 4 || x->nb[1] % 16 || normed->nb[1] % 16 || gate_inp->nb[1] % 16) return false;
    return data_aligned(x, 16) && data_aligned(normed, 16) && data_aligned(norm_w, 16) && data_aligned(gate_inp, 16);
}

// qmm_moe_combine_supported
inline bool sup_moe_combine(const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * out) {
    if (!x || !w || !out || x->type != G_F32 || w->type != G_F32 || out->type != G_F32) return false;
    const int64_t E = x->ne[0], U = x->ne[1], N = x->ne[2];
    if (E < 4 || E % 4 || U < 1 || U > 64 || N < 1 || N > 65535 || x->ne[3] != 1) return false;
    if (w->ne[0] != 1 || w->ne[1] != U || w->ne[2] != N || w->ne[3] != 1 || out->ne[0] != E || out->ne[1] != N || out->ne[2] != 1 || out->ne[3] != 1) return false;
    if (x->nb[0] != 4 || out->nb[0] != 4 || x->nb[1] % 16 || x->nb[2] % 16 || out->nb[1] % 16 || w->nb[1] % 4 || w->nb[2] % 4) return false;
    return true;
}
// qmm_moe_combine_add_rms_norm_supported
inline bool sup_moe_combine_add_rms_norm(const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * b, const qmm_tensor * nw, const qmm_tensor * sum,
                                         const qmm_tensor * dst) {
    if (!b || !nw || !sum || !dst || !sup_moe_combine(x, w, sum)) return false;
    const int64_t E = x->ne[0], N = x->ne[2];
    if (!row_norm_in_regs(E) || b->type != G_F32 || nw->type != G_F32 || dst->type != G_F32) return false;
    for (const qmm_tensor * t : { b, sum, dst })
        if (t->ne[0] != E || t->ne[1] != N || t->ne[2] != 1 || t->ne[3] != 1 || t->nb[0] != 4 || t->nb[1] % 16 || !data_aligned(t, 16)) return false;
    return nw->ne[0] == E && nw->ne[1] * nw->ne[2] * nw->ne[3] == 1 && nw->nb[0] == 4 && data_aligned(nw, 16) && data_aligned(x, 16);
}

// ---------------------------------------------------------------------------------------------- one launch

// the kernel families, with the template arguments GluePlan::targ holds for each, in the kernel's order
enum GlueKernel { GK_NONE,
                  GK_BINARY,                // binary_kernel<OP, VEC>
                  GK_UNARY,                 // unary_kernel<OP, MUL2>
                  GK_RMS_NORM,              // rms_norm_kernel<MUL>
                  GK_RMS_NORM_VEC,          // rms_norm_vec_kernel<MUL, ADD, NT>
                  GK_NORM,                  // norm_kernel
                  GK_SOFT_MAX_WAVE,         // soft_max_wave_kernel<V4>
                  GK_SOFT_MAX,              // soft_max_kernel<MASK_F16>
                  GK_ROPE,                  // rope_kernel
                  GK_MEMCPY,                // hipMemcpyAsync, no kernel
                  GK_CPY, GK_CPY_TRANSPOSE, // cpy_kernel<TS, TD>, cpy_transpose_kernel<TS, TD>, types by their ids (G_F32, G_F16)
                  GK_GET_ROWS,              // get_rows_kernel<TS>
                  GK_GET_ROWS_Q,            // get_rows_q_kernel<T>
                  GK_MUL_MAT_F16,           // mul_mat_f16_kernel<VEC>
                  GK_MUL_MAT_DOT_BLOCK,     // mul_mat_dot_block_kernel
                  GK_MUL_MAT_DOT,           // mul_mat_dot_kernel<TA>
                  GK_ARGSORT, GK_SUM_ROWS,  // argsort_kernel, sum_rows_kernel
                  GK_ROPE_STORE,            // rope_store_kernel<VT>
                  GK_MOE_ROUTER,            // moe_router_kernel
                  GK_MOE_ROUTER_LOGITS,     // moe_router_logits_kernel<NORM>
                  GK_MOE_COMBINE,           // moe_combine_kernel
                  GK_MOE_COMBINE_ADD_NORM,  // moe_combine_add_norm_kernel<NT>
                  GK_COUNT };

// every label a glue launch can leave in a trace (qmm_trace_begin), one per launch: the kernel and the branch taken.  The rope store,
// the router forms and the combine forms leave none
enum GlueLabel { GL_NONE, GL_BINARY_VEC, GL_BINARY_SCALAR, GL_UNARY, GL_RMS_NORM_VEC_1024, GL_RMS_NORM_VEC_256, GL_RMS_NORM, GL_NORM,
                 GL_SOFT_MAX_WAVE_1, GL_SOFT_MAX_WAVE_2, GL_SOFT_MAX_WAVE_4, GL_SOFT_MAX_LDS, GL_SOFT_MAX_DST, GL_ROPE, GL_MEMCPY, GL_CPY,
                 GL_CPY_TRANSPOSE, GL_GET_ROWS, GL_GET_ROWS_Q, GL_MUL_MAT_F16_VEC, GL_MUL_MAT_F16_SCALAR, GL_MUL_MAT_DOT_BLOCK, GL_MUL_MAT_DOT,
                 GL_ARGSORT, GL_SUM_ROWS, GL_COUNT };
// (soft_max_wave: float4 per lane; soft_max: where the row is staged; memcpy: also when src == dst and nothing is copied; get_rows_q: the
// one format, its type id is GluePlan::targ[0], formatted by QMM_TRACE and so only while tracing)
constexpr const char * GLUE_LABELS[GL_COUNT] = {
    nullptr, "binary_kernel<vec>", "binary_kernel<scalar>", "unary_kernel", "rms_norm_vec_kernel<1024>", "rms_norm_vec_kernel<256>", "rms_norm_kernel",
    "norm_kernel", "soft_max_wave_kernel<1>", "soft_max_wave_kernel<2>", "soft_max_wave_kernel<4>", "soft_max_kernel<lds>", "soft_max_kernel<dst>",
    "rope_kernel", "memcpy", "cpy_kernel", "cpy_transpose_kernel", "get_rows_kernel", "get_rows_q_kernel<%d>", "mul_mat_f16_kernel<vec>",
    "mul_mat_f16_kernel<scalar>", "mul_mat_dot_block_kernel", "mul_mat_dot_kernel", "argsort_kernel", "sum_rows_kernel",
};

struct GluePlan {
    int          kernel;          // GlueKernel
    int          targ[3];         // its template arguments in the kernel's order: bools 0 / 1, element types by their ids
    unsigned     grid[3], block;
    size_t       lds;             // dynamic LDS bytes
    unsigned     karg[2];         // rope_store_kernel<true>: the two kernel arguments its grid is the sum of (rope blocks, tiles along ne0)
    bool         launch;          // false: nothing is launched or copied
    const char * label;           // of GLUE_LABELS, or NULL: no trace entry
    int          err;             // a refusal only the pointers' low bits decide: QMM_OK or the code, ...
    const char * msg;             // ... and the whole text
};

inline GluePlan glue_plan(int kernel, GlueLabel label, unsigned gx, unsigned block, int t0 = 0, int t1 = 0, int t2 = 0) {
    GluePlan p = {};
    p.kernel = kernel;  p.targ[0] = t0;  p.targ[1] = t1;  p.targ[2] = t2;
    p.grid[0] = gx;  p.grid[1] = 1;  p.grid[2] = 1;  p.block = block;
    p.launch = true;
    p.label = GLUE_LABELS[label];
    return p;
}
inline GluePlan glue_nothing(GlueLabel label = GL_NONE) {
    GluePlan p = {};
    p.label = GLUE_LABELS[label];
    return p;
}
inline GluePlan glue_refusal(int err, const char * msg) {
    GluePlan p = {};
    p.err = err;  p.msg = msg;
    return p;
}

// one block per group of rows; vector path when every row is 16-byte aligned and src1 has full rows
inline GluePlan glue_binary_plan(int op, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * d) {
    const uint32_t rows = (uint32_t) nrows(d);
    const bool vec = d->ne[0] % 4 == 0 && b->ne[0] == d->ne[0] && b->nb[0] == 4 && aligned_to(a, 16) && aligned_to(b, 16) && aligned_to(d, 16);
    const uint32_t per_row = (uint32_t) (vec ? d->ne[0] / 4 : d->ne[0]);
    const uint32_t rpb = per_row >= 256 ? 1 : 256 / per_row;          // rows per block for short rows, as binary_kernel takes them
    return glue_plan(GK_BINARY, vec ? GL_BINARY_VEC : GL_BINARY_SCALAR, (rows + rpb - 1) / rpb, 256, op, vec);
}

// contiguous f32, a float4 per thread; b: the second factor of SILU_MUL
inline GluePlan glue_unary_plan(int op, const qmm_tensor * b, const qmm_tensor * d) {
    const uint32_t n = (uint32_t) nelements(d);
    if (n == 0) return glue_nothing();
    return glue_plan(GK_UNARY, GL_UNARY, (n + 1023) / 1024, 256, op, b != nullptr);
}

// y = rms_norm(a [+ b]) [* w]; `sum` receives a + b when b is given.  One block per row
inline GluePlan glue_rms_norm_plan(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * d, const qmm_tensor * sum) {
    const unsigned rows = (unsigned) nrows(d);
    const bool vec = row_norm_in_regs(a->ne[0]) && aligned_to(a, 16) && aligned_to(d, 16) && (!w || data_aligned(w, 16)) &&
                     (!b || (aligned_to(b, 16) && aligned_to(sum, 16)));
    if (vec) {
        const int nt = row_norm_threads(rows, a->ne[0]);
        return glue_plan(GK_RMS_NORM_VEC, nt == 1024 ? GL_RMS_NORM_VEC_1024 : GL_RMS_NORM_VEC_256, rows, (unsigned) nt, w != nullptr, b != nullptr, nt);
    }
    if (b) return glue_refusal(QMM_EUNSUPPORTED, "ADD + RMS_NORM: rows must be 16-byte aligned, ne0 % 4 == 0 and ne0 <= 16384");
    return glue_plan(GK_RMS_NORM, GL_RMS_NORM, rows, 256, w != nullptr);
}

// one block per row (rows up to 8192 values are staged in LDS, longer rows in dst); rows of up to 1024 values, f32 mask, no ALiBi, and
// enough of them: one wave per row, four rows per block, the row in registers
inline GluePlan glue_soft_max_plan(const qmm_tensor * a, const qmm_tensor * mask, const qmm_tensor * d) {
    const uint32_t nc = (uint32_t) a->ne[0], rows = (uint32_t) nrows(d);
    if (f32_param(d, 1) == 0.0f && (!mask || mask->type == G_F32) && nc % 4 == 0 && nc <= 1024 && rows >= 1024 && data_aligned(a, 16) &&
        data_aligned(d, 16) && (!mask || data_aligned(mask, 16))) {
        const int v4 = nc <= 256 ? 1 : nc <= 512 ? 2 : 4;
        return glue_plan(GK_SOFT_MAX_WAVE, v4 == 1 ? GL_SOFT_MAX_WAVE_1 : v4 == 2 ? GL_SOFT_MAX_WAVE_2 : GL_SOFT_MAX_WAVE_4, (rows + 3) / 4, 256, v4);
    }
    GluePlan p = glue_plan(GK_SOFT_MAX, nc <= 8192 ? GL_SOFT_MAX_LDS : GL_SOFT_MAX_DST, rows, 256, mask && mask->type == G_F16);
    p.lds = nc <= 8192 ? (size_t) nc * 4 : 0;
    return p;
}

inline GluePlan glue_cpy_plan(const qmm_tensor * a, const qmm_tensor * d) {
    const uint32_t n = (uint32_t) nelements(a);
    if (n == 0) return glue_nothing();
    if (a->type == d->type && contiguous(a) && contiguous(d)) {
        GluePlan p = glue_nothing(GL_MEMCPY);
        p.kernel = GK_MEMCPY;
        p.launch = a->data != d->data;
        return p;
    }
    // transposed source into dense rows (the V-cache store)
    if (transpose_2d(a, d, 8)) {
        GluePlan p = glue_plan(GK_CPY_TRANSPOSE, GL_CPY_TRANSPOSE, (unsigned) ((a->ne[0] + 31) / 32), 256, a->type, d->type);
        p.grid[1] = (unsigned) ((a->ne[1] + 31) / 32);
        return p;
    }
    return glue_plan(GK_CPY, GL_CPY, (n + 255) / 256, 256, a->type, d->type);
}

// F16 src0: 64 x 64 tiles on the MFMA, 16-byte loads where both operands allow them; F32 src0: few outputs with a long K take a
// workgroup per dst element, everything else a wave
inline GluePlan glue_mul_mat_f_plan(const qmm_tensor * a, const qmm_tensor * b) {
    const int32_t M = (int32_t) a->ne[1], N = (int32_t) b->ne[1], K = (int32_t) a->ne[0];
    const unsigned batch = (unsigned) (b->ne[2] * b->ne[3]);
    GluePlan p;
    if (a->type == G_F16) {
        const bool vec = aligned_to(a, 16) && aligned_to(b, 16);
        p = glue_plan(GK_MUL_MAT_F16, vec ? GL_MUL_MAT_F16_VEC : GL_MUL_MAT_F16_SCALAR, (unsigned) ((M + MM_T - 1) / MM_T), 256, vec);
        p.grid[1] = (unsigned) ((N + MM_T - 1) / MM_T);
    } else {
        const int64_t e = (int64_t) M * N;
        if (e <= 2048 && K >= 1024) p = glue_plan(GK_MUL_MAT_DOT_BLOCK, GL_MUL_MAT_DOT_BLOCK, (unsigned) e, DOT_T);
        else                        p = glue_plan(GK_MUL_MAT_DOT, GL_MUL_MAT_DOT, (unsigned) ((e + 3) / 4), 256, G_F32);
    }
    p.grid[2] = batch;
    return p;
}

// qmm_op_compute, for operands sup_op takes
inline GluePlan glue_op_plan(int op, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * c, const qmm_tensor * d) {
    (void) c;
    if (is_binary(op)) return glue_binary_plan(op, a, b, d);
    if (is_unary(op)) return glue_unary_plan(op, nullptr, d);
    switch (op) {
        case QMM_OP_SILU_MUL:     return glue_unary_plan(QMM_OP_SILU, b, d);
        case QMM_OP_NORM:         return glue_plan(GK_NORM, GL_NORM, (unsigned) nrows(d), 256);
        case QMM_OP_RMS_NORM:     return glue_rms_norm_plan(a, nullptr, nullptr, d, nullptr);
        case QMM_OP_RMS_NORM_MUL: return glue_rms_norm_plan(a, nullptr, b, d, nullptr);
        case QMM_OP_ROPE:         return glue_plan(GK_ROPE, GL_ROPE, ((uint32_t) (nelements(d) / 2) + 255) / 256, 256);      // a thread per pair
        case QMM_OP_SOFT_MAX:     return glue_soft_max_plan(a, b, d);
        case QMM_OP_CPY:          return glue_cpy_plan(a, d);
        case QMM_OP_GET_ROWS:     // one block per dst row
            if (a->type == G_F32 || a->type == G_F16) return glue_plan(GK_GET_ROWS, GL_GET_ROWS, (unsigned) nrows(d), 256, a->type);
            return glue_plan(GK_GET_ROWS_Q, GL_GET_ROWS_Q, (unsigned) nrows(d), 256, a->type);
        case QMM_OP_MUL_MAT_F:    return glue_mul_mat_f_plan(a, b);
        case QMM_OP_ARGSORT:      return glue_plan(GK_ARGSORT, GL_ARGSORT, (unsigned) nrows(a), 256);                         // one block per row
        case QMM_OP_SUM_ROWS:     return glue_plan(GK_SUM_ROWS, GL_SUM_ROWS, ((uint32_t) nrows(a) + 3) / 4, 256);              // one wave per row
        default:                  return glue_plan(GK_NONE, GL_NONE, 0, 0);      // (sup_op takes no other op; run_glue holds no kernel for this)
    }
}

// qmm_op_add_rms_norm
inline GluePlan glue_add_rms_norm_plan(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * sum, const qmm_tensor * dst) {
    return glue_rms_norm_plan(a, b, w, dst, sum);
}

// qmm_rope_kv_store: the grid is the concatenation of the index spaces of q, k and v (k, v optional).  A v part that is a 2-D
// transpose large enough for tiles goes through LDS in blocks behind the rope blocks, one 32 x 32 tile each
inline GluePlan glue_rope_kv_store_plan(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * v_dst) {
    const uint32_t nq = rope_heads_threads(q), nk = k ? rope_heads_threads(k) : 0, nv = v ? (uint32_t) nelements(v) : 0;
    if (v && transpose_2d(v, v_dst, 32)) {
        const uint32_t pair_blocks = (nq + nk + 255) / 256, tiles0 = (uint32_t) ((v->ne[0] + 31) / 32), tiles1 = (uint32_t) ((v->ne[1] + 31) / 32);
        GluePlan p = glue_plan(GK_ROPE_STORE, GL_NONE, pair_blocks + tiles0 * tiles1, 256, true);
        p.karg[0] = pair_blocks;  p.karg[1] = tiles0;
        return p;
    }
    return glue_plan(GK_ROPE_STORE, GL_NONE, (nq + nk + nv + 255) / 256, 256, false);
}

// qmm_moe_router: one wave per token; with the logits (and the norm in front of them, whose row is kept in LDS): one workgroup per token
inline GluePlan glue_moe_router_plan(const qmm_tensor * logits) {
    return glue_plan(GK_MOE_ROUTER, GL_NONE, (unsigned) (((int) logits->ne[1] + 3) / 4), 256);
}
inline GluePlan glue_moe_router_logits_plan(const qmm_tensor * x, bool norm) {
    GluePlan p = glue_plan(GK_MOE_ROUTER_LOGITS, GL_NONE, (unsigned) x->ne[1], 1024, norm);
    p.lds = norm ? (size_t) x->ne[0] * 4 : 0;
    return p;
}

// qmm_moe_combine: a float4 of one token per thread
inline GluePlan glue_moe_combine_plan(const qmm_tensor * x, const qmm_tensor * out) {
    if (!data_aligned(x, 16) || !data_aligned(out, 16)) return glue_refusal(QMM_EINVAL, "qmm_moe_combine: x / out must be 16-byte aligned");
    GluePlan p = glue_plan(GK_MOE_COMBINE, GL_NONE, (unsigned) (((int) x->ne[0] / 4 + 255) / 256), 256);
    p.grid[1] = (unsigned) x->ne[2];
    return p;
}
// qmm_moe_combine_add_rms_norm: one block per token
inline GluePlan glue_moe_combine_add_rms_norm_plan(const qmm_tensor * x) {
    const int nt = row_norm_threads((int) x->ne[2], (int) x->ne[0]);
    return glue_plan(GK_MOE_COMBINE_ADD_NORM, GL_NONE, (unsigned) (int) x->ne[2], (unsigned) nt, nt);
}

} // namespace qmm
