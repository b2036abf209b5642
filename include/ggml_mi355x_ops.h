/*
 * ggml_mi355x_ops.h — C-ABI of the per-layer glue ops that sit either side of the quantized MUL_MAT path
 * (RMS_NORM, ADD/MUL/SUB/DIV, SCALE, UNARY, ROPE, SOFT_MAX, CPY/CONT/DUP, GET_ROWS and the
 * F16/F32 x F32 MUL_MATs of attention), so that a whole transformer layer is one scheduler split and the KV cache
 * lives in HBM.  Same library (libggml_mi355x_qmm.so), same conventions as ggml_mi355x_qmm.h.
 *
 * Reference interface this mirrors: the cDSP entry points take three tensor descriptors,
 *     int ggmlop_dsp_add    (remote_handle64, const dsptensor * src0, const dsptensor * src1, dsptensor * dst)
 *     int ggmlop_dsp_softmax(...), ggmlop_dsp_rmsnorm(...)        (kernels/ggmlop_ap_skel.h:267-273; bodies
 *     kernels/ggml-dsp.c:991-1089 (add), :1353-1365 (softmax / rmsnorm are empty stubs there))
 * with `dsptensor` = {type, ne[4], nb[4], op, op_params[16], flags, data, data_len} (ggmlop_ap_skel.h:234-244).
 * `qmm_tensor` is that descriptor for this boundary (64-bit extents, device pointer).  Semantics of every op are those
 * of the ggml CPU backend (file:line at each kernel in csrc/qmm_ops.hip); parity is checked by the reference's own
 * tests/test-backend-ops.cpp against the CPU backend.
 */
#ifndef GGML_MI355X_OPS_H
#define GGML_MI355X_OPS_H

#include "ggml_mi355x_qmm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qmm_tensor {
    void *  data;             /* DEVICE pointer */
    int32_t type;             /* ggml_type: F32 = 0, F16 = 1, I32 = 26, quantized types as in ggml_mi355x_qmm.h (TQ1_0 = 34, TQ2_0 = 35 among them) */
    int32_t flags;            /* 0, or QMM_TENSOR_* bits where an entry point names one */
    int64_t ne[4];            /* elements */
    int64_t nb[4];            /* bytes */
    int32_t op_params[16];    /* ggml_tensor::op_params of the node (dst only) */
} qmm_tensor;

/* qmm_tensor::flags.  QMM_TENSOR_KV_ROWS, on the `v` operand of qmm_attn_decode[_supported] and qmm_attn_prefill[_supported] only:
 * v's rows are cache positions, as K's are (the V operand of GGML_OP_FLASH_ATTN_EXT), not the transposed cache.  Any other bit, and
 * this bit on any other operand or entry point, is refused. */
#define QMM_TENSOR_KV_ROWS 1

enum qmm_op {
    QMM_OP_ADD = 1, QMM_OP_SUB, QMM_OP_MUL, QMM_OP_DIV,
    QMM_OP_SCALE,
    QMM_OP_SILU, QMM_OP_GELU, QMM_OP_GELU_QUICK, QMM_OP_RELU, QMM_OP_TANH, QMM_OP_SIGMOID, QMM_OP_NEG, QMM_OP_EXP,
    QMM_OP_RMS_NORM,          /* op_params[0] = eps (f32) */
    QMM_OP_ROPE,              /* src1 = positions (i32), src2 = frequency factors (f32) or NULL; op_params as ggml_rope_ext */
    QMM_OP_SOFT_MAX,          /* src1 = mask (f32 / f16) or NULL; op_params = {scale, max_bias} */
    QMM_OP_CPY,               /* also CONT and DUP: src0 -> dst, any strides, F32 / F16 either side; and for a Q8_0 K cache (type 8, blocks of
                                 one f16 d and 32 int8): F32 (ne0 % 32 == 0, rows dense, any 4-byte strides) -> contiguous Q8_0, the bytes of the
                                 CPU backend's quantize_row_q8_0 in the context's act mode, and Q8_0 (blocks dense in a row, 2-byte strides) ->
                                 contiguous F32 / F16, f32(d) * q; element i of src in src's index order is element i of dst.  The same two
                                 forms for a K cache in Q4_0 / Q4_1 / Q5_0 / Q5_1 (types 2, 3, 6, 7: blocks of 18 / 20 / 22 / 24 bytes, f16 d,
                                 [f16 m], [4 bytes qh], 16 bytes of nibbles): F32 -> type gives the bytes of quantize_row_q4_0_ref / q4_1_ref /
                                 q5_0_ref / q5_1_ref (the CPU backend's from_float for them; no act mode), type -> F32 / F16 the values of
                                 dequantize_row_q4_0 / q4_1 / q5_0 / q5_1 (the f16 form rounded once more) */
    QMM_OP_GET_ROWS,          /* src0 rows (F32 / F16 / every quantized weight type of ggml_mi355x_qmm.h) picked by src1 (i32) -> f32 */
    QMM_OP_MUL_MAT_F,         /* src0 F16 or F32 (any row strides, broadcast over dims 2/3), src1 F32 -> f32 */
    /* fused pairs the plugin forms from consecutive nodes */
    QMM_OP_RMS_NORM_MUL,      /* dst = rms_norm(src0) * src1, src1 one f32 row broadcast over all rows */
    QMM_OP_SILU_MUL,          /* dst = silu(src0) * src1, same shapes, contiguous (SwiGLU of build_ffn) */
    /* the MoE router (build_moe_ffn) */
    QMM_OP_ARGSORT,           /* i32 indices that order each row; op_params[0] = 0 ascending, 1 descending (ggml_top_k = this + a view) */
    QMM_OP_SUM_ROWS,          /* dst [1, ne1, ne2, ne3] = row sums */
    QMM_OP_NORM,              /* LayerNorm without affine part: (x - mean) / sqrt(var + eps), op_params[0] = eps */
    QMM_OP_COUNT
};

/* 1 when the combination of op, types, shapes and strides is implemented, 0 otherwise.  The plugin's supports_op asks this,
 * so the library is the single place that knows the surface.  src1 / src2 may be NULL where the op has none. */
QMM_API int qmm_op_supported(int op, const qmm_tensor * src0, const qmm_tensor * src1, const qmm_tensor * src2,
                             const qmm_tensor * dst);

/* Runs one op on `stream`.  QMM_EUNSUPPORTED for anything qmm_op_supported() rejects; nothing falls back to the CPU. */
QMM_API int qmm_op_compute(qmm_ctx * ctx, int op, const qmm_tensor * src0, const qmm_tensor * src1, const qmm_tensor * src2,
                           const qmm_tensor * dst, void * stream);

/* The residual add that feeds a norm, in one pass: sum = a + b (same shapes), dst = rms_norm(sum) [* w] (w = one f32 row or NULL).
 * Two results, hence its own entry point.  In llama.cpp's layer: ffn_inp = cur + inpSA -> ffn_norm, and the layer's output
 * add -> the next layer's attn_norm (src/llama-model.cpp:4280-4300, 4340-4346). */
QMM_API int qmm_op_add_rms_norm_supported(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * sum,
                                          const qmm_tensor * dst);
QMM_API int qmm_op_add_rms_norm(qmm_ctx * ctx, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * sum,
                                const qmm_tensor * dst, float eps, void * stream);

/* Attention for a batch of up to 8 tokens in one launch: the chain build_attn_mha emits without flash attention
 * (src/llama-graph.cpp:1166-1203): dst = cont(permute(mul_mat(v, soft_max_ext(mul_mat(k, q), mask, scale)), 0, 2, 1, 3)).
 *   q    f32 [D, N, H]       (any row / head strides)        k  f16 [D, n_kv, H_kv]   rows dense, 16-byte aligned
 *   v    f16 [n_kv, Dv, H_kv] the transposed V cache          mask f32 [n_kv, >= N]
 *   dst  f32 [Dv * H, N]
 * D in {64, 128, 256}, n_kv a multiple of 8 (llama.cpp pads it to 32), H a multiple of H_kv (grouped-query attention).
 *
 * With v->flags == QMM_TENSOR_KV_ROWS the operands are those of GGML_OP_FLASH_ATTN_EXT on an F16 cache (build_attn_mha with flash
 * attention, src/llama-graph.cpp:1153-1165; arithmetic of ggml_compute_forward_flash_attn_ext_f16, ggml-cpu.c:10258-10471, with
 * max_bias = 0 and logit_softcap = 0, sums in f32):
 *   q    f32 [D, N, H]       (any row / head strides)        k  f16 [D, n_kv, H_kv]   rows dense, 16-byte aligned
 *   v    f16 [Dv, n_kv, H_kv] rows dense, row and head strides 16-byte aligned, as k
 *   mask f32 or f16 [n_kv, >= N]                             dst f32 [Dv * H, N]       (the op's [Dv, H, N])
 * D = Dv in {64, 128}, n_kv a multiple of 64 up to 16384 (llama.cpp pads it to 256 with flash attention), H a multiple of H_kv.
 *
 * With k->type == 8 (a Q8_0 K cache, llama.cpp's -ctk q8_0 without flash attention; v->flags == 0): the first chain with
 *   k    Q8_0 [D, n_kv, H_kv]  blocks dense in a row (nb[0] == 34), nb[1] and nb[2] multiples of 2 (llama.cpp: nb[2] = 34 D / 32, nb[1] = H_kv nb[2])
 * and every other operand as there.  D in {64, 128}, Dv <= 128, N <= 8, n_kv a multiple of 32 up to 16384.  Scores in the CPU path's arithmetic
 * for a Q8_0 src0: q quantized to Q8_0 per 32 values in the context's act mode, integer dots times d_k * d_q, f32 sums in block order.
 *
 * With k->type in {2, 3, 6, 7} (a K cache in Q4_0 / Q4_1 / Q5_0 / Q5_1; v->flags == 0): the same operands and limits with this type's block
 * size in k->nb[0] (18 / 20 / 22 / 24).  Scores in the CPU path's arithmetic for such a src0: q quantized in the context's act mode to Q8_0
 * (Q4_0 / Q5_0) or Q8_1 (Q4_1 / Q5_1: d and s = d * sum), integer dots, then sumi * d_k * d_q (Q4_0), (d_k * d_q) * sumi (Q5_0),
 * (d_k * d_q) * sumi + m_k * s_q (Q4_1 / Q5_1), every operation rounded on its own, f32 sums in block order. */
QMM_API int qmm_attn_decode_supported(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                                      const qmm_tensor * dst);
QMM_API int qmm_attn_decode(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                            const qmm_tensor * dst, float scale, void * stream);

/* The same chain for a prompt batch of any size whose scores fit LDS (n_kv <= 512, a multiple of 32; D = Dv in {64, 128}): one
 * workgroup per (64 tokens, head) keeps the 64 x n_kv score tile in LDS between the two MFMA products, so the f32 score tensor
 * (33 MB per layer at 512 x 512 x 32 heads) never exists.  Same operands and result layout as qmm_attn_decode.
 * Longer caches are walked 512 columns at a time with a running maximum and sum per token row.
 *
 * With v->flags == QMM_TENSOR_KV_ROWS: the flash-attention operands described at qmm_attn_decode, for any N >= 1; D = Dv in
 * {64, 128}, n_kv a multiple of 64, q rows and heads 16-byte aligned.
 *
 * With k->type == 8 (k as described at qmm_attn_decode, v->flags == 0): D = Dv in {64, 128}, n_kv a multiple of 32.  One launch unpacks the
 * n_kv x H_kv K rows to f16 (k = f16(f32(d) * q)) into the context's workspace, at most 64 MiB of it (2 D n_kv H_kv bytes; beyond: not
 * supported), then the launch above runs on that image: its arithmetic, bit for bit.
 *
 * With k->type in {2, 3, 6, 7} (k as described at qmm_attn_decode, v->flags == 0): the same, the image holding k = f16(dequantize_row_*). */
QMM_API int qmm_attn_prefill_supported(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                                       const qmm_tensor * dst);
QMM_API int qmm_attn_prefill(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                             const qmm_tensor * dst, float scale, void * stream);

/* What follows the q / k / v projections of a few-token batch in build_attn (src/llama-graph.cpp:1306-1365), in one launch:
 *   q_dst = rope(q) (f32; q_dst carries the ROPE node's op_params), k_dst = (f16) rope(k) straight into the K cache view,
 *   v_dst = (f16) v into the (transposed) V cache view, element i of v (in v's index order) to element i of v_dst, as CPY does.
 * k / k_dst and v / v_dst are optional pairs (NULL).  A Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 k_dst is refused here: a quantized
 * K cache is stored by qmm_rope_kq_store below, or by ROPE and QMM_OP_CPY. */
QMM_API int qmm_rope_kv_store_supported(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                                        const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst);
QMM_API int qmm_rope_kv_store(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                              const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst, void * stream);

/* The same on a quantized K cache (-ctk q8_0 / q4_0 / q4_1 / q5_0 / q5_1), any batch size, in one launch: q, pos, ff, q_dst and the optional
 * pair v / v_dst as above (modes normal and NEOX, n_dims <= D, YaRN parameters in q_dst->op_params).  k is required: f32 [D, H_kv, N], dense
 * rows, 4-byte strides and data, D % 32 == 0, D * H_kv <= 8192, ne[0] / ne[2] / ne[3] agreeing with q.  k_dst is required: type 8, 2, 3, 6 or
 * 7, k's extents, contiguous in that type's blocks, data on a 2-byte boundary.  Everything else is refused: an F16 k_dst (qmm_rope_kv_store
 * takes it), IQ4_NL and every other type, rows of partial blocks, a non-contiguous k_dst.
 *   q_dst, v_dst  bit for bit what qmm_rope_kv_store(q, pos, ff, q_dst, NULL, NULL, v, v_dst) writes
 *   k_dst         byte for byte what QMM_OP_ROPE (k -> a contiguous f32 tensor, q_dst's op_params) followed by QMM_OP_CPY (-> k_dst) writes:
 *                 Q8_0 blocks in the context's act mode, the other four as quantize_row_*_ref; no byte outside its blocks is written */
QMM_API int qmm_rope_kq_store_supported(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                                        const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst);
QMM_API int qmm_rope_kq_store(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                              const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst, void * stream);

/* The router of a mixture-of-experts block behind its logits (build_moe_ffn, src/llama-graph.cpp:818-858) as one launch:
 *   ids     i32 [n_expert, n_tokens] = argsort(soft_max(logits), descending); its first n_used entries per row are ggml_top_k
 *   weights f32 [n_used * n_tokens] contiguous = the selected probabilities, divided by their sum when `normalise` (norm_w)
 * logits f32 [n_expert <= 64, n_tokens]. */
QMM_API int qmm_moe_router_supported(const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used);
QMM_API int qmm_moe_router(qmm_ctx * ctx, const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used,
                           int normalise, void * stream);

/* The same with the logits themselves, for up to 8 tokens (token generation): logits = gate_inp [K, n_expert] (F32) x [K, n_tokens],
 * written to `logits` with the bits qmm_op(MUL_MAT) gives, then the router above; one launch for build_moe_ffn's first six nodes. */
QMM_API int qmm_moe_router_logits_supported(const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * logits, const qmm_tensor * ids,
                                            const qmm_tensor * weights, int64_t n_used);
QMM_API int qmm_moe_router_logits(qmm_ctx * ctx, const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * logits, const qmm_tensor * ids,
                                  const qmm_tensor * weights, int64_t n_used, int normalise, void * stream);
/* ... and with the RMS norm in front of it (build_moe_ffn's input is ffn_norm = rms_norm(ffn_inp) * w, src/llama-model.cpp:4301-4305): `x` is the
 * un-normed row [K <= 16384, n_tokens <= 8], `normed` receives rms_norm(x, eps) * norm_w with the bits qmm_op(RMS_NORM_MUL) gives (the expert
 * MUL_MAT_IDs read it), the logits are taken against it.  `normed` may be `x` itself (same rows) and nothing else that overlaps it. */
QMM_API int qmm_moe_router_logits_norm_supported(const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * norm_w, const qmm_tensor * normed,
                                                 const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used);
QMM_API int qmm_moe_router_logits_norm(qmm_ctx * ctx, const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * norm_w, float eps,
                                       const qmm_tensor * normed, const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights,
                                       int64_t n_used, int normalise, void * stream);

/* The other end of the block: out [E, n_tokens] = sum over the used experts of x [E, n_used, n_tokens] * w [1, n_used, n_tokens]
 * (ggml_mul by the router weights, then the ggml_add chain over 2-D views, src/llama-graph.cpp:896-911), in the graph's order. */
QMM_API int qmm_moe_combine_supported(const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * out);
QMM_API int qmm_moe_combine(qmm_ctx * ctx, const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * out, void * stream);
/* ... with the residual add and the RMS norm that follow the block in the layer (src/llama-model.cpp:4318-4330, 4216: ffn_moe_out + ffn_inp
 * -> l_out, then the next attn_norm or result_norm): sum [E, n_tokens] = combine(x, w) + b, dst = rms_norm(sum) * nw [E]; one launch,
 * both results the bits of qmm_moe_combine followed by qmm_op_add_rms_norm.  With one token (one workgroup) sum and dst may overlap any input
 * (all inputs are read before the first store); with more tokens they must be clear of x and w, and of b except as the very same rows. */
QMM_API int qmm_moe_combine_add_rms_norm_supported(const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * b, const qmm_tensor * nw,
                                                   const qmm_tensor * sum, const qmm_tensor * dst);
QMM_API int qmm_moe_combine_add_rms_norm(qmm_ctx * ctx, const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * b, const qmm_tensor * nw,
                                         const qmm_tensor * sum, const qmm_tensor * dst, float eps, void * stream);

/* qmm_rope_kv_store and qmm_attn_decode as ONE launch for a batch of up to 8 tokens (normal-mode RoPE over the whole head,
 * D <= 128): q [D, H, N] arrives un-roped (q_rope: the ROPE node's descriptor, for its op_params), k_new [D, H_kv, N] and
 * v_new (v_cur^T, [N, Dv * H_kv]) are the batch's projections, k_store / v_store where qmm_rope_kv_store would put them, k / v the
 * cache views the attention reads, j0 the cache row of the batch's first token.  Every workgroup forms the new rows it needs
 * itself and takes them from LDS, so nothing reads rows j0 .. j0 + N of the cache while one workgroup per kv head stores them.
 * F16 caches only: a Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 k_store or k is refused. */
QMM_API int qmm_attn_decode_rope_supported(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_rope,
                                           const qmm_tensor * k_new, const qmm_tensor * k_store, const qmm_tensor * v_new,
                                           const qmm_tensor * v_store, const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask,
                                           const qmm_tensor * dst, int64_t j0);
QMM_API int qmm_attn_decode_rope(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_rope,
                                 const qmm_tensor * k_new, const qmm_tensor * k_store, const qmm_tensor * v_new, const qmm_tensor * v_store,
                                 const qmm_tensor * k, const qmm_tensor * v, const qmm_tensor * mask, const qmm_tensor * dst, float scale,
                                 int64_t j0, void * stream);

#ifdef __cplusplus
}
#endif
#endif
