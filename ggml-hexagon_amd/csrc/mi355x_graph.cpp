// mi355x_graph.cpp — the graph pass: which ops the device takes, the glue ops, flash attention, the reader analysis, graph_compute
// (the fusion sites: mi355x_sites.cpp; the MUL_MAT / MUL_MAT_ID launches themselves: mi355x_mulmat.cpp).
#include "mi355x_internal.h"

namespace mi355x {

// ----------------------------------------------------------------------------------------------- ops

// IQ3_XXS / IQ3_S / IQ2_XS / IQ2_S / IQ1_S / IQ1_M: taken once every registered device holds the type's grid (ggml-mi355x.cpp derives it from ggml at registration and
// hands it to qmm_set_codebook); a kernel library without that entry point, or a grid that does not pass the checks, leaves them to the CPU
bool g_codebook_ok[5] = { false, false, false, false, false };
static bool codebook_type(enum ggml_type t) {
    return t == GGML_TYPE_IQ3_XXS || t == GGML_TYPE_IQ3_S || t == GGML_TYPE_IQ2_XS || t == GGML_TYPE_IQ2_S || t == GGML_TYPE_IQ1_S || t == GGML_TYPE_IQ1_M;
}

bool type_supported(enum ggml_type t) {
    if (t == GGML_TYPE_IQ3_XXS) return g_codebook_ok[0];
    if (t == GGML_TYPE_IQ3_S)   return g_codebook_ok[1];
    if (t == GGML_TYPE_IQ2_XS)  return g_codebook_ok[2];
    if (t == GGML_TYPE_IQ2_S)   return g_codebook_ok[3];
    if (t == GGML_TYPE_IQ1_S || t == GGML_TYPE_IQ1_M) return g_codebook_ok[4];             // one grid, both formats
    // the north-star's five formats plus SURVEY 8f-4's (round 2): any stock Q4_1 / Q5_0 / Q5_1 / Q2_K / Q3_K_* / IQ4_NL GGUF keeps its
    // matmul weights on the device; the kernel library answers the same question through qmm_row_size() != 0
    return t == GGML_TYPE_Q4_0 || t == GGML_TYPE_Q8_0 || t == GGML_TYPE_Q4_K || t == GGML_TYPE_Q5_K || t == GGML_TYPE_Q6_K ||
           t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q2_K || t == GGML_TYPE_Q3_K || t == GGML_TYPE_IQ4_NL || t == GGML_TYPE_IQ4_XS ||
           t == GGML_TYPE_TQ1_0 || t == GGML_TYPE_TQ2_0 ||      // the ternary file types: no grid, taken unconditionally
           t == GGML_TYPE_BF16;          // unquantized checkpoints: MUL_MAT only (supports_mul_mat_id refuses it), and no fold takes it (bf16_weight)
}

// A BF16 weight: the library runs it through kernels of their own (rows of K bf16 values, K in multiples of 32, rows on 16-byte
// boundaries) that fold no neighbour in.  Every fusion site that would hand a norm, a residual or a SwiGLU to a MUL_MAT group asks
// this first and leaves the neighbours to their own launches.
bool bf16_weight(const struct ggml_tensor * w) { return w && w->type == GGML_TYPE_BF16; }

bool is_ours(const struct ggml_tensor * t) {
    ggml_backend_buffer_t b = t->view_src ? t->view_src->buffer : t->buffer;
    return b && b->buft->iface.get_name == buft_get_name;
}

// src0 rows must be whole rows of blocks, src1/dst dense f32 rows
bool mul_mat_shape_ok(const struct ggml_tensor * op) {
    const ggml_tensor * a = op->src[0], * b = op->src[1];
    if (!a || !b || !type_supported(a->type) || b->type != GGML_TYPE_F32 || op->type != GGML_TYPE_F32) return false;
    if (a->ne[0] % ggml_blck_size(a->type) || a->ne[0] != b->ne[0]) return false;
    if (a->nb[0] != ggml_type_size(a->type) || a->nb[1] < ggml_row_size(a->type, a->ne[0])) return false;
    if (a->nb[1] % 2 || a->nb[2] % 2 || a->nb[3] % 2) return false;
    if (bf16_weight(a) && (a->ne[0] % 32 || a->nb[1] % 16 || a->nb[2] % 16 || a->nb[3] % 16 || (uintptr_t) a->data % 16)) return false;
    if (b->nb[0] != sizeof(float) || b->nb[1] % 16 || b->nb[2] % 16 || b->nb[3] % 16) return false;
    if (op->nb[0] != sizeof(float) || op->nb[1] % 4 || op->nb[1] < op->ne[0] * sizeof(float)) return false;
    return true;
}


bool supports_mul_mat(const struct ggml_tensor * op) {
    if (!mul_mat_shape_ok(op)) return false;
    const ggml_tensor * a = op->src[0], * b = op->src[1];
    if (is_split(a) && (a->ne[2] != 1 || a->ne[3] != 1 || b->ne[2] != 1 || b->ne[3] != 1)) return false;
    if (b->nb[1] < b->ne[0] * sizeof(float)) return false;                          // transposed / permuted src1
    if (b->ne[2] % a->ne[2] || b->ne[3] % a->ne[3]) return false;
    // a Q8_0 / Q4_0 / Q4_1 / Q5_0 / Q5_1 src0 may be permuted / strided in dims 1-3 (the view of a K cache of that type that kq reads;
    // mul_mat_shape_ok has asked for dense blocks and even strides): issue_mul_mat_broadcast takes one row stride per (i12, i13) and runs
    // the ggml-layout units, since weight_type never re-lays a tensor outside a weights buffer (nor a view that cuts a weight's rows)
    if (kcache_block_type(a->type) && !is_split(a)) return true;
    if (a->nb[2] < a->nb[1] * (size_t) a->ne[1] || (a->ne[3] > 1 && a->nb[3] < a->nb[2] * (size_t) a->ne[2])) return false;   // permuted src0
    return true;
}

bool supports_mul_mat_id(const struct ggml_tensor * op) {
    const ggml_tensor * as = op->src[0], * b = op->src[1], * ids = op->src[2];
    if (!mul_mat_shape_ok(op) || !ids || ids->type != GGML_TYPE_I32 || bf16_weight(as)) return false;
    if (is_split(as)) return false;                                                // as in the reference tree (ggml-cuda.cu:1973)
    if (as->ne[3] != 1 || b->ne[3] != 1 || ids->ne[2] != 1 || ids->ne[3] != 1) return false;
    if (ids->nb[0] != sizeof(int32_t) || ids->nb[1] % 4) return false;
    if (b->ne[1] != 1 && b->ne[1] != ids->ne[0]) return false;                     // ne11 broadcast rule (ggml.c:2781-2808)
    if (as->nb[2] < as->nb[1] * (size_t) as->ne[1]) return false;
    if (op->nb[2] % 4) return false;
    return true;
}


// ---- glue ops: everything between the quantized MUL_MATs of a layer, so that a layer is one split.
// The kernel library decides what it implements (qmm_op_supported); this side only translates ggml nodes.

qmm_tensor to_qt(const ggml_tensor * t, const mi355x_backend_ctx * ctx) {
    qmm_tensor q{};
    q.data = t->data;
    if (ctx && !ctx->redirects.empty()) {
        const ggml_tensor * root = root_of(t);
        for (const auto & r : ctx->redirects)
            if (r.t == root) q.data = r.data + ((const char *) t->data - (const char *) root->data);
    }
    q.type = (int32_t) dev_type(t);
    for (int i = 0; i < 4; ++i) { q.ne[i] = t->ne[i]; q.nb[i] = (int64_t) t->nb[i]; }
    memcpy(q.op_params, t->op_params, sizeof(q.op_params));
    return q;
}

// ggml node -> library op; 0 when the node is not a glue op of this backend
int glue_op(const ggml_tensor * node) {
    switch (node->op) {
        case GGML_OP_ADD:      return QMM_OP_ADD;
        case GGML_OP_SUB:      return QMM_OP_SUB;
        case GGML_OP_MUL:      return QMM_OP_MUL;
        case GGML_OP_DIV:      return QMM_OP_DIV;
        case GGML_OP_SCALE:    return QMM_OP_SCALE;
        case GGML_OP_RMS_NORM: return QMM_OP_RMS_NORM;
        case GGML_OP_NORM:     return QMM_OP_NORM;
        case GGML_OP_ROPE:     return QMM_OP_ROPE;
        case GGML_OP_SOFT_MAX: return QMM_OP_SOFT_MAX;
        case GGML_OP_CPY: case GGML_OP_CONT: case GGML_OP_DUP: return QMM_OP_CPY;
        case GGML_OP_GET_ROWS: return QMM_OP_GET_ROWS;
        case GGML_OP_ARGSORT:  return QMM_OP_ARGSORT;
        case GGML_OP_SUM_ROWS: return QMM_OP_SUM_ROWS;
        case GGML_OP_MUL_MAT:  return node->src[0] && (node->src[0]->type == GGML_TYPE_F16 || node->src[0]->type == GGML_TYPE_F32) ? QMM_OP_MUL_MAT_F : 0;
        case GGML_OP_UNARY:
            switch (ggml_get_unary_op(node)) {
                case GGML_UNARY_OP_SILU:       return QMM_OP_SILU;
                case GGML_UNARY_OP_GELU:       return QMM_OP_GELU;
                case GGML_UNARY_OP_GELU_QUICK: return QMM_OP_GELU_QUICK;
                case GGML_UNARY_OP_RELU:       return QMM_OP_RELU;
                case GGML_UNARY_OP_TANH:       return QMM_OP_TANH;
                case GGML_UNARY_OP_SIGMOID:    return QMM_OP_SIGMOID;
                case GGML_UNARY_OP_NEG:        return QMM_OP_NEG;
                case GGML_UNARY_OP_EXP:        return QMM_OP_EXP;
                default:                       return 0;
            }
        default: return 0;
    }
}

// the operands as the library wants them: CPY's dst is src[1]'s layout (the node itself is a view of it)
bool supports_glue(const ggml_tensor * node) {
    const int op = glue_op(node);
    if (!op) return false;
    if (!sw().glue) return false;
    if (op == QMM_OP_GET_ROWS && node->src[0] && codebook_type(node->src[0]->type) && !type_supported(node->src[0]->type)) return false;
    qmm_tensor s[3];
    const qmm_tensor * ps[3] = { nullptr, nullptr, nullptr };
    for (int i = 0; i < 3; ++i)
        if (node->src[i]) { s[i] = to_qt(node->src[i], nullptr); ps[i] = &s[i]; }
    const qmm_tensor d = to_qt(node, nullptr);
    if (op == QMM_OP_CPY) return qmm_op_supported(op, ps[0], nullptr, nullptr, &d) != 0;
    return qmm_op_supported(op, ps[0], ps[1], ps[2], &d) != 0;
}

// the one call of qmm_op_compute, on the context's stream
int op_compute(mi355x_backend_ctx * ctx, int op, const qmm_tensor * s0, const qmm_tensor * s1, const qmm_tensor * s2, const qmm_tensor * d) {
    return qmm_op_compute(ctx->dev->qmm, op, s0, s1, s2, d, qmm_stream(ctx->dev->qmm));
}

enum ggml_status compute_glue(mi355x_backend_ctx * ctx, const ggml_tensor * node, int op, const ggml_tensor * s0, const ggml_tensor * s1,
                              const ggml_tensor * s2) {
    qmm_tensor s[3];
    const qmm_tensor * ps[3] = { nullptr, nullptr, nullptr };
    const ggml_tensor * srcs[3] = { s0, s1, s2 };
    for (int i = 0; i < 3; ++i)
        if (srcs[i]) { s[i] = to_qt(srcs[i], ctx); ps[i] = &s[i]; }
    const qmm_tensor d = to_qt(node, ctx);
    return launched(op_compute(ctx, op, ps[0], ps[1], ps[2], &d), "MI355X %s(%s): %s\n", ggml_op_name(node->op), node->name);
}

// ---- GGML_OP_FLASH_ATTN_EXT (build_attn_mha with flash attention, src/llama-graph.cpp:1153-1165): q f32 [D, N, H], k / v f16
// [D, n_kv, H_kv] (v with cache positions as rows: QMM_TENSOR_KV_ROWS), an f16 mask, dst f32 [Dv, H, N] = the merged heads the attention
// entry points write.  The node goes through those entry points (qmm_attn_decode for up to 8 tokens, qmm_attn_prefill beyond); ALiBi and
// the soft-cap live in op_params only (the library never sees them) and are refused here, like a missing mask and a quantized or BF16 cache.
struct flash_attn_operands { qmm_tensor q, k, v, m, d; };
bool flash_attn_operands_of(const ggml_tensor * node, const mi355x_backend_ctx * ctx, flash_attn_operands & o) {
    const ggml_tensor * q = node->src[0], * k = node->src[1], * v = node->src[2], * m = node->src[3];
    if (!q || !k || !v || !m) return false;
    if (q->type != GGML_TYPE_F32 || k->type != GGML_TYPE_F16 || v->type != GGML_TYPE_F16 || m->type != GGML_TYPE_F16 || node->type != GGML_TYPE_F32) return false;
    float max_bias, logit_softcap;
    memcpy(&max_bias, (const float *) node->op_params + 1, sizeof(float));
    memcpy(&logit_softcap, (const float *) node->op_params + 2, sizeof(float));
    if (max_bias != 0.0f || logit_softcap != 0.0f) return false;
    if (q->ne[3] != 1 || k->ne[3] != 1 || v->ne[3] != 1 || m->ne[2] != 1 || m->ne[3] != 1 || node->ne[3] != 1 || !ggml_is_contiguous(node)) return false;
    o.q = to_qt(q, ctx);  o.k = to_qt(k, ctx);  o.v = to_qt(v, ctx);  o.m = to_qt(m, ctx);  o.d = to_qt(node, ctx);
    o.v.flags = QMM_TENSOR_KV_ROWS;
    o.d.ne[0] = node->ne[0] * node->ne[1];  o.d.ne[1] = node->ne[2];  o.d.ne[2] = 1;         // [Dv, H, N] contiguous = [Dv * H, N]
    o.d.nb[1] = (int64_t) node->nb[2];  o.d.nb[2] = o.d.nb[3] = (int64_t) ggml_nbytes(node);
    return true;
}

bool supports_flash_attn(const ggml_tensor * node) {
    flash_attn_operands o;
    if (!sw().glue || !flash_attn_operands_of(node, nullptr, o)) return false;
    return qmm_attn_decode_supported(&o.q, &o.k, &o.v, &o.m, &o.d) || qmm_attn_prefill_supported(&o.q, &o.k, &o.v, &o.m, &o.d);
}

// The one place that launches attention: qmm_attn_decode when it takes the operands (a few tokens), else qmm_attn_prefill.  `probe_prefill`:
// the caller does not know yet that one of the two takes them (a fusion site; a FLASH_ATTN_EXT node was asked at scheduling time).
// ATTN_DECODE / ATTN_PREFILL: launched; 0: neither takes the operands; -1: the launch failed (logged as `what`(`name`)).
int issue_attention(mi355x_backend_ctx * ctx, const qmm_tensor & q, const qmm_tensor & k, const qmm_tensor & v, const qmm_tensor & m, const qmm_tensor & d,
                    float scale, const char * what, const char * name, bool probe_prefill) {
    qmm_ctx * qc = ctx->dev->qmm;
    const bool few = qmm_attn_decode_supported(&q, &k, &v, &m, &d) != 0;
    if (!few && probe_prefill && !qmm_attn_prefill_supported(&q, &k, &v, &m, &d)) return 0;
    const int rc = few ? qmm_attn_decode(qc, &q, &k, &v, &m, &d, scale, qmm_stream(qc)) : qmm_attn_prefill(qc, &q, &k, &v, &m, &d, scale, qmm_stream(qc));
    if (launched(rc, "MI355X %s(%s): %s\n", what, name) != GGML_STATUS_SUCCESS) return -1;
    return few ? ATTN_DECODE : ATTN_PREFILL;
}

enum ggml_status compute_flash_attn(mi355x_backend_ctx * ctx, const ggml_tensor * node) {
    flash_attn_operands o;
    if (!flash_attn_operands_of(node, ctx, o)) {
        GGML_LOG_ERROR("MI355X FLASH_ATTN_EXT(%s): operands outside the offloaded surface\n", node->name);
        return GGML_STATUS_FAILED;
    }
    float scale;
    memcpy(&scale, node->op_params, sizeof(float));
    return issue_attention(ctx, o.q, o.k, o.v, o.m, o.d, scale, "FLASH_ATTN_EXT", node->name, false) < 0 ? GGML_STATUS_FAILED : GGML_STATUS_SUCCESS;
}

// the analysis step of a graph_compute call
void analyze_readers(mi355x_backend_ctx * ctx, const ggml_cgraph * cgraph) {
    // Reader analysis.  Candidates are the nodes a fusion wants to skip or move: RMS_NORM / SILU (fused into the MUL behind them),
    // kq / soft_max / kqv (the attention launch) and the quantized MUL_MATs (grouped with an earlier one on the same src1).
    // One pass over all operands records, per candidate, how many nodes of this graph read its memory (directly or through
    // views), the last of them, and whether all of them are glue ops (whose operand pointers this file can redirect).
    std::vector<mi355x_backend_ctx::reader_info> & rd = ctx->readers;
    ctx->redirects.clear();
    ctx->hoist_used = 0;
    // Token generation hands over the same graph again and again (same tensors at the same addresses: llama.cpp rebuilds it in the same
    // context memory, ggml-alloc places it the same way; only offsets INTO the KV cache move, and the cache is nobody's candidate): the
    // analysis below depends on nothing but what this signature covers, so an unchanged signature keeps the previous result
    // (58 us per token otherwise, in front of the first launch).
    uint64_t sig = 1469598103934665603ull ^ (uint64_t) cgraph->n_nodes ^ (fuse_off() ? 0x9e3779b97f4a7c15ull : 0);
    auto mix = [&sig](uint64_t v) { sig = (sig ^ v) * 1099511628211ull; };
    for (int i = 0; i < cgraph->n_nodes; ++i) {
        const ggml_tensor * n = cgraph->nodes[i];
        mix((uint64_t) (uintptr_t) n);  mix(n->view_src ? 0 : (uint64_t) (uintptr_t) n->data);      // (views into the KV cache move with every token; they own no memory)
        mix((uint64_t) n->op ^ ((uint64_t) n->flags << 32));  mix((uint64_t) (uintptr_t) n->view_src);
        mix((uint64_t) n->ne[0] ^ ((uint64_t) n->ne[1] << 20) ^ ((uint64_t) n->ne[2] << 40));  mix((uint64_t) n->nb[1] ^ ((uint64_t) n->nb[2] << 24));
        for (int j = 0; j < GGML_MAX_SRC && n->src[j]; ++j) mix((uint64_t) (uintptr_t) n->src[j] + (uint64_t) j);
    }
    if (sig == ctx->readers_sig && ctx->readers_sig_nodes == cgraph->n_nodes) return;
    ctx->readers_sig = sig;
    ctx->readers_sig_nodes = cgraph->n_nodes;
    rd.clear();
    if (!fuse_off()) {
        for (int i = 0; i + 1 < cgraph->n_nodes; ++i) {
            const ggml_tensor * n0 = cgraph->nodes[i];
            if (n0->op == GGML_OP_RMS_NORM || (n0->op == GGML_OP_UNARY && ggml_get_unary_op(n0) == GGML_UNARY_OP_SILU) ||
                n0->op == GGML_OP_SOFT_MAX || n0->op == GGML_OP_MUL_MAT || n0->op == GGML_OP_MUL_MAT_ID || n0->op == GGML_OP_ROPE || n0->op == GGML_OP_MUL ||
                n0->op == GGML_OP_GET_ROWS || n0->op == GGML_OP_SUM_ROWS || n0->op == GGML_OP_ADD || n0->op == GGML_OP_CONT || n0->op == GGML_OP_DIV)
                rd.push_back({ n0, 0, -1, true });
        }
        if (!rd.empty()) {
            auto less = [](const mi355x_backend_ctx::reader_info & x, const ggml_tensor * t) { return x.t < t; };
            std::sort(rd.begin(), rd.end(), [](const auto & x, const auto & y) { return x.t < y.t; });
            for (int i = 0; i < cgraph->n_nodes; ++i) {
                const ggml_tensor * n = cgraph->nodes[i];
                if (is_noop(n)) continue;                                          // a view reads nothing; its readers are found through view_src
                const bool glue = glue_op(n) != 0 || n->op == GGML_OP_FLASH_ATTN_EXT;     // (compute_flash_attn resolves its four operands through to_qt as well)
                // a quantized 2-D MUL_MAT of this device takes its src1 pointer through to_qt as well (form_group)
                const bool mm_src1 = !glue && n->op == GGML_OP_MUL_MAT && n->src[0] && n->src[1] && !is_split(n->src[0]) && n->src[0]->ne[2] == 1 &&
                                     n->src[0]->ne[3] == 1 && n->src[1]->ne[2] == 1 && n->src[1]->ne[3] == 1;
                for (int j = 0; j < GGML_MAX_SRC && n->src[j]; ++j) {
                    const ggml_tensor * root = n->src[j]->view_src ? n->src[j]->view_src : n->src[j];
                    auto it = std::lower_bound(rd.begin(), rd.end(), root, less);
                    if (it != rd.end() && it->t == root) {
                        ++it->uses;
                        it->last_reader = i;
                        it->glue_only = it->glue_only && (glue || (mm_src1 && j == 1 && it->t->op == GGML_OP_CONT));   // (only the merged-heads CONT is sent to the scratch on this account)
                    }
                }
            }
            // Readers OUTSIDE this cgraph.  The scheduler hands a backend one split = a contiguous run of
            // the graph's nodes; a tensor of this split may also be read by a later split (an op this device refuses inside a layer, a
            // weight kept on the CPU with -ot: ggml-backend.cpp:1355-1448 copies such a tensor out of t->data after graph_compute).  The
            // counts above see this split only, so a candidate counts as fully known only where that can be PROVEN: some later node of
            // this cgraph owns memory that overlaps the candidate's.  ggml-alloc plans the whole graph at once and hands a block out
            // again only behind its tensor's last reader anywhere, so every reader then lies between the two nodes, inside this
            // split.  Anything else (nobody here reuses the block: typically the last tensors of a split) may have readers elsewhere: its
            // count is poisoned, no site matches it, it is computed into its own t->data at its own place.
            // One reverse sweep with the union of the later nodes' byte ranges (a compute arena: a handful of intervals).
            std::map<uintptr_t, uintptr_t> & later = ctx->later_ranges;        // start -> end, disjoint
            later.clear();
            for (int i = cgraph->n_nodes - 1; i >= 0; --i) {
                const ggml_tensor * n = cgraph->nodes[i];
                if (!n->data || ggml_is_empty(n)) continue;
                const uintptr_t a = (uintptr_t) n->data, b = a + ggml_nbytes(n);
                auto it = std::lower_bound(rd.begin(), rd.end(), n, less);
                if (it != rd.end() && it->t == n) {
                    auto nx = later.upper_bound(a);                            // first interval starting behind a
                    bool hit = nx != later.end() && nx->first < b;
                    if (!hit && nx != later.begin()) { auto pv = std::prev(nx); hit = pv->second > a; }
                    if (!hit) { it->uses = 1 << 20; it->glue_only = false; }
                }
                if (n->view_src) continue;                                     // views own nothing (in-place results are views of their operand)
                // insert [a, b), merging what it touches
                uintptr_t lo = a, hi = b;
                auto f = later.upper_bound(lo);
                if (f != later.begin() && std::prev(f)->second >= lo) { --f; lo = f->first; }
                while (f != later.end() && f->first <= hi) { hi = std::max(hi, f->second); f = later.erase(f); }
                later[lo] = hi;
            }
        }
    }
}

enum ggml_status graph_compute_once(ggml_backend_t backend, struct ggml_cgraph * cgraph, bool * f16_overflow) {
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    *f16_overflow = false;
    graph_timer * timer = sw().timing ? &ctx->timer : nullptr;
    const uint64_t queued = ++ctx->dev->enq;
    if (timer) timer->begin(cgraph);
    analyze_readers(ctx, cgraph);
    const int n_nodes = cgraph->n_nodes;
    if (timer) timer->analyzed(ctx->dev->qmm);
    const bool chain = sw().chain && !fuse_off();
    if (chain && qmm_chain_begin(ctx->dev->qmm)) {
        GGML_LOG_ERROR("MI355X graph_compute: %s\n", qmm_last_error());
        return GGML_STATUS_FAILED;
    }
    struct chain_guard {            // every return path below stops the recording (and launches what was recorded)
        qmm_ctx * q; bool on;
        ~chain_guard() { if (on) qmm_chain_end(q); }
    } guard{ ctx->dev->qmm, chain };
    std::vector<char> & done = ctx->done;
    done.assign(n_nodes, 0);
    std::vector<const ggml_tensor *> & deferred = ctx->deferred;
    deferred.assign(n_nodes, nullptr);
    graph_pass P{ ctx, cgraph, n_nodes, done, deferred };
    for (int i = 0; i < n_nodes; ++i) {
        struct ggml_tensor * node = cgraph->nodes[i];
        if (done[i] || is_noop(node)) continue;                                      // ggml-hexagon.cpp:5561-5566
        while (!ctx->redirects.empty() && ctx->redirects.front().last_reader < i) ctx->redirects.erase(ctx->redirects.begin());
        if (ctx->redirects.empty()) ctx->hoist_used = 0;       // nothing lives in the scratch any more: the next layer starts at its base again
        enum ggml_status st;
        const int gop = glue_op(node);
        if (gop) {
            const int r = P.offer_to_sites(i, gop);                           // a fusion that starts here (mi355x_sites.cpp), else the node alone
            if (r < 0) return GGML_STATUS_FAILED;
            if (r > 0) continue;
            if (gop == QMM_OP_CPY) {
                st = compute_glue(ctx, node, gop, node->src[0], nullptr, nullptr);
            } else {
                st = compute_glue(ctx, node, gop, node->src[0], node->src[1], node->src[2]);
            }
        } else if (node->op == GGML_OP_MUL_MAT) {
            if (kcache_block_type(node->src[0]->type) && node->src[0]->view_src) {    // kq on a quantized K cache is no glue op: the attention site sees it first
                const int r = P.offer_to_sites(i, 0);
                if (r < 0) return GGML_STATUS_FAILED;
                if (r > 0) continue;
            }
            st = P.issue_mul_mat(i);                                            // may hoist later MUL_MATs
        } else if (node->op == GGML_OP_MUL_MAT_ID) {
            st = P.issue_mul_mat_id(i);
        } else if (node->op == GGML_OP_FLASH_ATTN_EXT) {
            st = compute_flash_attn(ctx, node);                                 // opaque to the fusion sites: its own launch
        } else {
            GGML_LOG_ERROR("MI355X: op %s (%s) is outside the offloaded surface\n", ggml_op_name(node->op), node->name);
            st = GGML_STATUS_FAILED;
        }
        if (st != GGML_STATUS_SUCCESS) return st;
    }
    if (chain) {
        guard.on = false;
        if (qmm_chain_end(ctx->dev->qmm)) {
            GGML_LOG_ERROR("MI355X graph_compute: %s\n", qmm_last_error());
            return GGML_STATUS_FAILED;
        }
    }
    if (timer) timer->issued(ctx->dev->qmm);
    // the scheduler reads results right after graph_compute/synchronize; a bad expert id surfaces here
    if (const int rc = qmm_synchronize(ctx->dev->qmm, qmm_stream(ctx->dev->qmm))) {
        if (rc == QMM_EUNSUPPORTED && strstr(qmm_last_error(), "non-finite") && !ctx->dev->prefill_bf16) {
            *f16_overflow = true;                               // the caller re-issues the graph in bf16
            return GGML_STATUS_FAILED;
        }
        GGML_LOG_ERROR("MI355X graph_compute: %s\n", qmm_last_error());
        return GGML_STATUS_FAILED;
    }
    free_retired();                 // (the root has waited for every device's slice: nothing queued reads an outgrown staging block)
    { std::lock_guard<std::mutex> lock(ctx->dev->ring_mu); ctx->dev->staged_pending = false; }
    if (ctx->dev->enq.load() == queued) ctx->dev->enq_synced.store(queued);
    if (timer) timer->end(ctx->dev->qmm, cgraph);
    return GGML_STATUS_SUCCESS;
}

// a prompt whose f16-mode prefill met a weight block beyond the f16 range (valid GGUF bits: |d * sc * q| >= 65504) used to fail
// llama_decode although token generation on the same model works (the mat-vec path dots integers).  The library reports it at the
// graph's synchronize; the graph is then issued once more in QMM_PREC_BF16, which has f32's range (NMSE <= 5e-4 against the CPU, the
// reference's own bar), and the device stays in that mode: a model with such a block needs it for every prompt.  Re-issuing is safe:
// a graph's leaves and inputs are never reused by ggml-alloc, every other tensor is rewritten by its node, KV-cache stores rewrite the
// same rows with the same values.
// With GGML_MI355X_PREC=q8 (sw().prec_q8) the library's context is in QMM_PREC_Q8_EXACT (qmm_create reads the same switch): Q2_K / Q3_K /
// Q4_K / Q5_K / Q6_K / IQ4_XS prompts dot integers and cannot overflow, so only a weight type that mode runs as f16 on Q8 activations can bring a graph here;
// the retry then moves the device from q8 to bf16, for every type.
enum ggml_status backend_graph_compute(ggml_backend_t backend, struct ggml_cgraph * cgraph) {
    bool overflow = false;
    enum ggml_status st = graph_compute_once(backend, cgraph, &overflow);
    if (st != GGML_STATUS_SUCCESS && overflow) {
        auto * ctx = (mi355x_backend_ctx *) backend->context;
        GGML_LOG_WARN("MI355X: a weight block of this model exceeds the f16 range; prompt batches on %s run in bf16 from here on (" QMM_SWITCH_ENV(PREC) "=bf16 avoids the first attempt)\n",
                      ctx->name.c_str());
        if (qmm_set_precision(ctx->dev->qmm, QMM_PREC_BF16)) return st;
        ctx->dev->prefill_bf16 = true;
        ctx->readers_sig = 0;                                   // (nothing cached depends on the mode; start the attempt from a clean analysis all the same)
        st = graph_compute_once(backend, cgraph, &overflow);
    }
    return st;
}

} // namespace mi355x
