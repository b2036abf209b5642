// mi355x_graph.cpp — the graph pass: which ops the device takes, the reader analysis, the fusion sites, the glue ops, graph_compute
// (the MUL_MAT / MUL_MAT_ID launches themselves: mi355x_mulmat.cpp).
#include "mi355x_internal.h"

namespace mi355x {

// ----------------------------------------------------------------------------------------------- ops

bool type_supported(enum ggml_type t) {
    // the north-star's five formats plus SURVEY 8f-4's (round 2): any stock Q4_1 / Q5_0 / Q5_1 / Q2_K / Q3_K_* / IQ4_NL GGUF keeps its
    // matmul weights on the device; the kernel library answers the same question through qmm_row_size() != 0
    return t == GGML_TYPE_Q4_0 || t == GGML_TYPE_Q8_0 || t == GGML_TYPE_Q4_K || t == GGML_TYPE_Q5_K || t == GGML_TYPE_Q6_K ||
           t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q2_K || t == GGML_TYPE_Q3_K || t == GGML_TYPE_IQ4_NL || t == GGML_TYPE_IQ4_XS ||
           t == GGML_TYPE_BF16;           // unquantized checkpoints: MUL_MAT only (supports_mul_mat_id refuses it), and no fold takes it (bf16_weight)
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
        const ggml_tensor * root = t->view_src ? t->view_src : t;
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
    qmm_tensor s[3];
    const qmm_tensor * ps[3] = { nullptr, nullptr, nullptr };
    for (int i = 0; i < 3; ++i)
        if (node->src[i]) { s[i] = to_qt(node->src[i], nullptr); ps[i] = &s[i]; }
    const qmm_tensor d = to_qt(node, nullptr);
    if (op == QMM_OP_CPY) return qmm_op_supported(op, ps[0], nullptr, nullptr, &d) != 0;
    return qmm_op_supported(op, ps[0], ps[1], ps[2], &d) != 0;
}

enum ggml_status compute_glue(mi355x_backend_ctx * ctx, const ggml_tensor * node, int op, const ggml_tensor * s0, const ggml_tensor * s1,
                              const ggml_tensor * s2) {
    qmm_tensor s[3];
    const qmm_tensor * ps[3] = { nullptr, nullptr, nullptr };
    const ggml_tensor * srcs[3] = { s0, s1, s2 };
    for (int i = 0; i < 3; ++i)
        if (srcs[i]) { s[i] = to_qt(srcs[i], ctx); ps[i] = &s[i]; }
    const qmm_tensor d = to_qt(node, ctx);
    if (qmm_op_compute(ctx->dev->qmm, op, ps[0], ps[1], ps[2], &d, qmm_stream(ctx->dev->qmm))) {
        GGML_LOG_ERROR("MI355X %s(%s): %s\n", ggml_op_name(node->op), node->name, qmm_last_error());
        return GGML_STATUS_FAILED;
    }
    return GGML_STATUS_SUCCESS;
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

enum ggml_status compute_flash_attn(mi355x_backend_ctx * ctx, const ggml_tensor * node) {
    flash_attn_operands o;
    float scale;
    memcpy(&scale, node->op_params, sizeof(float));
    const bool ok = flash_attn_operands_of(node, ctx, o);
    const bool few = ok && qmm_attn_decode_supported(&o.q, &o.k, &o.v, &o.m, &o.d) != 0;
    if (!ok || (few ? qmm_attn_decode(ctx->dev->qmm, &o.q, &o.k, &o.v, &o.m, &o.d, scale, qmm_stream(ctx->dev->qmm))
                    : qmm_attn_prefill(ctx->dev->qmm, &o.q, &o.k, &o.v, &o.m, &o.d, scale, qmm_stream(ctx->dev->qmm)))) {
        GGML_LOG_ERROR("MI355X FLASH_ATTN_EXT(%s): %s\n", node->name, ok ? qmm_last_error() : "operands outside the offloaded surface");
        return GGML_STATUS_FAILED;
    }
    return GGML_STATUS_SUCCESS;
}

// Pairs the library runs as one launch: RMS_NORM -> MUL by a one-row weight (build_norm), SILU -> MUL (build_ffn's SwiGLU).
// Legal only when the first node's result has no other reader: `single_use` is computed per graph in graph_compute.
int fused_pair(const ggml_tensor * n0, const ggml_tensor * n1, const ggml_tensor ** other) {
    if (n1->op != GGML_OP_MUL || (n1->src[0] != n0 && n1->src[1] != n0) || n1->src[0] == n1->src[1]) return 0;
    *other = n1->src[0] == n0 ? n1->src[1] : n1->src[0];
    if (!ggml_are_same_shape(n0, n1) || (n0->flags & GGML_TENSOR_FLAG_OUTPUT)) return 0;
    qmm_tensor a = to_qt(n0->src[0], nullptr), b = to_qt(*other, nullptr), d = to_qt(n1, nullptr);
    memcpy(d.op_params, n0->op_params, sizeof(d.op_params));
    if (n0->op == GGML_OP_RMS_NORM && qmm_op_supported(QMM_OP_RMS_NORM_MUL, &a, &b, nullptr, &d)) return QMM_OP_RMS_NORM_MUL;
    if (n0->op == GGML_OP_UNARY && ggml_get_unary_op(n0) == GGML_UNARY_OP_SILU && qmm_op_supported(QMM_OP_SILU_MUL, &a, &b, nullptr, &d))
        return QMM_OP_SILU_MUL;
    return 0;
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

// The quantized MUL_MATs that read `b` (group_member), looked for among the live nodes from `start` on: n of them, the first `cap` at
// at[]; `all` when they are every reader `b` has in this graph, at least one and at most `cap`.  The scan ends at the first live
// node in front of them that is something else (it reads or runs first: the graph's order stays).  Both hold-back sites pass
// cap = 4, the size of a group (site_add_rms_norm used to stop counting there, the few-token site counted on and compared
// afterwards: the same answer, since every member is a reader).
graph_pass::reader_group graph_pass::scan_reader_group(const ggml_tensor * b, int start, int cap) const {
    reader_group g;
    const auto * ri = info(b);
    for (int j = start; j < n_nodes && j <= start + LOOKAHEAD && ri && g.n < cap; ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (done[j] || is_noop(t)) continue;
        if (group_member(t, b, false)) g.at[g.n++] = j;
        else if (g.n == 0) break;                                          // something else reads or runs first: keep the graph's order
    }
    g.all = ri && g.n >= 1 && g.n == ri->uses;
    for (int m = 0; m < g.n; ++m) g.all = g.all && !bf16_weight(cgraph->nodes[g.at[m]]->src[0]);      // no norm is held back for a BF16 group
    return g;
}

// a MUL whose operand is a SILU that was held back (site_hold_silu): silu(gate) * up in one pass, or folded into the staging of the MUL_MAT behind it
int graph_pass::site_deferred_silu_mul(int i, ggml_tensor * node, int gop) {
    (void) gop;
    enum ggml_status st;
    if (deferred[i]) {
        // MUL whose operand is a SILU that was held back: silu(gate) * up in one pass
        const ggml_tensor * silu = deferred[i];
        const ggml_tensor * gate = silu->src[0], * up = node->src[0] == silu ? node->src[1] : node->src[0];
        // prompt batch, and the product feeds exactly one quantized MUL_MAT right behind it (ffn_down): that MUL_MAT's
        // activation prep reads gate and up itself; no launch and no round trip for the product
        const int j = next_live(i + 1);
        if (j < n_nodes && node->ne[1] > QMM_MATVEC_MAX_N && node->ne[2] == 1 && node->ne[3] == 1 && single_use(node) &&
            !(node->flags & GGML_TENSOR_FLAG_OUTPUT) && !sw().prec_set) {
            const ggml_tensor * mm = cgraph->nodes[j];
            const qmm_tensor qg = to_qt(gate, ctx), qu = to_qt(up, ctx);      // resolved now: a redirect may expire before node j
            if (group_member(mm, node, false) && !bf16_weight(mm->src[0]) && gate->nb[0] == 4 && up->nb[0] == 4 && gate->nb[1] % 16 == 0 && up->nb[1] % 16 == 0 &&
                (uintptr_t) qg.data % 16 == 0 && (uintptr_t) qu.data % 16 == 0) {
                pending_swiglu = { (const float *) qg.data, (const float *) qu.data, (int64_t) (gate->nb[1] / 4), (int64_t) (up->nb[1] / 4), mm };
                return 1;
            }
        }
        st = compute_glue(ctx, node, QMM_OP_SILU_MUL, gate, up, nullptr);
        if (st != GGML_STATUS_SUCCESS) return -1;
        return 1;
    }
    return 0;
}

// SILU read by one MUL further down (build_ffn: gate, silu, up, mul): held back for that MUL
int graph_pass::site_hold_silu(int i, ggml_tensor * node, int gop) {
    (void) gop;
    const ggml_tensor * other = nullptr;
    if (node->op == GGML_OP_UNARY && ggml_get_unary_op(node) == GGML_UNARY_OP_SILU && single_use(node)) {
        // find the MUL that reads it (build_ffn: gate, silu, up, mul): hold the SILU back when nothing in between
        // writes over its input
        int j = i + 1;
        bool safe = true;
        for (; j < n_nodes && j <= i + LOOKAHEAD; ++j) {
            const ggml_tensor * t = cgraph->nodes[j];
            if (t->src[0] == node || t->src[1] == node) break;
            if (!done[j] && !is_noop(t) && ranges_overlap(t, node->src[0])) safe = false;
        }
        if (safe && j < n_nodes && j <= i + LOOKAHEAD && fused_pair(node, cgraph->nodes[j], &other) == QMM_OP_SILU_MUL) {
            deferred[j] = node;
            return 1;
        }
    }
    return 0;
}

// residual ADD -> RMS_NORM -> MUL(w): one launch with two results
int graph_pass::site_add_rms_norm(int i, ggml_tensor * node, int gop) {
    (void) gop;
    const ggml_tensor * other = nullptr;
    if (node->op == GGML_OP_ADD && i + 2 < n_nodes && !fuse_off()) {
        // residual add -> RMS_NORM -> MUL by the norm weight: one pass with two results
        ggml_tensor * rn = cgraph->nodes[i + 1], * mul = cgraph->nodes[i + 2];
        if (rn->op == GGML_OP_RMS_NORM && rn->src[0] == node && single_use(rn) && fused_pair(rn, mul, &other) == QMM_OP_RMS_NORM_MUL) {
            const qmm_tensor a = to_qt(node->src[0], ctx), b = to_qt(node->src[1], ctx), w = to_qt(other, ctx), sum = to_qt(node, ctx), d = to_qt(mul, ctx);
            // A prompt batch whose normed rows are read by ONE group of quantized MUL_MATs right behind the MUL (q / k / v, gate / up) and by
            // nothing else: no launch here; the group's activation prep adds, norms and stores the sum (fold_norm; round 3)
            if (node->ne[1] > QMM_MATVEC_MAX_N && node->ne[2] == 1 && node->ne[3] == 1 && ggml_are_same_shape(node->src[0], node->src[1]) &&
                ggml_are_same_shape(node, node->src[0]) && !sw().prep_norm_off) {
                const reader_group g = scan_reader_group(mul, i + 3, 4);
                const int found = g.n;
                qmm_weight gw[4];
                for (int m = 0; m < found; ++m) {
                    const ggml_tensor * w = cgraph->nodes[g.at[m]]->src[0];
                    gw[m] = qmm_weight{ w->data, (int64_t) w->nb[1], w->ne[1], nullptr, 0, weight_type(ctx, w) };
                }
                const ggml_tensor * x0 = node->src[0], * x1 = node->src[1];
                if (g.all && !(mul->flags & GGML_TENSOR_FLAG_OUTPUT) && !(node->flags & GGML_TENSOR_FLAG_OUTPUT) &&
                    x0->type == GGML_TYPE_F32 && x1->type == GGML_TYPE_F32 && x0->nb[0] == 4 && x1->nb[0] == 4 && node->nb[0] == 4 &&
                    x0->nb[1] % 16 == 0 && x1->nb[1] % 16 == 0 && node->nb[1] % 16 == 0 && (uintptr_t) a.data % 16 == 0 && (uintptr_t) b.data % 16 == 0 &&
                    (uintptr_t) sum.data % 16 == 0 && (uintptr_t) other->data % 16 == 0 &&
                    // the sum is stored while other rows of the operands are still read: in place over an operand only with the same rows
                    early_write_ok(node, { x0 }, x0) && early_write_ok(node, { x1 }, x1) && early_write_ok(node, { other }) &&
                    qmm_mul_mat_group_norm_supported(ctx->dev->qmm, gw, found, node->ne[0], node->ne[1])) {
                    pending_norm = { rn, mul, other, found, node };
                    done[i + 1] = done[i + 2] = 1;
                    if (dbg()) fprintf(stderr, "held back: add + norm (%s, %s) for the prep of %d MUL_MATs\n", node->name, mul->name, found);
                    return 1;
                }
            }
            // `mul`'s buffer is written two nodes early: it may be the block of an ADD operand that dies here (same rows: fine, a
            // workgroup holds its row in registers before it stores; anything else: keep the graph's order)
            const bool e_ok = early_write_ok(mul, { node->src[0], node->src[1], other, node }, nullptr) ||
                              (early_write_ok(mul, { node->src[1], other, node }, nullptr) && early_write_ok(mul, { node->src[0] }, node->src[0])) ||
                              (early_write_ok(mul, { node->src[0], other, node }, nullptr) && early_write_ok(mul, { node->src[1] }, node->src[1]));
            if (e_ok && qmm_op_add_rms_norm_supported(&a, &b, &w, &sum, &d)) {
                if (qmm_op_add_rms_norm(ctx->dev->qmm, &a, &b, &w, &sum, &d, rms_eps(rn), qmm_stream(ctx->dev->qmm))) {
                    GGML_LOG_ERROR("MI355X ADD+RMS_NORM(%s): %s\n", node->name, qmm_last_error());
                    return -1;
                }
                done[i + 1] = done[i + 2] = 1;
                return 1;
            }
        }
    }
    return 0;
}

// kq -> soft_max -> kqv -> permute -> cont (build_attn_mha) as one launch
int graph_pass::site_attention(int i, ggml_tensor * node, int gop) {
    (void) gop;
    if (gop == QMM_OP_MUL_MAT_F && node->src[0]->type == GGML_TYPE_F16 && single_use(node) && !fuse_off()) {
        // kq -> soft_max -> kqv -> permute -> cont (build_attn_mha): one launch, for a few tokens (qmm_attn_decode) and for prompt
        // batches whose scores fit LDS (qmm_attn_prefill)
        int idx[4], k = 0;
        for (int j = i + 1; j < n_nodes && j <= i + 8 && k < 4; ++j) {
            const ggml_tensor * t = cgraph->nodes[j];
            if (t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_TRANSPOSE) continue;
            idx[k++] = j;
        }
        if (k == 4) {
            ggml_tensor * sm = cgraph->nodes[idx[0]], * kqv = cgraph->nodes[idx[1]], * pm = cgraph->nodes[idx[2]], * ct = cgraph->nodes[idx[3]];
            float scale, max_bias;
            memcpy(&scale, (const float *) sm->op_params + 0, sizeof(float));
            memcpy(&max_bias, (const float *) sm->op_params + 1, sizeof(float));
            if (sm->op == GGML_OP_SOFT_MAX && sm->src[0] == node && sm->src[1] && max_bias == 0.0f && single_use(sm) &&
                kqv->op == GGML_OP_MUL_MAT && kqv->src[1] == sm && kqv->src[0]->type == GGML_TYPE_F16 && single_use(kqv) &&
                pm->op == GGML_OP_PERMUTE && pm->src[0] == kqv && pm->ne[0] == kqv->ne[0] && pm->ne[1] == kqv->ne[2] &&
                pm->ne[2] == kqv->ne[1] && ct->op == GGML_OP_CONT && ct->src[0] == pm &&
                ((early_write_ok(ct, { node->src[0], kqv->src[0], sm->src[1] }) && early_write_ok(ct, { node->src[1] }, node->src[1], true)) ||
                 hoist_elsewhere(ctx, ct))) {      // ggml-alloc puts ct across the dead Q blocks in llama.cpp's layers: written to the scratch instead, wo reads it there
                const qmm_tensor q = to_qt(node->src[1], ctx), kk = to_qt(node->src[0], ctx), v = to_qt(kqv->src[0], ctx), m = to_qt(sm->src[1], ctx), d = to_qt(ct, ctx);
                const bool few = qmm_attn_decode_supported(&q, &kk, &v, &m, &d) != 0;
                if (few || qmm_attn_prefill_supported(&q, &kk, &v, &m, &d)) {
                    if (few ? qmm_attn_decode(ctx->dev->qmm, &q, &kk, &v, &m, &d, scale, qmm_stream(ctx->dev->qmm))
                            : qmm_attn_prefill(ctx->dev->qmm, &q, &kk, &v, &m, &d, scale, qmm_stream(ctx->dev->qmm))) {
                        GGML_LOG_ERROR("MI355X attention(%s): %s\n", node->name, qmm_last_error());
                        return -1;
                    }
                    if (dbg()) fprintf(stderr, "fused: attention (%s, %s)\n", few ? "few tokens" : "prompt", node->name);
                    for (int j = 0; j < 4; ++j) done[idx[j]] = 1;
                    return 1;
                }
            }
        }
    }
    return 0;
}

// kqv -> permute -> cont: the product written straight into the merged-heads layout
int graph_pass::site_kqv_into_merged_heads(int i, ggml_tensor * node, int gop) {
    (void) gop;
    if (gop == QMM_OP_MUL_MAT_F && node->src[0]->type == GGML_TYPE_F16 && single_use(node) && !fuse_off() && !done[i]) {
        // kqv -> permute(0, 2, 1, 3) -> cont (build_attn_mha's head merge) at any batch size: the product is written
        // straight into the cont's layout (dst strides of dims 1 and 2 swapped), the copy never runs
        int jp = i + 1;
        while (jp < n_nodes && (cgraph->nodes[jp]->op == GGML_OP_RESHAPE || cgraph->nodes[jp]->op == GGML_OP_VIEW)) ++jp;
        int jc = jp + 1;
        while (jc < n_nodes && (cgraph->nodes[jc]->op == GGML_OP_RESHAPE || cgraph->nodes[jc]->op == GGML_OP_VIEW)) ++jc;
        if (jc < n_nodes) {
            const ggml_tensor * pm = cgraph->nodes[jp], * ct = cgraph->nodes[jc];
            if (pm->op == GGML_OP_PERMUTE && pm->src[0] == node && ct->op == GGML_OP_CONT && ct->src[0] == pm && !done[jc] &&
                pm->ne[0] == node->ne[0] && pm->ne[1] == node->ne[2] && pm->ne[2] == node->ne[1] && node->ne[3] == 1 &&
                ct->type == GGML_TYPE_F32 && ggml_is_contiguous(ct) && ggml_nelements(ct) == ggml_nelements(node) &&
                early_write_ok(ct, { node->src[0], node->src[1] })) {
                qmm_tensor d = to_qt(node, ctx);
                d.data = to_qt(ct, ctx).data;                                 // element (d, n, h) of kqv = element (d, h, n) of the merged result (ct may live in the scratch)
                d.nb[1] = (int64_t) node->ne[0] * node->ne[2] * 4;
                d.nb[2] = (int64_t) node->ne[0] * 4;
                d.nb[3] = (int64_t) ggml_nbytes(ct);
                const qmm_tensor a = to_qt(node->src[0], ctx), b = to_qt(node->src[1], ctx);
                if (qmm_op_supported(QMM_OP_MUL_MAT_F, &a, &b, nullptr, &d)) {
                    if (qmm_op_compute(ctx->dev->qmm, QMM_OP_MUL_MAT_F, &a, &b, nullptr, &d, qmm_stream(ctx->dev->qmm))) {
                        GGML_LOG_ERROR("MI355X MUL_MAT(%s) into merged heads: %s\n", node->name, qmm_last_error());
                        return -1;
                    }
                    done[jc] = 1;
                    return 1;
                }
            }
        }
    }
    return 0;
}

// experts * weights and the sum over the used experts (build_moe_ffn's tail): one launch
int graph_pass::site_moe_combine(int i, ggml_tensor * node, int gop) {
    (void) gop;
    if (node->op == GGML_OP_MUL && node->src[1]->ne[0] == 1 && node->ne[1] >= 2 && node->ne[1] == node->src[1]->ne[1] && node->ne[3] == 1 &&
        !fuse_off()) {
        // experts * weights and the sum over the used experts through 2-D views (build_moe_ffn's tail): one launch
        const int U = (int) node->ne[1];
        const auto * rm = info(node);
        int idx[64], k = 0;
        for (int j = i + 1; j < n_nodes && j <= i + 4 * U + 4 && k < U - 1; ++j) {
            const ggml_tensor * t = cgraph->nodes[j];
            if (done[j] || is_noop(t)) continue;
            if (t->op != GGML_OP_ADD) break;
            idx[k++] = j;
        }
        const auto root = [](const ggml_tensor * t) { return t->view_src ? t->view_src : t; };
        const auto is_slice = [&](const ggml_tensor * v, int u) {           // view_2d(experts, E, N, nb[2], u * nb[1])
            return root(v) == node && v->ne[0] == node->ne[0] && v->ne[1] == node->ne[2] && v->ne[2] == 1 && v->nb[1] == node->nb[2] &&
                   (const char *) v->data == (const char *) node->data + (size_t) u * node->nb[1];
        };
        bool ok = k == U - 1 && rm && rm->uses == U && U <= 64 && !(node->flags & GGML_TENSOR_FLAG_OUTPUT);
        for (int a = 0; ok && a < U - 1; ++a) {
            const ggml_tensor * ad = cgraph->nodes[idx[a]];
            ok = is_slice(ad->src[1], a + 1) && (a == 0 ? is_slice(ad->src[0], 0) : ad->src[0] == cgraph->nodes[idx[a - 1]]) &&
                 (a == U - 2 || (single_use(ad) && !(ad->flags & GGML_TENSOR_FLAG_OUTPUT)));
        }
        if (ok && !sw().moe_combine_norm_off) {
            // Round 3: the residual add, the RMS norm and the norm weight that follow the block in the layer (ffn_moe_out + ffn_inp -> l_out,
            // then the next attn_norm / result_norm) in the same launch: the next three live nodes must be exactly ADD(last, r),
            // RMS_NORM(add), MUL(rms, w).  Never written then: the product, the partial sums, the block's output and the un-weighted
            // norm: each has exactly the readers of the pattern (closed readers: analyze_readers).  Written HERE, U + 2 nodes early,
            // while other workgroups (one per token) still read the expert rows, the weights and the residual: l_out and the normed row
            // must be clear of the experts and the weights (another layout) and may sit on the residual only as the very same rows.
            const ggml_tensor * last = cgraph->nodes[idx[U - 2]];
            const int ja = next_live(idx[U - 2] + 1);
            const ggml_tensor * other = nullptr;
            if (ja + 2 < n_nodes && single_use(last) && !(last->flags & GGML_TENSOR_FLAG_OUTPUT)) {
                ggml_tensor * add = cgraph->nodes[ja], * rn = cgraph->nodes[ja + 1], * mul = cgraph->nodes[ja + 2];
                if (add->op == GGML_OP_ADD && (add->src[0] == last || add->src[1] == last) && add->src[0] != add->src[1] && rn->op == GGML_OP_RMS_NORM &&
                    rn->src[0] == add && single_use(rn) && !(rn->flags & GGML_TENSOR_FLAG_OUTPUT) && fused_pair(rn, mul, &other) == QMM_OP_RMS_NORM_MUL) {
                    const ggml_tensor * r = add->src[0] == last ? add->src[1] : add->src[0];
                    const auto clear_of = [&](const ggml_tensor * t) {
                        return early_write_ok(t, { node->src[0], node->src[1], other }) && (early_write_ok(t, { r }) || early_write_ok(t, { r }, r));
                    };
                    // one token = one workgroup, which holds all its inputs in registers before it stores (moe_combine_add_norm_kernel): the
                    // results may then lie on any input (ggml-alloc does put l_out on the dead router weights and the normed row on the residual)
                    const bool one = add->ne[1] == 1 && add->ne[2] == 1 && add->ne[3] == 1;
                    if ((one || (clear_of(add) && clear_of(mul))) && !ranges_overlap(add, mul)) {
                        const qmm_tensor x = to_qt(node->src[0], ctx), w = to_qt(node->src[1], ctx), qb = to_qt(r, ctx), nw = to_qt(other, ctx), qs = to_qt(add, ctx),
                                         qd = to_qt(mul, ctx);
                        if (qmm_moe_combine_add_rms_norm_supported(&x, &w, &qb, &nw, &qs, &qd)) {
                            if (qmm_moe_combine_add_rms_norm(ctx->dev->qmm, &x, &w, &qb, &nw, &qs, &qd, rms_eps(rn), qmm_stream(ctx->dev->qmm))) {
                                GGML_LOG_ERROR("MI355X MoE combine + ADD + RMS_NORM(%s): %s\n", node->name, qmm_last_error());
                                return -1;
                            }
                            if (dbg()) fprintf(stderr, "fused: moe combine + add + rms_norm (%s)\n", add->name);
                            for (int a = 0; a < U - 1; ++a) done[idx[a]] = 1;
                            done[ja] = done[ja + 1] = done[ja + 2] = 1;
                            return 1;
                        }
                    }
                }
            }
        }
        if (ok) {
            const ggml_tensor * last = cgraph->nodes[idx[U - 2]];
            // the launch writes the LAST add's buffer at the MUL's position, while other workgroups still read the experts and the
            // weights: ggml-alloc may have put it on either (both are dead at the add's place in the graph).  A token's U expert
            // rows and its one output row are laid out differently, so not even the same address is in place
            if (!early_write_ok(last, { node->src[0], node->src[1] }) && !hoist_elsewhere(ctx, last)) return 0;
            const qmm_tensor x = to_qt(node->src[0], ctx), w = to_qt(node->src[1], ctx), o = to_qt(last, ctx);
            if (qmm_moe_combine_supported(&x, &w, &o)) {
                if (qmm_moe_combine(ctx->dev->qmm, &x, &w, &o, qmm_stream(ctx->dev->qmm))) {
                    GGML_LOG_ERROR("MI355X MoE combine(%s): %s\n", node->name, qmm_last_error());
                    return -1;
                }
                for (int a = 0; a < U - 1; ++a) done[idx[a]] = 1;
                return 1;
            }
        }
    }
    return 0;
}

// soft_max -> argsort -> get_rows -> sum_rows -> div behind the router logits: one launch
int graph_pass::site_moe_router(int i, ggml_tensor * node, int gop) {
    (void) gop;
    // entered one node earlier, at the logits' own MUL_MAT (F32 gate_inp, a few tokens), the launch computes the logits too
    // (qmm_moe_router_logits, round 3): the logits land in their own buffer at their own place in the graph, so nothing about them
    // changes for any other reader; the ids and the weights are written one node earlier than before, now also beside the reads of
    // the MUL_MAT's src1, which joins the operands they must stay clear of
    ggml_tensor * lgt = nullptr;
    // ... and entered two nodes before that, at the RMS norm whose product with ffn_norm's weights is the logits' src1 (the MoE branch of
    // the layer, src/llama-model.cpp:4301-4305), the launch forms the normed row too and stores it for the expert MUL_MAT_IDs
    // (qmm_moe_router_logits_norm): the separate norm launch (4.75 us of a Mixtral layer's ~84) is gone
    ggml_tensor * nrm = nullptr, * nmul = nullptr;
    const ggml_tensor * nwgt = nullptr;
    int i_nmul = -1, i_lgt = -1;
    if (node->op == GGML_OP_RMS_NORM && i + 2 < n_nodes && node->ne[1] <= 8 && node->ne[2] == 1 && node->ne[3] == 1 && single_use(node) && !fuse_off() &&
        !sw().router_norm_off && !sw().router_logits_off) {
        ggml_tensor * m = cgraph->nodes[i + 1];
        const int j2 = next_live(i + 2);                                        // (the 3-D reshape of the normed row for the expert MUL_MAT_IDs sits in between)
        if (j2 >= n_nodes || done[i + 1] || fused_pair(node, m, &nwgt) != QMM_OP_RMS_NORM_MUL) return 0;
        ggml_tensor * t = cgraph->nodes[j2];
        if (t->op != GGML_OP_MUL_MAT || t->src[1] != m || t->src[0]->type != GGML_TYPE_F32 || (m->flags & GGML_TENSOR_FLAG_OUTPUT)) return 0;
        nrm = node;  nmul = m;  i_nmul = i + 1;  i_lgt = j2;
        i = j2;
        node = t;
    }
    if (node->op == GGML_OP_MUL_MAT && node->src[0]->type == GGML_TYPE_F32 && node->src[1]->type == GGML_TYPE_F32 && node->type == GGML_TYPE_F32 && node->ne[0] <= 64 &&
        node->ne[1] <= 8 && node->ne[2] == 1 && node->ne[3] == 1 && !fuse_off() && !sw().router_logits_off) {
        const int j = next_live(i + 1);
        if (j >= n_nodes || cgraph->nodes[j]->op != GGML_OP_SOFT_MAX || cgraph->nodes[j]->src[0] != node) return 0;
        lgt = node;
        i = j;
        node = cgraph->nodes[j];
    } else if (nrm) {
        if (dbg()) fprintf(stderr, "fusion declined: moe router with its norm (%s): not the logits' MUL_MAT\n", nmul->name);
        return 0;
    }
    if (node->op == GGML_OP_SOFT_MAX && !node->src[1] && node->ne[0] <= 64 && node->ne[2] == 1 && node->ne[3] == 1 && !fuse_off()) {
        // the MoE router behind its logits (build_moe_ffn): soft_max -> argsort (top_k view) -> get_rows -> sum_rows -> div
        float scale, max_bias;
        memcpy(&scale, (const float *) node->op_params + 0, sizeof(float));
        memcpy(&max_bias, (const float *) node->op_params + 1, sizeof(float));
        // llama.cpp's graph order puts get_rows / sum_rows / div (the weights, needed only by the final mul) BEHIND the expert
        // MUL_MAT_IDs: the argsort follows the soft_max directly, the other three are looked for further down and run here,
        // early (their inputs exist; where the div's buffer is still in use at this point the weights go to the scratch)
        const auto root = [](const ggml_tensor * t) { return t->view_src ? t->view_src : t; };
        int idx[4], k = 0;
        std::vector<const ggml_tensor *> & skipped = ctx->skipped;
        skipped.clear();
        for (int j = i + 1; j < n_nodes && j <= i + 64 && k < 4; ++j) {
            const ggml_tensor * t = cgraph->nodes[j];
            if (done[j] || is_noop(t)) continue;
            const bool want = (k == 0 && t->op == GGML_OP_ARGSORT && t->src[0] == node) ||
                              (k == 1 && t->op == GGML_OP_GET_ROWS && root(t->src[0]) == node && root(t->src[1]) == cgraph->nodes[idx[0]]) ||
                              (k == 2 && t->op == GGML_OP_SUM_ROWS && root(t->src[0]) == cgraph->nodes[idx[1]]) ||
                              (k == 3 && t->op == GGML_OP_DIV && root(t->src[0]) == cgraph->nodes[idx[1]] && t->src[1] == cgraph->nodes[idx[2]]);
            if (want) idx[k++] = j;
            else if (k == 0) break;                                             // the argsort must come first
            else skipped.push_back(t);
        }
        if (k == 4 && scale == 1.0f && max_bias == 0.0f) {
            ggml_tensor * as = cgraph->nodes[idx[0]], * gr = cgraph->nodes[idx[1]], * sr = cgraph->nodes[idx[2]], * dv = cgraph->nodes[idx[3]];
            const auto * ri = info(node), * rg = info(gr), * rs = info(sr);
            if (as->op == GGML_OP_ARGSORT && as->src[0] == node && as->op_params[0] == GGML_SORT_ORDER_DESC &&
                gr->op == GGML_OP_GET_ROWS && root(gr->src[0]) == node && gr->src[0]->ne[0] == 1 && root(gr->src[1]) == as &&
                gr->src[1]->data == as->data && gr->src[1]->nb[1] == as->nb[1] && gr->src[1]->ne[1] == as->ne[1] &&
                sr->op == GGML_OP_SUM_ROWS && root(sr->src[0]) == gr && dv->op == GGML_OP_DIV && root(dv->src[0]) == gr && dv->src[1] == sr &&
                ri && ri->uses == 2 && rg && rg->uses == 2 && rs && rs->uses == 1 && ggml_is_contiguous(dv) && ggml_is_contiguous(gr) &&
                !(node->flags & GGML_TENSOR_FLAG_OUTPUT) && !(gr->flags & GGML_TENSOR_FLAG_OUTPUT) && !(sr->flags & GGML_TENSOR_FLAG_OUTPUT)) {
                const int64_t n_used = gr->src[1]->ne[0];
                // the ids are written while other waves (one per token) still read logits rows: in place only at the very same address
                // with the same rows (a wave reads its row first).  The weights are written now, not at the div's place in the graph:
                // their block must be free here AND clear of the logits: at the div's place the logits are dead, so a non-inplace
                // dv may sit on them with rows of 4 * n_used bytes against 4 * n_expert; otherwise into the scratch
                if (!early_write_ok(as, { node->src[0], lgt ? lgt->src[1] : nullptr, lgt ? lgt->src[0] : nullptr }, node->src[0])) return 0;
                if (!(can_hoist(dv, skipped) && early_write_ok(dv, { node->src[0], as, lgt ? lgt->src[1] : nullptr, lgt ? lgt->src[0] : nullptr })) && !hoist_elsewhere(ctx, dv)) return 0;
                const qmm_tensor lg = to_qt(node->src[0], ctx), ids = to_qt(as, ctx), w = to_qt(dv, ctx);
                if (nrm) {
                    // the normed row is written where the MUL would put it, two nodes early and beside this launch's reads of the un-normed
                    // rows (in place over them is fine: a workgroup holds its row in registers before it stores) and of the weights; the
                    // router's outputs stay clear of all of them
                    const ggml_tensor * x0 = nrm->src[0];
                    if (!(early_write_ok(nmul, { nwgt, lgt->src[0] }) && early_write_ok(nmul, { x0 }, x0))) return 0;
                    if (!early_write_ok(lgt, { x0, nwgt, nmul, lgt->src[0] }) || !early_write_ok(as, { x0, nwgt, nmul }) ||
                        (to_qt(dv, ctx).data == dv->data && !early_write_ok(dv, { x0, nwgt, nmul }))) return 0;
                    const qmm_tensor gi = to_qt(lgt->src[0], ctx), xin = to_qt(x0, ctx), nw = to_qt(nwgt, ctx), ny = to_qt(nmul, ctx);
                    if (!is_ours(lgt->src[0]) || is_split(lgt->src[0]) || !qmm_moe_router_logits_norm_supported(&gi, &xin, &nw, &ny, &lg, &ids, &w, n_used)) {
                        if (dbg()) fprintf(stderr, "fusion declined: moe router with its norm (%s): operands not supported\n", nmul->name);
                        return 0;
                    }
                    if (qmm_moe_router_logits_norm(ctx->dev->qmm, &gi, &xin, &nw, rms_eps(nrm), &ny, &lg, &ids, &w, n_used, 1, qmm_stream(ctx->dev->qmm))) {
                        GGML_LOG_ERROR("MI355X MoE router with norm and logits(%s): %s\n", node->name, qmm_last_error());
                        return -1;
                    }
                    if (dbg()) fprintf(stderr, "fused: moe router (%s) with its logits (%s) and their norm (%s)\n", node->name, lgt->name, nmul->name);
                    done[i_nmul] = done[i_lgt] = done[i] = 1;                   // mul, logits, soft_max; the caller entered with the norm
                    for (int j = 0; j < 4; ++j) done[idx[j]] = 1;
                    return 1;
                }
                if (lgt) {
                    const qmm_tensor gi = to_qt(lgt->src[0], ctx), xin = to_qt(lgt->src[1], ctx);
                    if (!is_ours(lgt->src[0]) || is_split(lgt->src[0]) || !qmm_moe_router_logits_supported(&gi, &xin, &lg, &ids, &w, n_used)) return 0;
                    if (qmm_moe_router_logits(ctx->dev->qmm, &gi, &xin, &lg, &ids, &w, n_used, 1, qmm_stream(ctx->dev->qmm))) {
                        GGML_LOG_ERROR("MI355X MoE router with logits(%s): %s\n", node->name, qmm_last_error());
                        return -1;
                    }
                    if (dbg()) fprintf(stderr, "fused: moe router (%s) with its logits (%s)\n", node->name, lgt->name);
                    done[i] = 1;                                                // the soft_max; the caller marks the MUL_MAT it entered with
                    for (int j = 0; j < 4; ++j) done[idx[j]] = 1;
                    return 1;
                }
                if (qmm_moe_router_supported(&lg, &ids, &w, n_used)) {
                    if (qmm_moe_router(ctx->dev->qmm, &lg, &ids, &w, n_used, 1, qmm_stream(ctx->dev->qmm))) {
                        GGML_LOG_ERROR("MI355X MoE router(%s): %s\n", node->name, qmm_last_error());
                        return -1;
                    }
                    if (dbg()) fprintf(stderr, "fused: moe router (%s)\n", node->name);
                    for (int j = 0; j < 4; ++j) done[idx[j]] = 1;
                    return 1;
                }
            }
        }
    }
    return 0;
}

// rope(q) with rope(k) -> K cache, v -> V cache and, for a few tokens, the attention: one launch
int graph_pass::site_rope_kv_attention(int i, ggml_tensor * node, int gop) {
    (void) gop;
    if (node->op == GGML_OP_ROPE && !fuse_off()) {
        // rope(q) with, from further down the graph, rope(k) -> K cache and v -> V cache (build_attn's two ggml_cpy): one launch
        // (any batch size: at 512 tokens 29 us of four launches become one, pp512 31.2k -> 32.0k).
        // Their inputs must exist already (k and v were hoisted into the q/k/v group); the cache is not compute-buffer
        // memory, so storing early cannot collide with anything in between.
        auto ready = [&](const ggml_tensor * t) {                            // was t's root produced before this point?
            const ggml_tensor * root = t->view_src ? t->view_src : t;
            for (int j = i + 1; j < n_nodes && j <= i + 2 * LOOKAHEAD; ++j)
                if (cgraph->nodes[j] == root) return done[j] != 0;
            return true;
        };
        int jk = -1, jck = -1, jcv = -1;
        for (int j = i + 1; j < n_nodes && j <= i + 2 * LOOKAHEAD; ++j) {
            const ggml_tensor * t = cgraph->nodes[j];
            if (done[j] || is_noop(t)) continue;
            if (jk < 0 && t->op == GGML_OP_ROPE && t->src[1] == node->src[1] && t->src[2] == node->src[2] && t->ne[0] == node->ne[0] &&
                !memcmp(t->op_params, node->op_params, sizeof(t->op_params)) && t->type == GGML_TYPE_F32 && ggml_is_contiguous(t) &&
                single_use(t) && ready(t->src[0])) {
                jk = j;
            } else if (jk >= 0 && jck < 0 && t->op == GGML_OP_CPY && t->src[0] == cgraph->nodes[jk] && t->type == GGML_TYPE_F16 && ggml_is_contiguous(t)) {
                jck = j;
            } else if (jcv < 0 && t->op == GGML_OP_CPY && t->type == GGML_TYPE_F16 && t->src[0]->type == GGML_TYPE_F32 &&
                       (t->src[0]->view_src ? t->src[0]->view_src : t->src[0])->op == GGML_OP_MUL_MAT && ready(t->src[0]) &&
                       (jk < 0 || t->src[0] != cgraph->nodes[jk])) {
                jcv = j;
            } else if (t->op == GGML_OP_MUL_MAT || t->op == GGML_OP_SOFT_MAX || t->op == GGML_OP_FLASH_ATTN_EXT) {
                break;                                                         // attention starts: nothing to find beyond
            }
        }
        if (jk >= 0 && jck < 0) jk = -1;                                       // rope(k) without its store stays where it is
        if (jk >= 0 || jcv >= 0) {
            const qmm_tensor q = to_qt(node->src[0], ctx), pos = to_qt(node->src[1], ctx), qd = to_qt(node, ctx);
            qmm_tensor ff{}, k{}, kd{}, v{}, vd{};
            if (node->src[2]) ff = to_qt(node->src[2], ctx);
            if (jk >= 0) {
                const ggml_tensor * rk = cgraph->nodes[jk];
                k = to_qt(rk->src[0], ctx);
                kd = to_qt(rk, ctx);                                           // shape of rope(k), bytes of the cache view
                kd.data = cgraph->nodes[jck]->data;
                kd.type = GGML_TYPE_F16;
                kd.nb[0] = 2;
                for (int a = 1; a < 4; ++a) kd.nb[a] = kd.nb[a - 1] * kd.ne[a - 1];
            }
            if (jcv >= 0) {
                v = to_qt(cgraph->nodes[jcv]->src[0], ctx);
                vd = to_qt(cgraph->nodes[jcv], ctx);
            }
            const qmm_tensor * pff = node->src[2] ? &ff : nullptr, * pk = jk >= 0 ? &k : nullptr, * pkd = jk >= 0 ? &kd : nullptr,
                             * pv = jcv >= 0 ? &v : nullptr, * pvd = jcv >= 0 ? &vd : nullptr;
            // ... and when the attention chain follows (few tokens): rope, KV store and attention in one launch
            // (GGML_MI355X_ATTN_ROPE=0: two launches; tg128 395 -> 403 tok/s)
            if (jk >= 0 && jcv >= 0 && node->ne[2] <= 8 && single_use(node) && sw().attn_rope) {
                int idx[5], kq_n = 0;
                for (int j = std::max(jck, jcv) + 1; j < n_nodes && j <= i + 4 * LOOKAHEAD && kq_n < 5; ++j) {
                    const ggml_tensor * t = cgraph->nodes[j];
                    if (done[j] || t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_TRANSPOSE) continue;
                    if (kq_n == 0 && t->op == GGML_OP_PERMUTE) continue;                   // q's permute in front of kq
                    idx[kq_n++] = j;
                }
                if (kq_n == 5) {
                    ggml_tensor * kqn = cgraph->nodes[idx[0]], * sm = cgraph->nodes[idx[1]], * kqv = cgraph->nodes[idx[2]], * pm = cgraph->nodes[idx[3]],
                                * ct = cgraph->nodes[idx[4]];
                    float scale, max_bias;
                    memcpy(&scale, (const float *) sm->op_params + 0, sizeof(float));
                    memcpy(&max_bias, (const float *) sm->op_params + 1, sizeof(float));
                    if (kqn->op == GGML_OP_MUL_MAT && kqn->src[0]->type == GGML_TYPE_F16 && kqn->src[1]->op == GGML_OP_PERMUTE &&
                        kqn->src[1]->src[0] == node && single_use(kqn) && sm->op == GGML_OP_SOFT_MAX && sm->src[0] == kqn && sm->src[1] &&
                        max_bias == 0.0f && single_use(sm) && kqv->op == GGML_OP_MUL_MAT && kqv->src[1] == sm &&
                        kqv->src[0]->type == GGML_TYPE_F16 && single_use(kqv) && pm->op == GGML_OP_PERMUTE && pm->src[0] == kqv &&
                        pm->ne[0] == kqv->ne[0] && pm->ne[1] == kqv->ne[2] && pm->ne[2] == kqv->ne[1] && ct->op == GGML_OP_CONT && ct->src[0] == pm &&
                        ((early_write_ok(ct, { node->src[1], node->src[2], cgraph->nodes[jk]->src[0], cgraph->nodes[jcv]->src[0],
                                               kqn->src[0], kqv->src[0], sm->src[1] }) &&
                          early_write_ok(ct, { node->src[0] }, node->src[0], true) && early_write_ok(ct, { node }, node, true)) ||
                         hoist_elsewhere(ctx, ct))) {
                        const qmm_tensor kc = to_qt(kqn->src[0], ctx), vc = to_qt(kqv->src[0], ctx), m = to_qt(sm->src[1], ctx), d = to_qt(ct, ctx);
                        const int64_t off = (const char *) kd.data - (const char *) kc.data;
                        const int64_t j0 = kc.nb[1] > 0 && off >= 0 && off % kc.nb[1] == 0 ? off / kc.nb[1] : -1;
                        const bool v_ok = (const char *) vd.data - (const char *) vc.data == j0 * 2;
                        if (j0 >= 0 && v_ok && qmm_attn_decode_rope_supported(&q, &pos, pff, &qd, &k, &kd, &v, &vd, &kc, &vc, &m, &d, j0)) {
                            if (qmm_attn_decode_rope(ctx->dev->qmm, &q, &pos, pff, &qd, &k, &kd, &v, &vd, &kc, &vc, &m, &d, scale, j0,
                                                     qmm_stream(ctx->dev->qmm))) {
                                GGML_LOG_ERROR("MI355X rope + KV store + attention(%s): %s\n", node->name, qmm_last_error());
                                return -1;
                            }
                            if (dbg()) fprintf(stderr, "fused: rope + kv store + attention (%s)\n", node->name);
                            done[jk] = done[jck] = done[jcv] = 1;
                            for (int j = 0; j < 5; ++j) done[idx[j]] = 1;
                            return 1;
                        }
                    }
                }
            }
            if (qmm_rope_kv_store_supported(&q, &pos, pff, &qd, pk, pkd, pv, pvd)) {
                if (qmm_rope_kv_store(ctx->dev->qmm, &q, &pos, pff, &qd, pk, pkd, pv, pvd, qmm_stream(ctx->dev->qmm))) {
                    GGML_LOG_ERROR("MI355X rope + KV store(%s): %s\n", node->name, qmm_last_error());
                    return -1;
                }
                if (jk >= 0) done[jk] = done[jck] = 1;
                if (jcv >= 0) done[jcv] = 1;
                return 1;
            }
        }
    }
    return 0;
}

// RMS_NORM -> MUL(w) (build_norm).  Few tokens, and every reader of the normed row a quantized MUL_MAT of one group (q / k / v, gate / up,
// output): no launch here, fold_norm hands the norm to the mat-vec kernels, or materializes it if the group turns out smaller.
// Otherwise the pair as one launch.  (One site for both, so that the pair is probed once.)
int graph_pass::site_rms_norm_mul(int i, ggml_tensor * node, int gop) {
    (void) gop;
    if (!(i + 1 < n_nodes && node->op == GGML_OP_RMS_NORM && single_use(node))) return 0;
    const ggml_tensor * other = nullptr;
    int fop = fused_pair(node, cgraph->nodes[i + 1], &other);
    if (fop == QMM_OP_RMS_NORM_MUL && node->ne[1] <= QMM_MATVEC_MAX_N && node->ne[2] == 1 && node->ne[3] == 1 && !fuse_off()) {
        const ggml_tensor * mul = cgraph->nodes[i + 1];
        const ggml_tensor * x = node->src[0];
        const reader_group g = scan_reader_group(mul, i + 2, 4);
        const int64_t K = node->ne[0], N = node->ne[1];
        if (g.all && !(mul->flags & GGML_TENSOR_FLAG_OUTPUT) && x->nb[0] == 4 && x->nb[1] % 16 == 0 &&
            (uintptr_t) to_qt(x, ctx).data % 16 == 0 && (uintptr_t) other->data % 16 == 0 && K % 256 == 0 &&
            qmm::mv_fits_norm(N, K)) {
            pending_norm = { node, mul, other, g.n };
            done[i + 1] = 1;
            return 1;
        }
    }
    if (fop && !(early_write_ok(cgraph->nodes[i + 1], { other }) && early_write_ok(cgraph->nodes[i + 1], { node->src[0] }, node->src[0]))) fop = 0;
    if (!fop) return 0;
    ggml_tensor * out = cgraph->nodes[i + 1];
    ggml_tensor tmp = *out;                                              // dst of the pair, carrying the first node's op_params (eps)
    memcpy(tmp.op_params, node->op_params, sizeof(tmp.op_params));
    const enum ggml_status st = compute_glue(ctx, &tmp, fop, node->src[0], other, nullptr);
    done[i + 1] = 1;
    return st == GGML_STATUS_SUCCESS ? 1 : -1;
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
            int r = 0;
            if (deferred[i]) r = P.site_deferred_silu_mul(i, node, gop);
            if (r == 0) r = P.site_hold_silu(i, node, gop);
            if (r == 0) r = P.site_add_rms_norm(i, node, gop);
            if (r == 0) r = P.site_attention(i, node, gop);
            if (r == 0) r = P.site_kqv_into_merged_heads(i, node, gop);
            if (r == 0) r = P.site_moe_combine(i, node, gop);
            if (r == 0) r = P.site_moe_router(i, node, gop);
            if (r == 0) r = P.site_rope_kv_attention(i, node, gop);
            if (r == 0) r = P.site_rms_norm_mul(i, node, gop);
            if (r < 0) return GGML_STATUS_FAILED;
            if (r > 0) continue;
            if (gop == QMM_OP_CPY) {
                st = compute_glue(ctx, node, gop, node->src[0], nullptr, nullptr);
            } else {
                st = compute_glue(ctx, node, gop, node->src[0], node->src[1], node->src[2]);
            }
        } else if (node->op == GGML_OP_MUL_MAT) {
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
// With GGML_MI355X_PREC=q8 (sw().prec_q8) the library's context is in QMM_PREC_Q8_EXACT (qmm_create reads the same switch): Q4_K / Q5_K /
// Q6_K prompts dot integers and cannot overflow, so only a weight type that mode runs as f16 on Q8 activations can bring a graph here;
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
