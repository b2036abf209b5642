// mi355x_sites.cpp — the fusion sites of the graph pass: the matchers (const: they read the graph and the reader analysis and fill a small
// record of node indices), the sites (match, then the aliasing decisions, then one issue step) and the dispatch that offers a node to them.
#include "mi355x_internal.h"

namespace mi355x {

// ----------------------------------------------------------------------------------------------- matchers

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

// The quantized MUL_MATs that read `b` (group_member), looked for among the live nodes from `start` on: n of them, the first `cap` at
// at[]; `all` when they are every reader `b` has in this graph, at least one and at most `cap`.  The scan ends at the first live
// node in front of them that is something else (it reads or runs first: the graph's order stays).  Both hold-back sites pass
// cap = 4, the size of a group.
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

// kq -> soft_max -> kqv -> permute -> cont (build_attn_mha), every intermediate read by the next node only.  `kq` >= 0: the chain
// starts at that node and its other four are the next nodes from `from` on that are no RESHAPE / VIEW / TRANSPOSE (site_attention).
// kq < 0: all five are looked for from `from` on, behind a ROPE: nodes already issued are passed over as well, and so is q's PERMUTE
// in front of kq (site_rope_kv_attention).  Nothing is looked at beyond node `last`.
graph_pass::attn_chain graph_pass::match_attention(int kq, int from, int last) const {
    const bool behind_rope = kq < 0;
    int idx[5] = { kq, -1, -1, -1, -1 }, k = behind_rope ? 0 : 1;
    for (int j = from; j < n_nodes && j <= last && k < 5; ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (t->op == GGML_OP_RESHAPE || t->op == GGML_OP_VIEW || t->op == GGML_OP_TRANSPOSE) continue;
        if (behind_rope && (done[j] || (k == 0 && t->op == GGML_OP_PERMUTE))) continue;
        idx[k++] = j;
    }
    if (k < 5) return {};
    const ggml_tensor * kqn = cgraph->nodes[idx[0]], * sm = cgraph->nodes[idx[1]], * kqv = cgraph->nodes[idx[2]], * pm = cgraph->nodes[idx[3]],
                      * ct = cgraph->nodes[idx[4]];
    const sm_params p = soft_max_params(sm);
    if (!(kqn->op == GGML_OP_MUL_MAT && (kqn->src[0]->type == GGML_TYPE_F16 || kcache_block_type(kqn->src[0]->type)) && single_use(kqn) &&
          sm->op == GGML_OP_SOFT_MAX && sm->src[0] == kqn && sm->src[1] && p.max_bias == 0.0f && single_use(sm) &&
          kqv->op == GGML_OP_MUL_MAT && kqv->src[1] == sm && kqv->src[0]->type == GGML_TYPE_F16 && single_use(kqv) &&
          pm->op == GGML_OP_PERMUTE && pm->src[0] == kqv && pm->ne[0] == kqv->ne[0] && pm->ne[1] == kqv->ne[2] && pm->ne[2] == kqv->ne[1] &&
          ct->op == GGML_OP_CONT && ct->src[0] == pm)) return {};
    return { idx[0], idx[1], idx[2], idx[3], idx[4], p.scale };
}

// ADD -> RMS_NORM -> MUL(w) at nodes ja, ja + 1, ja + 2: the norm read by the MUL only and the pair one launch of the library.  With
// `operand`, the ADD must read it as one of two different operands (the MoE combine's last partial sum).
graph_pass::add_norm graph_pass::match_add_norm(int ja, const ggml_tensor * operand) const {
    if (ja + 2 >= n_nodes) return {};
    const ggml_tensor * add = cgraph->nodes[ja], * rn = cgraph->nodes[ja + 1];
    if (add->op != GGML_OP_ADD || (operand && ((add->src[0] != operand && add->src[1] != operand) || add->src[0] == add->src[1]))) return {};
    const ggml_tensor * w = nullptr;
    if (rn->op != GGML_OP_RMS_NORM || rn->src[0] != add || !single_use(rn) || fused_pair(rn, cgraph->nodes[ja + 2], &w) != QMM_OP_RMS_NORM_MUL) return {};
    return { ja, ja + 1, ja + 2, w };
}

// The MoE router (build_moe_ffn), worked forward from node `entry`: optionally the RMS norm and its MUL whose product is the logits'
// src1 (the MoE branch of the layer, src/llama-model.cpp:4301-4305), optionally the logits' own MUL_MAT (F32 gate_inp, a few tokens),
// then soft_max -> argsort (top_k view) -> get_rows -> sum_rows -> div.  llama.cpp's graph order puts get_rows / sum_rows / div (the
// weights, needed only by the final mul) BEHIND the expert MUL_MAT_IDs: the argsort follows the soft_max directly, the other three
// are looked for further down; the live nodes passed over on the way go to `skipped` (the site answers for running the three early).
graph_pass::router_match graph_pass::match_router(int entry, std::vector<const ggml_tensor *> & skipped) const {
    router_match r;
    if (fuse_off()) return r;
    int at = entry;                                                          // the node the next stage looks at
    const ggml_tensor * e = cgraph->nodes[entry];
    if (e->op == GGML_OP_RMS_NORM && entry + 2 < n_nodes && e->ne[1] <= 8 && e->ne[2] == 1 && e->ne[3] == 1 && single_use(e) &&
        !sw().router_norm_off && !sw().router_logits_off) {
        const ggml_tensor * m = cgraph->nodes[entry + 1];
        const int jl = next_live(entry + 2);                                 // (the 3-D reshape of the normed row for the expert MUL_MAT_IDs sits in between)
        if (jl >= n_nodes || done[entry + 1] || fused_pair(e, m, &r.nwgt) != QMM_OP_RMS_NORM_MUL) return r;
        const ggml_tensor * t = cgraph->nodes[jl];
        if (t->op != GGML_OP_MUL_MAT || t->src[1] != m || t->src[0]->type != GGML_TYPE_F32 || (m->flags & GGML_TENSOR_FLAG_OUTPUT)) return r;
        r.nrm = entry;  r.nmul = entry + 1;  at = jl;
    }
    const ggml_tensor * l = cgraph->nodes[at];
    if (l->op == GGML_OP_MUL_MAT && l->src[0]->type == GGML_TYPE_F32 && l->src[1]->type == GGML_TYPE_F32 && l->type == GGML_TYPE_F32 && l->ne[0] <= 64 &&
        l->ne[1] <= 8 && l->ne[2] == 1 && l->ne[3] == 1 && !sw().router_logits_off) {
        const int js = next_live(at + 1);
        if (js >= n_nodes || cgraph->nodes[js]->op != GGML_OP_SOFT_MAX || cgraph->nodes[js]->src[0] != l) return r;
        r.lgt = at;  at = js;
    } else if (r.nrm >= 0) {
        if (dbg()) fprintf(stderr, "fusion declined: moe router with its norm (%s): not the logits' MUL_MAT\n", cgraph->nodes[r.nmul]->name);
        return r;
    }
    const ggml_tensor * sm = cgraph->nodes[at];
    if (!(sm->op == GGML_OP_SOFT_MAX && !sm->src[1] && sm->ne[0] <= 64 && sm->ne[2] == 1 && sm->ne[3] == 1)) return r;
    int idx[4], k = 0;
    skipped.clear();
    for (int j = at + 1; j < n_nodes && j <= at + 64 && k < 4; ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (done[j] || is_noop(t)) continue;
        const bool want = (k == 0 && t->op == GGML_OP_ARGSORT && t->src[0] == sm) ||
                          (k == 1 && t->op == GGML_OP_GET_ROWS && root_of(t->src[0]) == sm && root_of(t->src[1]) == cgraph->nodes[idx[0]]) ||
                          (k == 2 && t->op == GGML_OP_SUM_ROWS && root_of(t->src[0]) == cgraph->nodes[idx[1]]) ||
                          (k == 3 && t->op == GGML_OP_DIV && root_of(t->src[0]) == cgraph->nodes[idx[1]] && t->src[1] == cgraph->nodes[idx[2]]);
        if (want) idx[k++] = j;
        else if (k == 0) break;                                             // the argsort must come first
        else skipped.push_back(t);
    }
    const sm_params p = soft_max_params(sm);
    if (k < 4 || p.scale != 1.0f || p.max_bias != 0.0f) return r;
    const ggml_tensor * as = cgraph->nodes[idx[0]], * gr = cgraph->nodes[idx[1]], * sr = cgraph->nodes[idx[2]], * dv = cgraph->nodes[idx[3]];
    const auto * ri = info(sm), * rg = info(gr), * rs = info(sr);
    if (!(as->op_params[0] == GGML_SORT_ORDER_DESC && gr->src[0]->ne[0] == 1 &&
          gr->src[1]->data == as->data && gr->src[1]->nb[1] == as->nb[1] && gr->src[1]->ne[1] == as->ne[1] &&
          ri && ri->uses == 2 && rg && rg->uses == 2 && rs && rs->uses == 1 && ggml_is_contiguous(dv) && ggml_is_contiguous(gr) &&
          !(sm->flags & GGML_TENSOR_FLAG_OUTPUT) && !(gr->flags & GGML_TENSOR_FLAG_OUTPUT) && !(sr->flags & GGML_TENSOR_FLAG_OUTPUT))) return r;
    r.sm = at;  r.argsort = idx[0];  r.get_rows = idx[1];  r.sum_rows = idx[2];  r.div = idx[3];
    r.n_used = gr->src[1]->ne[0];
    r.form = r.nrm >= 0 ? ROUTER_LOGITS_NORM : r.lgt >= 0 ? ROUTER_LOGITS : ROUTER;
    return r;
}

// experts * weights at MUL node i and the sum over the U used experts through 2-D views (build_moe_ffn's tail): the U - 1 ADDs behind it
graph_pass::combine_match graph_pass::match_moe_combine(int i) const {
    const ggml_tensor * node = cgraph->nodes[i];
    if (!(node->src[1]->ne[0] == 1 && node->ne[1] >= 2 && node->ne[1] <= 64 && node->ne[1] == node->src[1]->ne[1] && node->ne[3] == 1 && !fuse_off())) return {};
    combine_match c;
    const int U = (int) node->ne[1];
    const auto * rm = info(node);
    int k = 0;
    for (int j = i + 1; j < n_nodes && j <= i + 4 * U + 4 && k < U - 1; ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (done[j] || is_noop(t)) continue;
        if (t->op != GGML_OP_ADD) break;
        c.adds[k++] = j;
    }
    const auto is_slice = [&](const ggml_tensor * v, int u) {               // view_2d(experts, E, N, nb[2], u * nb[1])
        return root_of(v) == node && v->ne[0] == node->ne[0] && v->ne[1] == node->ne[2] && v->ne[2] == 1 && v->nb[1] == node->nb[2] &&
               (const char *) v->data == (const char *) node->data + (size_t) u * node->nb[1];
    };
    bool ok = k == U - 1 && rm && rm->uses == U && !(node->flags & GGML_TENSOR_FLAG_OUTPUT);
    for (int a = 0; ok && a < U - 1; ++a) {
        const ggml_tensor * ad = cgraph->nodes[c.adds[a]];
        ok = is_slice(ad->src[1], a + 1) && (a == 0 ? is_slice(ad->src[0], 0) : ad->src[0] == cgraph->nodes[c.adds[a - 1]]) &&
             (a == U - 2 || (single_use(ad) && !(ad->flags & GGML_TENSOR_FLAG_OUTPUT)));
    }
    if (ok) c.U = U;
    return c;
}

// Behind ROPE node i (rope(q)), among the live nodes in front of the attention: rope(k) with the same positions and parameters and its
// store into the K cache, and v's store into the V cache (build_attn's two ggml_cpy).  Their inputs must exist already (k and v were
// hoisted into the q/k/v group); rope(k) without its store stays where it is.  A contiguous K store pairs with rope(k) when it is F16, or in a
// block type of a quantized K cache (-ctk q8_0 / q4_0 / q4_1 / q5_0 / q5_1: kcache_block_type) and the kernel library has qmm_rope_kq_store
// (an older library, or the stub, has not: rope(k) and its CPY f32 -> block type then run as their own nodes).  The one-launch rope + store
// + attention stays F16 only: on a quantized cache the site never tries it, and the attention chain is taken at its kq (site_attention).
graph_pass::rope_kv_match graph_pass::match_rope_kv(int i) const {
    const ggml_tensor * node = cgraph->nodes[i];
    auto ready = [&](const ggml_tensor * t) {                                // was t's root produced before this point?
        for (int j = i + 1; j < n_nodes && j <= i + 2 * LOOKAHEAD; ++j)
            if (cgraph->nodes[j] == root_of(t)) return done[j] != 0;
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
        } else if (jk >= 0 && jck < 0 && t->op == GGML_OP_CPY && t->src[0] == cgraph->nodes[jk] && ggml_is_contiguous(t) &&
                   (t->type == GGML_TYPE_F16 || (kcache_block_type(t->type) && qmm_rope_kq_store_supported && qmm_rope_kq_store))) {
            jck = j;
        } else if (jcv < 0 && t->op == GGML_OP_CPY && t->type == GGML_TYPE_F16 && t->src[0]->type == GGML_TYPE_F32 &&
                   root_of(t->src[0])->op == GGML_OP_MUL_MAT && ready(t->src[0]) && (jk < 0 || t->src[0] != cgraph->nodes[jk])) {
            jcv = j;
        } else if (t->op == GGML_OP_MUL_MAT || t->op == GGML_OP_SOFT_MAX || t->op == GGML_OP_FLASH_ATTN_EXT) {
            break;                                                         // attention starts: nothing to find beyond
        }
    }
    if (jck < 0) jk = -1;
    return { jk, jck, jcv };
}

// ----------------------------------------------------------------------------------------------- sites

// a MUL whose operand is a SILU that was held back (site_hold_silu): silu(gate) * up in one pass, or folded into the staging of the MUL_MAT behind it
int graph_pass::site_deferred_silu_mul(int i) {
    const ggml_tensor * node = cgraph->nodes[i], * silu = deferred[i];
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
    return compute_glue(ctx, node, QMM_OP_SILU_MUL, gate, up, nullptr) == GGML_STATUS_SUCCESS ? 1 : -1;
}

// SILU read by one MUL further down (build_ffn: gate, silu, up, mul): held back for that MUL when nothing in between writes over its input
int graph_pass::site_hold_silu(int i) {
    const ggml_tensor * node = cgraph->nodes[i], * other = nullptr;
    if (!single_use(node)) return 0;
    int j = i + 1;
    bool safe = true;
    for (; j < n_nodes && j <= i + LOOKAHEAD; ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (t->src[0] == node || t->src[1] == node) break;
        if (!done[j] && !is_noop(t) && ranges_overlap(t, node->src[0])) safe = false;
    }
    if (!(safe && j < n_nodes && j <= i + LOOKAHEAD && fused_pair(node, cgraph->nodes[j], &other) == QMM_OP_SILU_MUL)) return 0;
    deferred[j] = node;
    return 1;
}

graph_pass::add_norm_operands graph_pass::marshal_add_norm(const ggml_tensor * add, const ggml_tensor * mul, const ggml_tensor * w) const {
    return { to_qt(add->src[0], ctx), to_qt(add->src[1], ctx), to_qt(w, ctx), to_qt(add, ctx), to_qt(mul, ctx) };
}
enum ggml_status graph_pass::launch_add_rms_norm(const add_norm_operands & o, const ggml_tensor * add, const ggml_tensor * rn) {
    qmm_ctx * q = ctx->dev->qmm;
    return launched(qmm_op_add_rms_norm(q, &o.a, &o.b, &o.w, &o.sum, &o.d, rms_eps(rn), qmm_stream(q)), "MI355X ADD+RMS_NORM(%s): %s\n", add->name);
}

// residual ADD -> RMS_NORM -> MUL(w): one launch with two results, or (a prompt batch) none: held back for the MUL_MATs behind it
int graph_pass::site_add_rms_norm(int i) {
    if (fuse_off()) return 0;
    const add_norm m = match_add_norm(i, nullptr);
    if (m.add < 0) return 0;
    ggml_tensor * node = cgraph->nodes[i], * rn = cgraph->nodes[m.rn], * mul = cgraph->nodes[m.mul];
    const ggml_tensor * x0 = node->src[0], * x1 = node->src[1];
    const add_norm_operands o = marshal_add_norm(node, mul, m.w);
    // A prompt batch whose normed rows are read by ONE group of quantized MUL_MATs right behind the MUL (q / k / v, gate / up) and by
    // nothing else: no launch here; the group's activation prep adds, norms and stores the sum (fold_norm; round 3)
    if (node->ne[1] > QMM_MATVEC_MAX_N && node->ne[2] == 1 && node->ne[3] == 1 && ggml_are_same_shape(x0, x1) && ggml_are_same_shape(node, x0) &&
        !sw().prep_norm_off) {
        const reader_group g = scan_reader_group(mul, i + 3, 4);
        qmm_weight gw[4];
        for (int k = 0; k < g.n; ++k) {
            const ggml_tensor * w = cgraph->nodes[g.at[k]]->src[0];
            gw[k] = qmm_weight{ w->data, (int64_t) w->nb[1], w->ne[1], nullptr, 0, weight_type(ctx, w) };
        }
        if (g.all && !(mul->flags & GGML_TENSOR_FLAG_OUTPUT) && !(node->flags & GGML_TENSOR_FLAG_OUTPUT) &&
            x0->type == GGML_TYPE_F32 && x1->type == GGML_TYPE_F32 && x0->nb[0] == 4 && x1->nb[0] == 4 && node->nb[0] == 4 &&
            x0->nb[1] % 16 == 0 && x1->nb[1] % 16 == 0 && node->nb[1] % 16 == 0 && (uintptr_t) o.a.data % 16 == 0 && (uintptr_t) o.b.data % 16 == 0 &&
            (uintptr_t) o.sum.data % 16 == 0 && (uintptr_t) m.w->data % 16 == 0 &&
            // the sum is stored while other rows of the operands are still read: in place over an operand only with the same rows
            early_write_ok(node, { x0 }, x0) && early_write_ok(node, { x1 }, x1) && early_write_ok(node, { m.w }) &&
            qmm_mul_mat_group_norm_supported(ctx->dev->qmm, gw, g.n, node->ne[0], node->ne[1])) {
            pending_norm = { rn, mul, m.w, g.n, node };
            done[m.rn] = done[m.mul] = 1;
            if (dbg()) fprintf(stderr, "held back: add + norm (%s, %s) for the prep of %d MUL_MATs\n", node->name, mul->name, g.n);
            return 1;
        }
    }
    // `mul`'s buffer is written two nodes early: it may be the block of an ADD operand that dies here (same rows: fine, a
    // workgroup holds its row in registers before it stores; anything else: keep the graph's order)
    const bool e_ok = early_write_ok(mul, { x0, x1, m.w, node }, nullptr) ||
                      (early_write_ok(mul, { x1, m.w, node }, nullptr) && early_write_ok(mul, { x0 }, x0)) ||
                      (early_write_ok(mul, { x0, m.w, node }, nullptr) && early_write_ok(mul, { x1 }, x1));
    if (!e_ok || !qmm_op_add_rms_norm_supported(&o.a, &o.b, &o.w, &o.sum, &o.d)) return 0;
    if (launch_add_rms_norm(o, node, rn) != GGML_STATUS_SUCCESS) return -1;
    done[m.rn] = done[m.mul] = 1;
    return 1;
}

// RMS_NORM -> MUL(w) (build_norm).  Few tokens, and every reader of the normed row a quantized MUL_MAT of one group (q / k / v, gate / up,
// output): no launch here, fold_norm hands the norm to the mat-vec kernels, or materializes it if the group turns out smaller.
// Otherwise the pair as one launch.  (One site for both, so that the pair is probed once.)
int graph_pass::site_rms_norm_mul(int i) {
    ggml_tensor * node = cgraph->nodes[i];
    if (!(i + 1 < n_nodes && single_use(node))) return 0;
    ggml_tensor * mul = cgraph->nodes[i + 1];
    const ggml_tensor * other = nullptr, * x = node->src[0];
    const int fop = fused_pair(node, mul, &other);
    if (fop == QMM_OP_RMS_NORM_MUL && node->ne[1] <= QMM_MATVEC_MAX_N && node->ne[2] == 1 && node->ne[3] == 1 && !fuse_off()) {
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
    if (!fop || !(early_write_ok(mul, { other }) && early_write_ok(mul, { x }, x))) return 0;
    ggml_tensor tmp = *mul;                                              // dst of the pair, carrying the first node's op_params (eps)
    memcpy(tmp.op_params, node->op_params, sizeof(tmp.op_params));
    const enum ggml_status st = compute_glue(ctx, &tmp, fop, x, other, nullptr);
    done[i + 1] = 1;
    return st == GGML_STATUS_SUCCESS ? 1 : -1;
}

// kq -> soft_max -> kqv -> permute -> cont (build_attn_mha): one launch, for a few tokens (qmm_attn_decode) and for prompt batches
// whose scores fit LDS (qmm_attn_prefill)
int graph_pass::site_attention(int i) {
    if (fuse_off()) return 0;
    const attn_chain c = match_attention(i, i + 1, i + 8);
    if (c.kq < 0) return 0;
    const ggml_tensor * kq = cgraph->nodes[c.kq], * ct = cgraph->nodes[c.ct];
    const ggml_tensor * q = kq->src[1], * k = kq->src[0], * v = cgraph->nodes[c.kqv]->src[0], * mask = cgraph->nodes[c.sm]->src[1];
    // ggml-alloc puts ct across the dead Q blocks in llama.cpp's layers: written to the scratch instead, wo reads it there
    if (!((early_write_ok(ct, { k, v, mask }) && early_write_ok(ct, { q }, q, true)) || hoist_elsewhere(ctx, ct))) return 0;
    const int r = issue_attention(ctx, to_qt(q, ctx), to_qt(k, ctx), to_qt(v, ctx), to_qt(mask, ctx), to_qt(ct, ctx), c.scale, "attention", kq->name, true);
    if (r <= 0) return r;
    if (dbg()) fprintf(stderr, "fused: attention (%s, %s)\n", r == ATTN_DECODE ? "few tokens" : "prompt", kq->name);
    for (int j : { c.sm, c.kqv, c.pm, c.ct }) done[j] = 1;
    return 1;
}

// kqv -> permute(0, 2, 1, 3) -> cont (build_attn_mha's head merge) at any batch size: the product is written straight into the
// cont's layout (dst strides of dims 1 and 2 swapped), the copy never runs
int graph_pass::site_kqv_into_merged_heads(int i) {
    const ggml_tensor * node = cgraph->nodes[i];
    if (!single_use(node) || fuse_off()) return 0;
    int jp = i + 1;
    while (jp < n_nodes && (cgraph->nodes[jp]->op == GGML_OP_RESHAPE || cgraph->nodes[jp]->op == GGML_OP_VIEW)) ++jp;
    int jc = jp + 1;
    while (jc < n_nodes && (cgraph->nodes[jc]->op == GGML_OP_RESHAPE || cgraph->nodes[jc]->op == GGML_OP_VIEW)) ++jc;
    if (jc >= n_nodes) return 0;
    const ggml_tensor * pm = cgraph->nodes[jp], * ct = cgraph->nodes[jc];
    if (!(pm->op == GGML_OP_PERMUTE && pm->src[0] == node && ct->op == GGML_OP_CONT && ct->src[0] == pm && !done[jc] &&
          pm->ne[0] == node->ne[0] && pm->ne[1] == node->ne[2] && pm->ne[2] == node->ne[1] && node->ne[3] == 1 &&
          ct->type == GGML_TYPE_F32 && ggml_is_contiguous(ct) && ggml_nelements(ct) == ggml_nelements(node) &&
          early_write_ok(ct, { node->src[0], node->src[1] }))) return 0;
    qmm_tensor d = to_qt(node, ctx);
    d.data = to_qt(ct, ctx).data;                                 // element (d, n, h) of kqv = element (d, h, n) of the merged result (ct may live in the scratch)
    d.nb[1] = (int64_t) node->ne[0] * node->ne[2] * 4;
    d.nb[2] = (int64_t) node->ne[0] * 4;
    d.nb[3] = (int64_t) ggml_nbytes(ct);
    const qmm_tensor a = to_qt(node->src[0], ctx), b = to_qt(node->src[1], ctx);
    if (!qmm_op_supported(QMM_OP_MUL_MAT_F, &a, &b, nullptr, &d)) return 0;
    if (launched(op_compute(ctx, QMM_OP_MUL_MAT_F, &a, &b, nullptr, &d), "MI355X MUL_MAT(%s) into merged heads: %s\n", node->name) != GGML_STATUS_SUCCESS) return -1;
    done[jc] = 1;
    return 1;
}

// experts * weights and the sum over the used experts (build_moe_ffn's tail): one launch, with the residual add, the RMS norm and the
// norm weight that follow the block in the layer where they are there
int graph_pass::site_moe_combine(int i) {
    const combine_match c = match_moe_combine(i);
    if (!c.U) return 0;
    const ggml_tensor * node = cgraph->nodes[i], * last = cgraph->nodes[c.adds[c.U - 2]];
    const ggml_tensor * ex = node->src[0], * wt = node->src[1];
    qmm_ctx * q = ctx->dev->qmm;
    // Round 3: ffn_moe_out + ffn_inp -> l_out, then the next attn_norm / result_norm in the same launch: the next three live nodes must
    // be exactly ADD(last, r), RMS_NORM(add), MUL(rms, w).  Never written then: the product, the partial sums, the block's output and the
    // un-weighted norm: each has exactly the readers of the pattern (closed readers: analyze_readers).  Written HERE, U + 2 nodes early,
    // while other workgroups (one per token) still read the expert rows, the weights and the residual: l_out and the normed row
    // must be clear of the experts and the weights (another layout) and may sit on the residual only as the very same rows.
    add_norm t;
    if (!sw().moe_combine_norm_off && single_use(last) && !(last->flags & GGML_TENSOR_FLAG_OUTPUT)) t = match_add_norm(next_live(c.adds[c.U - 2] + 1), last);
    int rc = 0;
    bool issued = false;
    if (t.add >= 0) {
        const ggml_tensor * add = cgraph->nodes[t.add], * mul = cgraph->nodes[t.mul];
        const ggml_tensor * r = add->src[0] == last ? add->src[1] : add->src[0];
        const auto clear_of = [&](const ggml_tensor * d) {
            return early_write_ok(d, { ex, wt, t.w }) && (early_write_ok(d, { r }) || early_write_ok(d, { r }, r));
        };
        // one token = one workgroup, which holds all its inputs in registers before it stores (moe_combine_add_norm_kernel): the
        // results may then lie on any input (ggml-alloc does put l_out on the dead router weights and the normed row on the residual)
        const bool one = add->ne[1] == 1 && add->ne[2] == 1 && add->ne[3] == 1;
        if ((one || (clear_of(add) && clear_of(mul))) && !ranges_overlap(add, mul)) {
            const qmm_tensor x = to_qt(ex, ctx), w = to_qt(wt, ctx), qb = to_qt(r, ctx), nw = to_qt(t.w, ctx), qs = to_qt(add, ctx), qd = to_qt(mul, ctx);
            if (qmm_moe_combine_add_rms_norm_supported(&x, &w, &qb, &nw, &qs, &qd)) {
                rc = qmm_moe_combine_add_rms_norm(q, &x, &w, &qb, &nw, &qs, &qd, rms_eps(cgraph->nodes[t.rn]), qmm_stream(q));
                issued = true;
            }
        }
    }
    if (!issued) {
        t = {};
        // the launch writes the LAST add's buffer at the MUL's position, while other workgroups still read the experts and the
        // weights: ggml-alloc may have put it on either (both are dead at the add's place in the graph).  A token's U expert
        // rows and its one output row are laid out differently, so not even the same address is in place
        if (!early_write_ok(last, { ex, wt }) && !hoist_elsewhere(ctx, last)) return 0;
        const qmm_tensor x = to_qt(ex, ctx), w = to_qt(wt, ctx), o = to_qt(last, ctx);
        if (!qmm_moe_combine_supported(&x, &w, &o)) return 0;
        rc = qmm_moe_combine(q, &x, &w, &o, qmm_stream(q));
    }
    if (launched(rc, "MI355X %s(%s): %s\n", t.add >= 0 ? "MoE combine + ADD + RMS_NORM" : "MoE combine", node->name) != GGML_STATUS_SUCCESS) return -1;
    if (t.add >= 0 && dbg()) fprintf(stderr, "fused: moe combine + add + rms_norm (%s)\n", cgraph->nodes[t.add]->name);
    for (int a = 0; a < c.U - 1; ++a) done[c.adds[a]] = 1;
    for (int j : { t.add, t.rn, t.mul }) if (j >= 0) done[j] = 1;
    return 1;
}

// The issue step of the router, one for its three forms: ROUTER enters the library behind the logits, ROUTER_LOGITS computes them too
// (they land in their own buffer at their own place in the graph, so nothing about them changes for any other reader),
// ROUTER_LOGITS_NORM also forms the normed row and stores it for the expert MUL_MAT_IDs (the separate norm launch, 4.75 us of a
// Mixtral layer's ~84, is gone).  0: the library declines the operands.
int graph_pass::issue_router(int entry, const router_match & r) {
    const ggml_tensor * sm = cgraph->nodes[r.sm], * lgt = r.lgt >= 0 ? cgraph->nodes[r.lgt] : nullptr, * nrm = r.nrm >= 0 ? cgraph->nodes[r.nrm] : nullptr,
                      * nmul = nrm ? cgraph->nodes[r.nmul] : nullptr;
    qmm_ctx * q = ctx->dev->qmm;
    const qmm_tensor lg = to_qt(sm->src[0], ctx), ids = to_qt(cgraph->nodes[r.argsort], ctx), w = to_qt(cgraph->nodes[r.div], ctx);
    qmm_tensor gi{}, xin{}, nw{}, ny{};
    if (lgt) { gi = to_qt(lgt->src[0], ctx);  xin = to_qt(nrm ? nrm->src[0] : lgt->src[1], ctx); }
    if (nrm) { nw = to_qt(r.nwgt, ctx);  ny = to_qt(nmul, ctx); }
    const bool ok = (!lgt || (is_ours(lgt->src[0]) && !is_split(lgt->src[0]))) &&
                    (r.form == ROUTER_LOGITS_NORM ? qmm_moe_router_logits_norm_supported(&gi, &xin, &nw, &ny, &lg, &ids, &w, r.n_used) :
                     r.form == ROUTER_LOGITS      ? qmm_moe_router_logits_supported(&gi, &xin, &lg, &ids, &w, r.n_used) :
                                                    qmm_moe_router_supported(&lg, &ids, &w, r.n_used)) != 0;
    if (!ok) {
        if (nrm && dbg()) fprintf(stderr, "fusion declined: moe router with its norm (%s): operands not supported\n", nmul->name);
        return 0;
    }
    const int rc = r.form == ROUTER_LOGITS_NORM ? qmm_moe_router_logits_norm(q, &gi, &xin, &nw, rms_eps(nrm), &ny, &lg, &ids, &w, r.n_used, 1, qmm_stream(q)) :
                   r.form == ROUTER_LOGITS      ? qmm_moe_router_logits(q, &gi, &xin, &lg, &ids, &w, r.n_used, 1, qmm_stream(q)) :
                                                  qmm_moe_router(q, &lg, &ids, &w, r.n_used, 1, qmm_stream(q));
    static const char * const what[] = { "", "MoE router", "MoE router with logits", "MoE router with norm and logits" };
    if (launched(rc, "MI355X %s(%s): %s\n", what[r.form], sm->name) != GGML_STATUS_SUCCESS) return -1;
    if (dbg()) {
        fprintf(stderr, "fused: moe router (%s)", sm->name);
        if (lgt) fprintf(stderr, " with its logits (%s)", lgt->name);
        if (nrm) fprintf(stderr, " and their norm (%s)", nmul->name);
        fputc('\n', stderr);
    }
    for (int j : { r.nmul, r.lgt, r.sm, r.argsort, r.get_rows, r.sum_rows, r.div }) if (j > entry) done[j] = 1;      // (node `entry` is the caller's)
    return 1;
}

// the MoE router as one launch, entered at the soft_max, at the logits' MUL_MAT or at the RMS norm in front of it (match_router)
int graph_pass::site_moe_router(int i) {
    std::vector<const ggml_tensor *> & skipped = ctx->skipped;
    const router_match r = match_router(i, skipped);
    if (r.form == ROUTER_NONE) return 0;
    const ggml_tensor * sm = cgraph->nodes[r.sm], * as = cgraph->nodes[r.argsort], * dv = cgraph->nodes[r.div];
    const ggml_tensor * lgt = r.lgt >= 0 ? cgraph->nodes[r.lgt] : nullptr, * gi = lgt ? lgt->src[0] : nullptr, * x1 = lgt ? lgt->src[1] : nullptr;
    // the ids are written while other waves (one per token) still read logits rows: in place only at the very same address
    // with the same rows (a wave reads its row first).  With the logits computed here, the ids and the weights are also written
    // beside the reads of the MUL_MAT's operands, which they must stay clear of.  The weights are written now, not at the div's place
    // in the graph: their block must be free here AND clear of the logits: at the div's place the logits are dead, so a non-inplace
    // dv may sit on them with rows of 4 * n_used bytes against 4 * n_expert; otherwise into the scratch
    if (!early_write_ok(as, { sm->src[0], x1, gi }, sm->src[0])) return 0;
    if (!(can_hoist(dv, skipped) && early_write_ok(dv, { sm->src[0], as, x1, gi })) && !hoist_elsewhere(ctx, dv)) return 0;
    if (r.form == ROUTER_LOGITS_NORM) {
        // the normed row is written where the MUL would put it, two nodes early and beside this launch's reads of the un-normed
        // rows (in place over them is fine: a workgroup holds its row in registers before it stores) and of the weights; the
        // router's outputs stay clear of all of them
        const ggml_tensor * nmul = cgraph->nodes[r.nmul], * x0 = cgraph->nodes[r.nrm]->src[0];
        if (!(early_write_ok(nmul, { r.nwgt, gi }) && early_write_ok(nmul, { x0 }, x0))) return 0;
        if (!early_write_ok(lgt, { x0, r.nwgt, nmul, gi }) || !early_write_ok(as, { x0, r.nwgt, nmul }) ||
            (to_qt(dv, ctx).data == dv->data && !early_write_ok(dv, { x0, r.nwgt, nmul }))) return 0;
    }
    return issue_router(i, r);
}

// rope(q) with, from further down the graph, rope(k) -> K cache and v -> V cache: one launch (any batch size: at 512 tokens 29 us of
// four launches become one, pp512 31.2k -> 32.0k); the cache is not compute-buffer memory, so storing early cannot collide with
// anything in between.  And when the attention chain follows (few tokens): rope, KV store and attention in one launch
// (GGML_MI355X_ATTN_ROPE=0: two launches; tg128 395 -> 403 tok/s)
int graph_pass::site_rope_kv_attention(int i) {
    if (fuse_off()) return 0;
    const rope_kv_match s = match_rope_kv(i);
    if (s.rk < 0 && s.cv < 0) return 0;
    const ggml_tensor * node = cgraph->nodes[i];
    qmm_ctx * qc = ctx->dev->qmm;
    const qmm_tensor q = to_qt(node->src[0], ctx), pos = to_qt(node->src[1], ctx), qd = to_qt(node, ctx);
    qmm_tensor ff{}, k{}, kd{}, v{}, vd{};
    if (node->src[2]) ff = to_qt(node->src[2], ctx);
    bool kq = false;                                                   // the K store goes into blocks of a quantized cache
    if (s.rk >= 0) {
        const ggml_tensor * rk = cgraph->nodes[s.rk], * ck = cgraph->nodes[s.ck];
        kq = kcache_block_type(ck->type);
        k = to_qt(rk->src[0], ctx);
        kd = to_qt(rk, ctx);                                           // shape of rope(k), bytes of the cache view
        kd.data = ck->data;
        kd.type = ck->type;
        if (kq) {                                                      // rows of whole blocks in the type's strides (rope(k)->ne[0] is a multiple of the block, or the library declines)
            kd.nb[0] = (int64_t) ggml_type_size(ck->type);
            kd.nb[1] = (int64_t) ggml_row_size(ck->type, kd.ne[0]);
            for (int a = 2; a < 4; ++a) kd.nb[a] = kd.nb[a - 1] * kd.ne[a - 1];
        } else {
            kd.nb[0] = 2;
            for (int a = 1; a < 4; ++a) kd.nb[a] = kd.nb[a - 1] * kd.ne[a - 1];
        }
    }
    if (s.cv >= 0) {
        v = to_qt(cgraph->nodes[s.cv]->src[0], ctx);
        vd = to_qt(cgraph->nodes[s.cv], ctx);
    }
    const qmm_tensor * pff = node->src[2] ? &ff : nullptr, * pk = s.rk >= 0 ? &k : nullptr, * pkd = s.rk >= 0 ? &kd : nullptr,
                     * pv = s.cv >= 0 ? &v : nullptr, * pvd = s.cv >= 0 ? &vd : nullptr;
    if (kq) {
        // one launch for rope(q), rope(k) into the cache's blocks and the V store; the cache is stored early as on F16.  Declined: the K
        // pair is dropped, rope(k) and its CPY stay their own nodes, and the launch below is rope(q) + the V store as before
        if (kd.ne[0] % ggml_blck_size((enum ggml_type) kd.type) == 0 && qmm_rope_kq_store_supported(&q, &pos, pff, &qd, pk, pkd, pv, pvd)) {
            const int rc = qmm_rope_kq_store(qc, &q, &pos, pff, &qd, pk, pkd, pv, pvd, qmm_stream(qc));
            if (launched(rc, "MI355X rope + quantized K store(%s): %s\n", node->name) != GGML_STATUS_SUCCESS) return -1;
            if (dbg()) fprintf(stderr, "fused: rope + quantized k store (%s, %s)\n", cgraph->nodes[s.rk]->name, ggml_type_name(cgraph->nodes[s.ck]->type));
            for (int j : { s.rk, s.ck, s.cv }) if (j >= 0) done[j] = 1;
            return 1;
        }
        if (s.cv < 0) return 0;
        pk = pkd = nullptr;
    }
    const bool k_pair = pk != nullptr;
    attn_chain c;                                                          // stays empty unless the attention goes into the launch
    qmm_tensor kc{}, vc{}, m{}, d{};
    int64_t j0 = -1;
    if (k_pair && s.cv >= 0 && node->ne[2] <= 8 && single_use(node) && sw().attn_rope) {
        c = match_attention(-1, std::max(s.ck, s.cv) + 1, i + 4 * LOOKAHEAD);
        bool ok = false;
        if (c.kq >= 0) {
            const ggml_tensor * kqn = cgraph->nodes[c.kq], * kqv = cgraph->nodes[c.kqv], * sm = cgraph->nodes[c.sm], * ct = cgraph->nodes[c.ct];
            ok = kqn->src[1]->op == GGML_OP_PERMUTE && kqn->src[1]->src[0] == node &&
                 ((early_write_ok(ct, { node->src[1], node->src[2], cgraph->nodes[s.rk]->src[0], cgraph->nodes[s.cv]->src[0], kqn->src[0], kqv->src[0], sm->src[1] }) &&
                   early_write_ok(ct, { node->src[0] }, node->src[0], true) && early_write_ok(ct, { node }, node, true)) ||
                  hoist_elsewhere(ctx, ct));
            if (ok) {
                kc = to_qt(kqn->src[0], ctx);  vc = to_qt(kqv->src[0], ctx);  m = to_qt(sm->src[1], ctx);  d = to_qt(ct, ctx);
                const int64_t off = (const char *) kd.data - (const char *) kc.data;
                j0 = kc.nb[1] > 0 && off >= 0 && off % kc.nb[1] == 0 ? off / kc.nb[1] : -1;
                const bool v_ok = (const char *) vd.data - (const char *) vc.data == j0 * 2;
                ok = j0 >= 0 && v_ok && qmm_attn_decode_rope_supported(&q, &pos, pff, &qd, &k, &kd, &v, &vd, &kc, &vc, &m, &d, j0);
            }
        }
        if (!ok) c = {};
    }
    if (c.kq < 0 && !qmm_rope_kv_store_supported(&q, &pos, pff, &qd, pk, pkd, pv, pvd)) return 0;
    const int rc = c.kq >= 0 ? qmm_attn_decode_rope(qc, &q, &pos, pff, &qd, &k, &kd, &v, &vd, &kc, &vc, &m, &d, c.scale, j0, qmm_stream(qc))
                             : qmm_rope_kv_store(qc, &q, &pos, pff, &qd, pk, pkd, pv, pvd, qmm_stream(qc));
    if (launched(rc, "MI355X %s(%s): %s\n", c.kq >= 0 ? "rope + KV store + attention" : "rope + KV store", node->name) != GGML_STATUS_SUCCESS) return -1;
    if (c.kq >= 0 && dbg()) fprintf(stderr, "fused: rope + kv store + attention (%s)\n", node->name);
    for (int j : { k_pair ? s.rk : -1, k_pair ? s.ck : -1, s.cv, c.kq, c.sm, c.kqv, c.pm, c.ct }) if (j >= 0) done[j] = 1;
    return 1;
}

// ----------------------------------------------------------------------------------------------- dispatch

// Glue node i, library op `gop`, is offered to the sites that can start at a node of its kind; the first that takes it wins.  1: issued
// (or held back), possibly together with later nodes marked in done[]; 0: no site took it, the caller issues the node alone; -1: a
// launch failed.  Where two sites start at the same kind of node their order matters:
//   MUL       a MUL that site_hold_silu claimed carries the SILU nobody has run: it is always finished as silu * up, never
//             looked at as the head of a MoE combine.
//   MUL_MAT   (F16 src0, or a view of a K cache in a block type (kcache_block_type), which graph_compute offers although it is no glue op and which can only be a kq)
//             the attention takes the whole chain from kq; only a kqv that no attention launch took (the chain was declined
//             when its kq came by) is left for the merged-heads write.  The attention site may have sent ct to the scratch by then,
//             and the merged-heads write follows it there.
//   RMS_NORM  the router with its norm consumes the RMS_NORM, its MUL and the logits; site_rms_norm_mul would otherwise run or
//             hold back the pair, and the router would find its MUL issued.
// A MUL_MAT on an F32 src0 and a SOFT_MAX can only start a router, an ADD a residual add + norm, a SILU its hold-back, a ROPE
// the rope + KV store.
int graph_pass::offer_to_sites(int i, int gop) {
    const ggml_tensor * node = cgraph->nodes[i];
    int r = 0;
    switch (node->op) {
        case GGML_OP_MUL:
            if (deferred[i]) return site_deferred_silu_mul(i);
            return site_moe_combine(i);
        case GGML_OP_UNARY:    return gop == QMM_OP_SILU ? site_hold_silu(i) : 0;
        case GGML_OP_ADD:      return site_add_rms_norm(i);
        case GGML_OP_MUL_MAT:                                                   // (QMM_OP_MUL_MAT_F: src0 is F16 or F32; gop 0: a view of a quantized K cache)
            if (kcache_block_type(node->src[0]->type)) return site_attention(i);
            if (node->src[0]->type != GGML_TYPE_F16) return site_moe_router(i);
            r = site_attention(i);
            return r ? r : site_kqv_into_merged_heads(i);
        case GGML_OP_RMS_NORM:
            r = site_moe_router(i);
            return r ? r : site_rms_norm_mul(i);
        case GGML_OP_SOFT_MAX: return site_moe_router(i);
        case GGML_OP_ROPE:     return site_rope_kv_attention(i);
        default:               return 0;
    }
}

} // namespace mi355x
