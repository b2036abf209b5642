// mi355x_mulmat.cpp — everything that issues MUL_MAT and MUL_MAT_ID: the group on one src1 with its hoists, the norm, SwiGLU and residual
// folds, the SwiGLU-input ffn_down, the broadcast form, the expert pair.  Each product is decided first (a mul_mat_call filled in steps)
// and issued once (launch); the row-split group lives in mi355x_split.cpp.
#include "mi355x_internal.h"

namespace mi355x {

// Is `t` a quantized MUL_MAT of the group that reads the activation `b` as src1 (wq / wk / wv, ffn_gate / ffn_up)?  The one test the
// fusion sites, form_group and the row-split group share.  `split` picks the kind of weight: false = an ordinary 2-D weight of
// this device's buffer type; true = a row-split weight (compute_mul_mat_split_group: quantized by dev_supports_op's gate, 2-D by
// split_buffer_init_tensor, so the split buffer type itself stands in for the other conditions).
bool group_member(const ggml_tensor * t, const ggml_tensor * b, bool split) {
    if (t->op != GGML_OP_MUL_MAT || t->src[1] != b) return false;
    const ggml_tensor * w = t->src[0];
    if (split) return is_split(w) && supports_mul_mat(t);
    return !glue_op(t) && supports_mul_mat(t) && is_ours(w) && !is_split(w) && w->ne[2] == 1 && w->ne[3] == 1;
}

// One MUL_MAT launch, described before it is made.  issue_mul_mat fills it in steps: form_group, then the folds in the order (a) norm,
// (c) SwiGLU, (b) residual ((c) asks mv_fits_swiglu with the norm already decided).  A step either edits the description and marks what
// it absorbed in done[], or leaves it untouched; launch() makes the one call.
struct mul_mat_call {
    qmm_weight    ws[4];                                   // the group: its matrices, each with the place of its result, ...
    int           n = 0, member[4] = { 0, 0, 0, 0 };       // ... and the node index of each
    const float * x = nullptr;                             // src1 (a merged-heads CONT may live in the scratch: attention sites)
    int64_t       ldx = 0, K = 0, N = 0;
    qmm_mv_extra  ex{};
    bool          use_ex = false;
    bool          folds = true;                            // BF16 matrices take no norm, SwiGLU or residual
    graph_pass::swiglu_src sg;                             // ffn_down of a prompt batch: its prep forms x = silu(gate) * up
};

// `w` as a matrix of a group whose result for node `d` goes to `out` (d->data, or the scratch)
static qmm_weight group_weight(mi355x_backend_ctx * ctx, const ggml_tensor * w, const ggml_tensor * d, void * out) {
    return qmm_weight{ w->data, (int64_t) w->nb[1], w->ne[1], (float *) out, (int64_t) (d->nb[1] / sizeof(float)), weight_type(ctx, w) };
}

// Group the MUL_MAT nodes that read the same src1 (wq/wk/wv, ffn gate/up): batch <= 8: one launch per weight type (or
// one mixed-type launch); larger batches: the 16-bit activation operand is prepared once per group.  In llama.cpp's
// graph order they are not neighbours (q, rope(q), k, rope(k), v; gate, silu, up), so the scan looks past other
// nodes and hoists a later MUL_MAT when that is safe (can_hoist).
void graph_pass::form_group(int i, mul_mat_call & c) {
    const ggml_tensor * dst = cgraph->nodes[i], * b = dst->src[1];
    c.K = dst->src[0]->ne[0];
    c.N = b->ne[1];
    c.member[c.n] = i;
    c.ws[c.n++] = group_weight(ctx, dst->src[0], dst, dst->data);
    std::vector<const ggml_tensor *> & skipped = ctx->skipped;
    skipped.clear();
    for (int j = i + 1; j < n_nodes && j <= i + LOOKAHEAD && c.n < 4 && !fuse_off(); ++j) {
        const ggml_tensor * d = cgraph->nodes[j];
        if (done[j] || is_noop(d)) continue;
        if (group_member(d, b, false) && d->src[0]->ne[0] == c.K) {
            void * out = d->data;
            if (!can_hoist(d, skipped)) out = hoist_elsewhere(ctx, d);             // its block is still in use here: compute into scratch
            if (out) {
                c.member[c.n] = j;
                c.ws[c.n++] = group_weight(ctx, d->src[0], d, out);
                done[j] = 1;
                continue;
            }
        }
        skipped.push_back(d);
    }
    const qmm_tensor qb = to_qt(b, ctx);
    if (dbg()) fprintf(stderr, "group of %d at %s (N=%lld) src1 %s %p -> %p\n", c.n, dst->name, (long long) c.N, b->name, b->data, qb.data);
    for (int m = 0; m < c.n; ++m) c.folds = c.folds && c.ws[m].type != (int) GGML_TYPE_BF16;
    if (!c.folds && dbg()) fprintf(stderr, "fusion declined: BF16 weights in the group at %s\n", dst->name);
    c.x = (const float *) qb.data;
    c.ldx = b->nb[1] / sizeof(float);
}

// (a) src1 is a held-back RMS_NORM * w (site_rms_norm_mul, site_add_rms_norm): when the group holds every reader of it the kernels form
//     the normed row themselves; otherwise it is materialized now, as the graph says
enum ggml_status graph_pass::fold_norm(int i, mul_mat_call & c) {
    const ggml_tensor * dst = cgraph->nodes[i];
    if (pending_norm.mul != dst->src[1]) return GGML_STATUS_SUCCESS;
    const norm_req pn = pending_norm;
    pending_norm = {};
    qmm_ctx * q = ctx->dev->qmm;
    // Few tokens: the kernels read the un-normed row while they write their results: a result that ggml-alloc placed in the block of
    // that row (dead once the norm has run, in the graph's order) would be overwritten under the staging of other workgroups.
    // A prompt batch (pn.add: site_add_rms_norm held ADD -> RMS_NORM -> MUL back): the group's activation prep adds, norms and stores the
    // sum.  The products are written by later launches of the same stream, so they may sit on the dead operands; not on the sum
    const ggml_tensor * kept = pn.rn->src[0];                                      // the un-normed row / the sum (= pn.add)
    bool norm_in_kernel = c.n == pn.readers && c.folds && (!pn.add || qmm_mul_mat_group_norm_supported(q, c.ws, c.n, c.K, c.N));
    for (int m = 0; norm_in_kernel && m < c.n; ++m)
        norm_in_kernel = !bytes_overlap(c.ws[m].dst, rows_extent(c.N, c.ws[m].ldd, c.ws[m].M), to_qt(kept, ctx).data, ggml_nbytes(kept));
    if (norm_in_kernel) {
        const ggml_tensor * x0 = pn.add ? pn.add->src[0] : kept;
        c.x = (const float *) to_qt(x0, ctx).data;
        c.ldx = x0->nb[1] / sizeof(float);
        c.ex.norm_w = (const float *) pn.w->data;
        c.ex.norm_eps = rms_eps(pn.rn);
        c.use_ex = true;
        if (pn.add) {
            const ggml_tensor * x1 = pn.add->src[1];
            c.ex.norm_add = (const float *) to_qt(x1, ctx).data;
            c.ex.norm_add_ld = x1->nb[1] / sizeof(float);
            c.ex.norm_sum = (float *) to_qt(pn.add, ctx).data;
            c.ex.norm_sum_ld = pn.add->nb[1] / sizeof(float);
            if (dbg()) fprintf(stderr, "fused: add + norm (%s) into the prep of %s\n", pn.add->name, dst->name);
        }
        return GGML_STATUS_SUCCESS;
    }
    if (!pn.add) {
        ggml_tensor tmp = *pn.mul;
        memcpy(tmp.op_params, pn.rn->op_params, sizeof(tmp.op_params));
        return compute_glue(ctx, &tmp, QMM_OP_RMS_NORM_MUL, kept, pn.w, nullptr);
    }
    // the graph's three nodes after all, as the site would have run them
    // TODO(advisor r3): the site's own launch asks early_write_ok of `mul` against the ADD's operands (e_ok); neither the
    // hold-back test nor this path does
    if (dbg()) fprintf(stderr, "fusion declined: add + norm (%s) into the prep of %s (group of %d of %d readers)\n", pn.add->name, dst->name, c.n, pn.readers);
    return launch_add_rms_norm(marshal_add_norm(pn.add, pn.mul, pn.w), pn.add, pn.rn);
}

// The SwiGLU behind a gate / up pair, nodes i0 and i1 (build_ffn, build_moe_ffn): a SILU of one result, then the MUL of it with the
// other, looked for among the live nodes behind i0.  Live nodes that are neither go to `between` (they run later than the fused
// launch: the caller answers for them); a caller that passes none accepts none, and the search ends at the first.
graph_pass::swiglu_match graph_pass::find_swiglu(int i0, int i1, std::vector<const ggml_tensor *> * between) const {
    const ggml_tensor * t0 = cgraph->nodes[i0], * t1 = cgraph->nodes[i1];
    swiglu_match s;
    for (int j = i0 + 1; j < n_nodes && j <= i0 + 2 * LOOKAHEAD; ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (j == i1 || done[j] || is_noop(t)) continue;
        if (s.silu < 0 && t->op == GGML_OP_UNARY && ggml_get_unary_op(t) == GGML_UNARY_OP_SILU && (t->src[0] == t0 || t->src[0] == t1)) { s.silu = j; continue; }
        if (s.silu >= 0 && t->op == GGML_OP_MUL) {
            const ggml_tensor * sl = cgraph->nodes[s.silu], * other = sl->src[0] == t0 ? t1 : t0;
            if ((t->src[0] == sl && t->src[1] == other) || (t->src[1] == sl && t->src[0] == other)) { s.mul = j; break; }
        }
        if (!between) break;
        between->push_back(t);
    }
    return s;
}

// (c) ffn_gate + ffn_up of a few-token batch whose only readers are silu(gate) and the MUL of the two (build_ffn's SwiGLU):
//     the kernel pairs the rows and writes the product; neither projection is stored
void graph_pass::fold_swiglu(int i, mul_mat_call & c) {
    if (!(c.n == 2 && c.folds && c.N <= QMM_MATVEC_MAX_N && qmm::mv_swiglu_pair(c.ws[0].type, c.ws[0].M, c.ws[1].type, c.ws[1].M) && !fuse_off())) return;
    const swiglu_match s = find_swiglu(i, c.member[1], nullptr);
    if (s.mul < 0) return;
    const ggml_tensor * t0 = cgraph->nodes[i], * t1 = cgraph->nodes[c.member[1]], * sl = cgraph->nodes[s.silu], * par = cgraph->nodes[s.mul];
    // the product lands in the MUL's buffer while the launch still stages x: that buffer must be disjoint from x (no live node lies
    // in between: the search accepted none)
    if (bytes_overlap(par->data, ggml_nbytes(par), c.x, rows_extent(c.N, c.ldx, c.K))) {
        if (dbg()) fprintf(stderr, "fusion declined: SwiGLU into %s\n", par->name);
        return;
    }
    if (single_use(t0) && single_use(t1) && single_use(sl) && ggml_are_same_shape(par, t0) && par->nb[0] == 4 &&
        !((par->flags | t0->flags | t1->flags) & GGML_TENSOR_FLAG_OUTPUT) && qmm::mv_fits_swiglu(c.N, c.K, c.ex.norm_w != nullptr)) {
        c.ex.swiglu = sl->src[0] == t0 ? 1 : 2;
        c.ws[0].dst = (float *) par->data;
        c.ws[0].ldd = (int64_t) (par->nb[1] / sizeof(float));
        done[s.silu] = done[s.mul] = 1;
        c.use_ex = true;
    }
}

// (b) a lone MUL_MAT whose only reader is the residual ADD right behind it (wo, ffn_down): dst = W x + residual, written
//     where the ADD would have put it
void graph_pass::fold_residual(int i, mul_mat_call & c) {
    const ggml_tensor * dst = cgraph->nodes[i];
    if (!(c.n == 1 && c.folds && c.N <= QMM_MATVEC_MAX_N && !fuse_off() && !(dst->flags & GGML_TENSOR_FLAG_OUTPUT))) return;
    const int j = next_live(i + 1);
    const ggml_tensor * add = j < n_nodes ? cgraph->nodes[j] : nullptr;
    if (!(add && single_use(dst) && add->op == GGML_OP_ADD && (add->src[0] == dst || add->src[1] == dst) && add->src[0] != add->src[1])) return;
    const ggml_tensor * r = add->src[0] == dst ? add->src[1] : add->src[0];
    // dst = W x + r is written where the ADD would put it, while x is still being staged by other workgroups: the ADD's buffer must
    // not be x's (ggml-alloc may hand the ADD the block of the dead src1), and r only where it is the very same rows (in place)
    const qmm_tensor qr = to_qt(r, ctx);
    const bool r_ok = !bytes_overlap(add->data, ggml_nbytes(add), qr.data, ggml_nbytes(r)) || (qr.data == add->data && r->nb[1] == add->nb[1]);
    const bool x_ok = !bytes_overlap(add->data, ggml_nbytes(add), c.x, rows_extent(c.N, c.ldx, c.K));
    if ((!r_ok || !x_ok) && dbg()) fprintf(stderr, "fusion declined: residual into %s\n", add->name);
    if (r_ok && x_ok && ggml_are_same_shape(r, dst) && ggml_are_same_shape(add, dst) && r->type == GGML_TYPE_F32 && r->nb[0] == 4 && add->nb[0] == 4 &&
        r->nb[1] == add->nb[1] && add->nb[1] % 4 == 0) {
        c.ex.residual[0] = (const float *) qr.data;
        c.ws[0].dst = (float *) add->data;
        c.ws[0].ldd = (int64_t) (add->nb[1] / sizeof(float));
        done[j] = 1;
        c.use_ex = true;
    }
}

// the one place a described MUL_MAT goes out
enum ggml_status graph_pass::launch(int i, const mul_mat_call & c) {
    qmm_ctx * q = ctx->dev->qmm;
    void * st = qmm_stream(q);
    const qmm_weight & w = c.ws[0];
    const int rc = c.sg.mm  ? qmm_mul_mat_swiglu_in(q, w.type, w.w, w.w_row_bytes, c.K, w.M, c.sg.gate, c.sg.ld_gate, c.sg.up, c.sg.ld_up, c.N, w.dst, w.ldd, st)
                 : c.use_ex ? qmm_mul_mat_group_ex(q, c.ws, c.n, c.K, c.x, c.N, c.ldx, &c.ex, st)
                            : qmm_mul_mat_group(q, c.ws, c.n, c.K, c.x, c.N, c.ldx, st);
    return launched(rc, c.sg.mm ? "MI355X MUL_MAT(%s) with SwiGLU input: %s\n" : "MI355X MUL_MAT(%s): %s\n", cgraph->nodes[i]->name);
}

// batched / broadcast form: one 2-D product per (i12, i13), src0 broadcast as ggml_compute_forward_mul_mat does
// (ggml-cpu.c:6711-6716: i03 = i13 / r3, i02 = i12 / r2)
enum ggml_status graph_pass::issue_mul_mat_broadcast(int i) {
    const ggml_tensor * dst = cgraph->nodes[i], * a = dst->src[0], * b = dst->src[1];
    qmm_ctx * q = ctx->dev->qmm;
    const int64_t r2 = b->ne[2] / a->ne[2], r3 = b->ne[3] / a->ne[3];
    for (int64_t i13 = 0; i13 < b->ne[3]; ++i13)
        for (int64_t i12 = 0; i12 < b->ne[2]; ++i12) {
            const char * wp = (const char *) a->data + (i12 / r2) * a->nb[2] + (i13 / r3) * a->nb[3];
            const char * xp = (const char *) b->data + i12 * b->nb[2] + i13 * b->nb[3];
            char * dp = (char *) dst->data + i12 * dst->nb[2] + i13 * dst->nb[3];
            const int rc = qmm_mul_mat(q, weight_type(ctx, a), wp, a->nb[1], a->ne[0], a->ne[1], (const float *) xp, b->ne[1], b->nb[1] / sizeof(float),
                                       (float *) dp, dst->nb[1] / sizeof(float), qmm_stream(q));
            if (rc) return launched(rc, "MI355X MUL_MAT(%s): %s\n", dst->name);
        }
    return GGML_STATUS_SUCCESS;
}

// node i is the MUL_MAT to run; later nodes that go out with it (its group, the folds) are marked in done[]
enum ggml_status graph_pass::issue_mul_mat(int i) {
    const ggml_tensor * dst = cgraph->nodes[i], * a = dst->src[0], * b = dst->src[1];
    mul_mat_call c;
    if (pending_swiglu.mm == dst) {                                                // site_deferred_silu_mul left gate and up for this ffn_down
        c.sg = pending_swiglu;
        pending_swiglu = {};
        c.ws[c.n++] = group_weight(ctx, a, dst, dst->data);
        c.K = a->ne[0];
        c.N = b->ne[1];
        return launch(i, c);
    }
    if (is_split(a)) return compute_mul_mat_split_group(ctx, cgraph->nodes + i, n_nodes - i, done.data() + i);
    if (a->ne[2] != 1 || a->ne[3] != 1 || b->ne[2] != 1 || b->ne[3] != 1) return issue_mul_mat_broadcast(i);
    form_group(i, c);
    const enum ggml_status st = fold_norm(i, c);
    if (st != GGML_STATUS_SUCCESS) return st;
    fold_swiglu(i, c);
    fold_residual(i, c);
    return launch(i, c);
}

// ---- MUL_MAT_ID

// ffn_gate_exps and ffn_up_exps are consecutive MUL_MAT_ID nodes on the same src1 and ids (llama.cpp build_moe_ffn): when the
// next node is such a twin, both go out in one call (one mat-vec launch, or one expert sort + activation prep)
static bool moe_twin(const ggml_tensor * d0, const ggml_tensor * d1) {
    if (d1->op != GGML_OP_MUL_MAT_ID || !supports_mul_mat_id(d1)) return false;
    const ggml_tensor * a0 = d0->src[0], * a1 = d1->src[0];
    if (d0->src[1] != d1->src[1] || d0->src[2] != d1->src[2] || a0 == a1 || !is_ours(a1) || !is_ours(d1)) return false;
    if (a0->type != a1->type || !ggml_are_same_shape(a0, a1) || a0->nb[1] != a1->nb[1] || a0->nb[2] != a1->nb[2]) return false;
    return d0->nb[1] == d1->nb[1] && d0->nb[2] == d1->nb[2] && ggml_are_same_shape(d0, d1);
}

// What qmm_mul_mat_id, _id_pair and _id_swiglu all take between the expert tensor(s) and the result(s): the experts' layout, src1 and
// the ids of MUL_MAT_ID node `dst`, marshalled once; `call` puts them into its entry point.
template <class F> static int with_id_operands(const ggml_tensor * dst, F && call) {
    const ggml_tensor * as = dst->src[0], * b = dst->src[1], * ids = dst->src[2];
    return call(as->nb[1], as->nb[2], as->ne[0], as->ne[1], as->ne[2], (const float *) b->data, b->ne[1], b->nb[1], b->nb[2],
                (const int32_t *) ids->data, ids->ne[0], ids->ne[1], ids->nb[1]);
}

// Token generation: the SwiGLU behind the pair i / twin (ggml_silu of one, ggml_mul with the other: ffn_moe_gate_par) in the same launch
// (round 3).  gate, up and the silu are then never written: each must have exactly the one reader of the pattern, all of them
// provably in this split (analyze_readers); the product is written HERE, two or three nodes early, while other workgroups still
// stage src1 and read the ids, and across whatever else the graph lists in between.  1: issued; 0: not there; -1: the launch failed.
int graph_pass::issue_moe_pair_swiglu(int i, int twin, int type) {
    const ggml_tensor * dst = cgraph->nodes[i], * dst1 = cgraph->nodes[twin], * b = dst->src[1], * ids = dst->src[2];
    if (!qmm_mul_mat_id_swiglu_supported(ids->ne[0], ids->ne[1]) || sw().moe_swiglu_off) return 0;
    std::vector<const ggml_tensor *> between;
    const swiglu_match s = find_swiglu(i, twin, &between);
    if (s.mul < 0) return 0;
    const ggml_tensor * sl = cgraph->nodes[s.silu], * par = cgraph->nodes[s.mul];
    const ggml_tensor * gate = sl->src[0], * up = gate == dst ? dst1 : dst;
    if (((gate->flags | up->flags | sl->flags) & GGML_TENSOR_FLAG_OUTPUT) || !single_use(gate) || !single_use(up) || !single_use(sl) || !is_ours(par) ||
        par->type != GGML_TYPE_F32 || !ggml_are_same_shape(par, dst) || par->nb[0] != 4 || par->nb[1] != dst->nb[1] || par->nb[2] != dst->nb[2] ||
        !can_hoist(par, between) || !early_write_ok(par, { b, ids })) return 0;
    qmm_ctx * q = ctx->dev->qmm;
    const int rc = with_id_operands(dst, [&](auto... m) { return qmm_mul_mat_id_swiglu(q, type, gate->src[0]->data, up->src[0]->data, m..., (float *) par->data, par->nb[1], par->nb[2], qmm_stream(q)); });
    if (launched(rc, "MI355X MUL_MAT_ID + SwiGLU(%s, %s): %s\n", dst->name, dst1->name) != GGML_STATUS_SUCCESS) return -1;
    if (dbg()) fprintf(stderr, "fused: expert pair + swiglu (%s)\n", par->name);
    done[twin] = done[s.silu] = done[s.mul] = 1;
    return 1;
}

enum ggml_status graph_pass::issue_mul_mat_id(int i) {
    const ggml_tensor * dst = cgraph->nodes[i], * as = dst->src[0];
    qmm_ctx * q = ctx->dev->qmm;
    // the twin (ffn_up_exps after ffn_gate_exps) may sit behind the SILU of the first one
    int twin = -1;
    std::vector<const ggml_tensor *> & skipped = ctx->skipped;
    skipped.clear();
    for (int j = i + 1; j < n_nodes && j <= i + LOOKAHEAD && twin < 0 && !fuse_off(); ++j) {
        const ggml_tensor * t = cgraph->nodes[j];
        if (done[j] || is_noop(t)) continue;
        if (moe_twin(dst, t) && can_hoist(t, skipped)) twin = j;
        else skipped.push_back(t);
        if (t->op == GGML_OP_MUL_MAT_ID && twin < 0) break;
    }
    void * st = qmm_stream(q);
    float * d0 = (float *) dst->data;
    if (twin < 0)
        return launched(with_id_operands(dst, [&](auto... m) { return qmm_mul_mat_id(q, weight_type(ctx, as), as->data, m..., d0, dst->nb[1], dst->nb[2], st); }),
                        "MI355X MUL_MAT_ID(%s): %s\n", dst->name);
    const ggml_tensor * dst1 = cgraph->nodes[twin];
    const int t0 = weight_type(ctx, as), t1 = weight_type(ctx, dst1->src[0]);
    if (t0 != t1) { GGML_LOG_ERROR("MI355X MUL_MAT_ID pair: layouts differ\n"); return GGML_STATUS_FAILED; }
    if (const int r = issue_moe_pair_swiglu(i, twin, t0)) return r > 0 ? GGML_STATUS_SUCCESS : GGML_STATUS_FAILED;
    const int rc = with_id_operands(dst, [&](auto... m) { return qmm_mul_mat_id_pair(q, t0, as->data, dst1->src[0]->data, m..., d0, (float *) dst1->data, dst->nb[1], dst->nb[2], st); });
    if (!rc) done[twin] = 1;
    return launched(rc, "MI355X MUL_MAT_ID(%s, %s): %s\n", dst->name, dst1->name);
}

} // namespace mi355x
