// mi355x_alias.cpp — when a launch may write a buffer early or run a node ahead of others: ggml-alloc reuses freed blocks, so every
// fusion and every hoist is a question about byte ranges.
#include "mi355x_internal.h"

namespace mi355x {

// A fused launch writes the buffer of a LATER node (`late`) at the position of an earlier one.  ggml-alloc may have given `late` a
// block that was freed once the earlier nodes' operands were dead, i.e. exactly the memory the launch still reads: other workgroups
// would overwrite it while it is being staged.  Legal only when `late` is disjoint from every operand (an operand at the very same
// address with the same row layout is fine where the launch reads an element before the same thread writes it: `inplace_ok`).
// The attention launches (qmm_attn_decode*, qmm_attn_prefill) write ct = the merged heads [Dv * H, N]; ggml-alloc likes to give ct
// the block of the dead Q.  That is in place and safe when the two coincide head for head: a workgroup owns one (head, token), reads
// its whole q row before anything else and writes the same bytes last; nobody else touches them.  `qv` is a view of Q as [D, H, N]
// (reshaped) or [D, N, H] (permuted); D must equal Dv.
bool attn_q_coincides(const ggml_tensor * ct, const ggml_tensor * qv) {
    if (!qv || qv->data != ct->data || qv->type != GGML_TYPE_F32 || qv->nb[0] != 4 || qv->ne[3] != 1) return false;
    const int64_t D = qv->ne[0];
    int hd = 1, td = 2;                                                             // head / token dimension of the view
    if (qv->nb[1] != (size_t) D * 4) { hd = 2; td = 1; }
    return qv->nb[hd] == (size_t) D * 4 && qv->nb[td] == ct->nb[1] && D * qv->ne[hd] == ct->ne[0] && qv->ne[td] == ct->ne[1];
}
bool early_write_ok(const ggml_tensor * late, std::initializer_list<const ggml_tensor *> operands, const ggml_tensor * inplace_ok, bool attn_q) {
    for (const ggml_tensor * o : operands) {
        if (!o || !ranges_overlap(late, o)) continue;
        if (o == inplace_ok && o->data == late->data && o->nb[1] == late->nb[1] && ggml_are_same_shape(o, late)) continue;
        if (attn_q && o == inplace_ok && attn_q_coincides(late, o)) continue;
        if (dbg()) fprintf(stderr, "fusion declined: %s would be written early over %s (%p ne %lld,%lld nb1 %zu | %p ne %lld,%lld,%lld nb %zu,%zu,%zu)\n", late->name, o->name,
                           late->data, (long long) late->ne[0], (long long) late->ne[1], late->nb[1], o->data, (long long) o->ne[0], (long long) o->ne[1],
                           (long long) o->ne[2], o->nb[0], o->nb[1], o->nb[2]);
        return false;
    }
    return true;
}
// may `t` run before the nodes in `skipped` although the graph lists it after them?  Its operands are ready (the caller
// checked), so the question is memory: ggml-alloc reuses freed blocks, so t's result must not land on anything a skipped
// node still reads or writes.
bool can_hoist(const ggml_tensor * t, const std::vector<const ggml_tensor *> & skipped) {
    for (const ggml_tensor * s : skipped) {
        if (ranges_overlap(t, s)) return false;
        for (int j = 0; j < GGML_MAX_SRC && s->src[j]; ++j)
            if (ranges_overlap(t, s->src[j])) return false;
    }
    return true;
}

// A MUL_MAT that cannot be hoisted in place (ggml-alloc gave it a block that is still live at the earlier point: in
// llama.cpp's layer Kcur reuses the block of the pre-RoPE Qcur) is computed into the context's scratch instead; every reader
// then gets the scratch pointer (to_qt).  Possible when all readers are glue ops of this graph and the result is not a graph
// output.  Returns NULL when it is not.
void * hoist_elsewhere(mi355x_backend_ctx * ctx, const ggml_tensor * d) {
    if (d->flags & GGML_TENSOR_FLAG_OUTPUT) return nullptr;
    const auto * it = find_reader(ctx, d);
    if (!it || !it->glue_only || it->uses == 0) return nullptr;
    const size_t bytes = (ggml_nbytes(d) + 255) & ~(size_t) 255;
    if (ctx->hoist_used + bytes > ctx->hoist_bytes) {
        if (ctx->hoist_used || !ctx->redirects.empty()) {                              // live results in the old block: not this time
            if (dbg()) fprintf(stderr, "hoist refused for %s: scratch exhausted (%zu of %zu bytes in use)\n", d->name, ctx->hoist_used, ctx->hoist_bytes);
            return nullptr;
        }
        if (!grow(ctx->dev, ctx->hoist_buf, ctx->hoist_bytes, std::max<size_t>((size_t) 64 << 20, 64 * bytes))) return nullptr;
    }
    char * p = (char *) ctx->hoist_buf + ctx->hoist_used;
    ctx->hoist_used += bytes;
    // the main loop drops redirects in order of their last reader
    auto pos = ctx->redirects.begin();
    while (pos != ctx->redirects.end() && pos->last_reader <= it->last_reader) ++pos;
    ctx->redirects.insert(pos, { d, p, it->last_reader });
    if (dbg()) fprintf(stderr, "redirect %s (%p) -> scratch %p, readers %d, last reader node %d\n", d->name, d->data, (void *) p, it->uses, it->last_reader);
    return p;
}

} // namespace mi355x
