// mi355x_buffers.cpp — the device buffer type (real HBM), the pinned host buffer type and the planar-weight bookkeeping.
#include "mi355x_internal.h"

namespace mi355x {

// ----------------------------------------------------------------------------------------------- planar weights

// every planar tensor that overlaps [p, p + size) goes back to wire layout (unless the range covers it and `overwritten`)
void planar_release(mi355x_buffer_ctx * bc, const char * p, size_t size, bool overwritten, void * stream) {
    std::lock_guard<std::mutex> lock(bc->mu);
    for (auto it = bc->planar.begin(); it != bc->planar.end();) {
        const char * t0 = it->first;
        const planar_rec & r = it->second;
        if (t0 < p + size && p < t0 + r.bytes) {
            const bool covered = overwritten && p <= t0 && t0 + r.bytes <= p + size;
            if (!covered) {
                // the buffer-level callers pass the NULL stream, and the device's own stream is non-blocking: launches queued
                // there that still read the planar rows (or the to-planar repack itself) must be through before the rows are re-laid
                void * own = qmm_stream(bc->dev->qmm);
                if (stream != own && qmm_synchronize(bc->dev->qmm, own)) GGML_LOG_ERROR("MI355X: %s\n", qmm_last_error());
                if (qmm_repack_rows(bc->dev->qmm, r.wire_type, (void *) t0, r.row_bytes, r.rows, r.K, 0, stream))
                    GGML_ABORT("MI355X: converting a planar weight back to wire layout failed: %s", qmm_last_error());
                // (a failing synchronize here reports conditions of OTHER work as well: a non-finite prefill, a bad expert id; they are
                // logged where they belong, not turned into an abort of this copy)
                if (qmm_synchronize(bc->dev->qmm, stream)) GGML_LOG_ERROR("MI355X: %s\n", qmm_last_error());
            }
            it = bc->planar.erase(it);
        } else {
            ++it;
        }
    }
}
// the tensor's buffer context when it lives in an ordinary (not split, not host) MI355X buffer
mi355x_buffer_ctx * our_buffer_ctx(const ggml_tensor * t) {
    ggml_backend_buffer_t b = t->view_src ? t->view_src->buffer : t->buffer;
    return b && b->buft->iface.get_name == buft_get_name ? (mi355x_buffer_ctx *) b->context : nullptr;
}
// type code for the kernel library: the planar code when the tensor's rows are in planar form (views: same rows as the root)
int dev_type(const ggml_tensor * t) {
    const ggml_tensor * root = t->view_src ? t->view_src : t;
    if (root->type != GGML_TYPE_Q4_0 && root->type != GGML_TYPE_Q8_0 && root->type != GGML_TYPE_Q6_K) return (int) t->type;
    mi355x_buffer_ctx * bc = our_buffer_ctx(root);
    if (!bc) return (int) t->type;
    std::lock_guard<std::mutex> lock(bc->mu);
    auto it = bc->planar.find((const char *) root->data);
    if (it == bc->planar.end()) return (int) t->type;
    if (t->ne[0] != root->ne[0] || t->nb[1] != root->nb[1]) {
        // a view that cuts rows of a planar weight (nothing in llama.cpp builds one; ADVICE r2: no abort): the weight goes back to wire
        // layout for good and the view is served from that
        GGML_LOG_WARN("MI355X: %s views part of the rows of %s; the weight returns to wire layout\n", t->name, root->name);
        const planar_rec r = it->second;
        void * own = qmm_stream(bc->dev->qmm);
        if (qmm_repack_rows(bc->dev->qmm, r.wire_type, (void *) it->first, r.row_bytes, r.rows, r.K, 0, own))
            GGML_ABORT("MI355X: converting a planar weight back to wire layout failed: %s", qmm_last_error());
        bc->wire_only.insert(it->first);
        bc->planar.erase(it);
        return (int) t->type;
    }
    return (int) t->type + 100;
}
// first use as a MUL_MAT / MUL_MAT_ID weight: convert the whole (root) tensor, on the compute stream, in front of the launch
int weight_type(mi355x_backend_ctx * ctx, const ggml_tensor * t) {
    const ggml_tensor * root = t->view_src ? t->view_src : t;
    mi355x_buffer_ctx * bc = sw().repack ? our_buffer_ctx(root) : nullptr;
    // weights only: a quantized tensor in a compute or KV buffer (a Q8_0 K cache) is rewritten all the time; re-laying it
    // in place behind its writers' backs would corrupt it
    if (bc && root->buffer && root->buffer->usage != GGML_BACKEND_BUFFER_USAGE_WEIGHTS) bc = nullptr;
    if (bf16_weight(root)) bc = nullptr;                          // BF16 rows have no planar form and the library is not asked about them
    int pt = bc ? qmm_planar_type((int) root->type, root->ne[0], (int64_t) root->nb[1]) : 0;
    if (sw().prec_q8 && root->type == GGML_TYPE_Q6_K) pt = 0;     // the Q8-exact prefill reads Q6_K in wire layout: planar rows would run as f16 on Q8
    if (!pt || !ggml_is_contiguous(root) || (uintptr_t) root->data % 16 || t->ne[0] != root->ne[0] || t->nb[1] != root->nb[1]) return dev_type(t);
    {
        std::lock_guard<std::mutex> lock(bc->mu);
        if (bc->planar.count((const char *) root->data)) return pt;
        if (bc->wire_only.count((const char *) root->data)) return (int) t->type;
        const int64_t rows = ggml_nrows(root);
        if (qmm_repack_rows(ctx->dev->qmm, (int) root->type, root->data, (int64_t) root->nb[1], rows, root->ne[0], 1, qmm_stream(ctx->dev->qmm))) {
            GGML_LOG_WARN("MI355X: repack of %s refused (%s); it stays in wire layout\n", root->name, qmm_last_error());
            return (int) t->type;
        }
        bc->planar[(const char *) root->data] = planar_rec{ (int) root->type, root->ne[0], rows, (int64_t) root->nb[1], ggml_nbytes(root) };
    }
    return pt;
}

// ----------------------------------------------------------------------------------------------- buffer

void buffer_free(ggml_backend_buffer_t buffer) {
    auto * ctx = (mi355x_buffer_ctx *) buffer->context;
    settle(ctx->dev);
    qmm_free(ctx->dev->qmm, ctx->base);
    delete ctx;
}
void * buffer_get_base(ggml_backend_buffer_t buffer) { return ((mi355x_buffer_ctx *) buffer->context)->base; }

enum ggml_status buffer_init_tensor(ggml_backend_buffer_t, struct ggml_tensor *) { return GGML_STATUS_SUCCESS; }

void buffer_memset_tensor(ggml_backend_buffer_t buffer, struct ggml_tensor * tensor, uint8_t value, size_t offset, size_t size) {
    auto * ctx = (mi355x_buffer_ctx *) buffer->context;
    settle(ctx->dev);
    planar_release(ctx, (const char *) tensor->data + offset, size, true, nullptr);
    if (qmm_memset(ctx->dev->qmm, (char *) tensor->data + offset, value, size, nullptr) || qmm_synchronize(ctx->dev->qmm, nullptr))
        GGML_ABORT("MI355X memset_tensor: %s", qmm_last_error());
}
constexpr size_t STAGED_SET_MAX = (size_t) 256 << 10, STAGED_RING = (size_t) 4 << 20;
// every path to device memory that does not run on the device's stream waits for the staged copies first
void settle(mi355x_device_ctx * d) {
    std::lock_guard<std::mutex> lock(d->ring_mu);
    if (d->staged_pending) {
        if (qmm_synchronize(d->qmm, qmm_stream(d->qmm))) GGML_LOG_ERROR("MI355X: %s\n", qmm_last_error());
        d->staged_pending = false;
    }
}
bool staged_set(mi355x_buffer_ctx * ctx, void * dst, const void * data, size_t size) {
    mi355x_device_ctx * d = ctx->dev;
    std::lock_guard<std::mutex> lock(d->ring_mu);
    if (!d->ring) {
        d->ring = (char *) qmm_host_malloc(d->qmm, STAGED_RING);
        if (!d->ring) return false;
        d->ring_bytes = STAGED_RING;
    }
    const size_t need = (size + 255) & ~(size_t) 255;
    if (d->ring_pos + need > d->ring_bytes) {                  // wrap: the slots in front are reused only behind the copies that read them
        if (qmm_synchronize(d->qmm, qmm_stream(d->qmm))) return false;
        d->ring_pos = 0;
    }
    memcpy(d->ring + d->ring_pos, data, size);
    if (qmm_memcpy_h2d_async(d->qmm, dst, d->ring + d->ring_pos, size, qmm_stream(d->qmm))) return false;
    d->ring_pos += need;
    d->staged_pending = true;       // (not counted in enq: the copy is ordered in front of everything queued later, its source is the ring, and every
    return true;                    //  other way to the destination settles the stream first: a synchronize need not wait for it)
}

void buffer_set_tensor(ggml_backend_buffer_t buffer, struct ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    host_timer timer_(0);
    auto * ctx = (mi355x_buffer_ctx *) buffer->context;
    if (size <= STAGED_SET_MAX && buffer->usage != GGML_BACKEND_BUFFER_USAGE_WEIGHTS && sw().staged_set) {
        bool empty;
        { std::lock_guard<std::mutex> lock(ctx->mu); empty = ctx->planar.empty(); }
        if (empty && staged_set(ctx, (char *) tensor->data + offset, data, size)) return;
    }
    settle(ctx->dev);
    planar_release(ctx, (const char *) tensor->data + offset, size, true, nullptr);       // wire bytes come in: the tensor is wire again
    if (qmm_memcpy_h2d(ctx->dev->qmm, (char *) tensor->data + offset, data, size, nullptr))
        GGML_ABORT("MI355X set_tensor: %s", qmm_last_error());
}
void buffer_get_tensor(ggml_backend_buffer_t buffer, const struct ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    host_timer timer_(1);
    auto * ctx = (mi355x_buffer_ctx *) buffer->context;
    settle(ctx->dev);
    planar_release(ctx, (const char *) tensor->data + offset, size, false, nullptr);      // wire bytes go out (converted again at the next use)
    if (qmm_memcpy_d2h(ctx->dev->qmm, data, (const char *) tensor->data + offset, size, nullptr))
        GGML_ABORT("MI355X get_tensor: %s", qmm_last_error());
}
bool buffer_cpy_tensor(ggml_backend_buffer_t buffer, const struct ggml_tensor * src, struct ggml_tensor * dst) {
    host_timer timer_(2);
    auto * ctx = (mi355x_buffer_ctx *) buffer->context;
    settle(ctx->dev);
    ggml_backend_buffer_t sb = src->view_src ? src->view_src->buffer : src->buffer;
    if (!sb || sb->buft->iface.get_name != buft_get_name) return false;           // not one of ours: let ggml stage through the host
    auto * sctx = (mi355x_buffer_ctx *) sb->context;
    if (sctx->dev != ctx->dev) return false;
    settle(sctx->dev);
    planar_release(sctx, (const char *) src->data, ggml_nbytes(src), false, nullptr);
    planar_release(ctx, (const char *) dst->data, ggml_nbytes(src), true, nullptr);
    if (qmm_memcpy_d2d(ctx->dev->qmm, dst->data, src->data, ggml_nbytes(src), nullptr) || qmm_synchronize(ctx->dev->qmm, nullptr))
        GGML_ABORT("MI355X cpy_tensor: %s", qmm_last_error());
    return true;
}
void buffer_clear(ggml_backend_buffer_t buffer, uint8_t value) {
    auto * ctx = (mi355x_buffer_ctx *) buffer->context;
    settle(ctx->dev);
    { std::lock_guard<std::mutex> lock(ctx->mu); ctx->planar.clear(); }
    if (qmm_memset(ctx->dev->qmm, ctx->base, value, buffer->size, nullptr) || qmm_synchronize(ctx->dev->qmm, nullptr))
        GGML_ABORT("MI355X clear: %s", qmm_last_error());
}

const ggml_backend_buffer_i buffer_iface = {
    /* .free_buffer   = */ buffer_free,
    /* .get_base      = */ buffer_get_base,
    /* .init_tensor   = */ buffer_init_tensor,
    /* .memset_tensor = */ buffer_memset_tensor,
    /* .set_tensor    = */ buffer_set_tensor,
    /* .get_tensor    = */ buffer_get_tensor,
    /* .cpy_tensor    = */ buffer_cpy_tensor,
    /* .clear         = */ buffer_clear,
    /* .reset         = */ nullptr,
};

// ----------------------------------------------------------------------------------------------- buffer type

const char * buft_get_name(ggml_backend_buffer_type_t buft) { return ((mi355x_device_ctx *) buft->context)->buft_name.c_str(); }

ggml_backend_buffer_t buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size) {
    auto * dev = (mi355x_device_ctx *) buft->context;
    void * p = qmm_malloc(dev->qmm, size + 256);        // +256: vector loads of the last weight row never leave the allocation
    if (!p) {
        GGML_LOG_ERROR("%s: allocating %.2f MiB on %s failed: %s\n", __func__, size / 1048576.0, dev->name.c_str(), qmm_last_error());
        return nullptr;
    }
    auto * bc = new mi355x_buffer_ctx;
    bc->dev = dev;
    bc->base = p;
    return ggml_backend_buffer_init(buft, buffer_iface, bc, size);
}
size_t buft_get_alignment(ggml_backend_buffer_type_t) { return 256; }
size_t buft_get_max_size(ggml_backend_buffer_type_t buft) {
    auto * dev = (mi355x_device_ctx *) buft->context;
    size_t f = 0, t = 0;
    qmm_device_info(dev->qmm, nullptr, 0, &f, &t, nullptr);
    return t;
}
bool buft_is_host(ggml_backend_buffer_type_t) { return false; }

const ggml_backend_buffer_type_i buft_iface = {
    /* .get_name       = */ buft_get_name,
    /* .alloc_buffer   = */ buft_alloc_buffer,
    /* .get_alignment  = */ buft_get_alignment,
    /* .get_max_size   = */ buft_get_max_size,
    /* .get_alloc_size = */ nullptr,
    /* .is_host        = */ buft_is_host,
};

// ----------------------------------------------------------------------------------------------- host (pinned) buffer type
// with caps {async, host_buffer, events} llama.cpp's loader uploads through four pinned staging buffers and
// events (src/llama-model-loader.cpp:904-1079) and the scheduler gives the CPU backend's compute buffer this type, so the
// per-token inputs leave from page-locked memory.  The buffer itself is an ordinary CPU buffer over hipHostMalloc'ed memory.

const char * host_buft_get_name(ggml_backend_buffer_type_t) { return GGML_MI355X_BACKEND_NAME "_Host"; }
void host_buffer_free(ggml_backend_buffer_t buffer) { qmm_host_free(g_devs[0].qmm, buffer->context); }
ggml_backend_buffer_t host_buft_alloc_buffer(ggml_backend_buffer_type_t buft, size_t size) {
    void * p = sw().no_pinned ? nullptr : qmm_host_malloc(g_devs[0].qmm, size);
    if (!p) return ggml_backend_buft_alloc_buffer(ggml_backend_cpu_buffer_type(), size);      // pageable memory still works, just slower
    ggml_backend_buffer_t buffer = ggml_backend_cpu_buffer_from_ptr(p, size);
    buffer->buft = buft;
    buffer->iface.free_buffer = host_buffer_free;
    return buffer;
}
ggml_backend_buffer_type_t host_buffer_type() {
    static ggml_backend_buffer_type buft = {
        { host_buft_get_name, host_buft_alloc_buffer, ggml_backend_cpu_buffer_type()->iface.get_alignment, nullptr,
          ggml_backend_cpu_buffer_type()->iface.get_alloc_size, ggml_backend_cpu_buffer_type()->iface.is_host },
        &g_devices[0], nullptr };
    return &buft;
}

} // namespace mi355x
