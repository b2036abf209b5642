// ggml-mi355x.cpp — ggml backend plugin for MI355X: reg / device / buffer type / buffer / backend vtables
// (contract: ggml/src/ggml-backend-impl.h:17-207) over the kernel C-ABI of include/ggml_mi355x_qmm.h (quantized MUL_MAT /
// MUL_MAT_ID, the hot path) and include/ggml_mi355x_ops.h (the other ops of a transformer layer).
//
// Mirrors the structure of the reference's "backend per ggml spec" section
// (ggml/src/ggml-hexagon/ggml-hexagon.cpp:5417-5427 buffer iface, 5708-5737 buffer type, 5818-5834 device iface,
// 5555-5574 graph_compute node loop, 5065-5115 supports_op gate, 5941-6007 reg, 6066-6125 init, 6127 DL_IMPL),
// with four deliberate differences:
//   * buffers are real HBM (is_host = false): weights are uploaded once by set_tensor and never re-marshalled
//     (the reference re-maps tensor memory through FastRPC per call, ggml-hexagon.cpp:4975-5060);
//   * op failures are reported as GGML_STATUS_FAILED (the reference logs and continues, :5053-5056);
//   * graph_compute schedules a split instead of walking it: MUL_MATs that share src1 run as one launch although llama.cpp's
//     graph order separates them, and chains of nodes (norm -> weight -> projections, projection -> residual add, gate / up ->
//     SwiGLU, rope -> KV-cache stores, KQ -> soft_max -> KQV -> head merge) run as single launches;
//   * pinned host buffers, asynchronous copies and events, so llama.cpp's pipelined loader applies.
// Row split over the devices of this process (llama.cpp -sm row) is the split buffer type of mi355x_split.cpp.
//
// This file: the switches, the backend (stream) interface, the device, the registry and the exported entry points; the other
// concerns have a file each (mi355x_internal.h lists them).  Only ggml headers and the C-ABI; all HIP lives in libggml_mi355x_qmm.so.
//
// The module stays ONE translation unit: this file is what every build recipe compiles, and it includes the six other sections below
// (so the node loop's small helpers inline across them as they did in one file).  Do not hand the sections to the compiler as well.

#include "mi355x_internal.h"

#include "mi355x_buffers.cpp"
#include "mi355x_split.cpp"
#include "mi355x_alias.cpp"
#include "mi355x_graph.cpp"
#include "mi355x_sites.cpp"
#include "mi355x_mulmat.cpp"

namespace mi355x {

plugin_switches read_plugin_switches() {
    using namespace qmm_sw;
    const values v = read();
    plugin_switches p{};
    p.glue = v[SW_GLUE];  p.fuse = v[SW_FUSE];  p.attn_rope = v[SW_ATTN_ROPE];  p.repack = v[SW_REPACK];  p.staged_set = v[SW_STAGED_SET];
    p.chain = v[SW_CHAIN] != 0;  p.rccl = v[SW_RCCL] != 0;  p.timing = v[SW_TIMING] != 0;
    p.no_pinned = v[SW_NO_PINNED];  p.debug = v[SW_DEBUG];
    p.router_norm_off = v[SW_ROUTER_NORM_OFF];  p.prep_norm_off = v[SW_PREP_NORM_OFF];  p.router_logits_off = v[SW_ROUTER_LOGITS_OFF];
    p.moe_swiglu_off = v[SW_MOE_SWIGLU_OFF];  p.moe_combine_norm_off = v[SW_MOE_COMBINE_NORM_OFF];
    p.prec_set = v.is_set(SW_PREC);  p.prec_bf16 = prec_is_bf16(v.str(SW_PREC));  p.prec_q8 = prec_is_q8(v.str(SW_PREC));
    p.virtual_devices = v.is_set(SW_VIRTUAL_DEVICES) ? atoi(v.str(SW_VIRTUAL_DEVICES)) : 0;
    return p;
}
int g_fuse_override = -1;
void set_fuse(int on) { g_fuse_override = on < 0 ? -1 : on != 0; }

mi355x_device_ctx      g_devs[GGML_MI355X_MAX_DEVICES];
ggml_backend_device    g_devices[GGML_MI355X_MAX_DEVICES];
int                    g_ndev = 0;

// ----------------------------------------------------------------------------------------------- codebooks (IQ3_XXS, IQ3_S, IQ2_XS, IQ2_S, IQ1_S / IQ1_M)

// The grids of the two 3-bit i-quants are tables of ggml's source; this module carries none.  It reads them out of the ggml it is
// loaded into, through the type's own to_float on blocks crafted so that every float IS one byte of one grid entry:
//   IQ3_XXS (98-byte block: f16 d | 64 index bytes | 8 sign / scale words): d = 4.0 and all words 0 make the sub-block scale
//           d * (0.5 + 0) * 0.5 = 1 and every sign +; block b holds the indices 64 b .. 64 b + 63;
//   IQ3_S   (110-byte block: f16 d | 64 index bytes | 8 qh bytes | 32 sign bytes | 4 scale bytes): d = 1.0, scales 0 (1 + 2 * 0 = 1),
//           signs 0; block b holds the low 8 bits of 64 b .. 64 b + 63, the ninth bit (qh) is set in blocks 4 .. 7.
// The four floats of group i of block b are the bytes of entry 64 b + i.  A table is used only if every float is an integer in 1 .. 255.
//
// The two 2-bit i-quants with eight weights per entry, the same way: d = 8.0, scales 0 and every sign + make the sub-block scale
// 8 * (0.5 + 0) * 0.25 = 1;
//   IQ2_XS  (74-byte block: f16 d | 32 u16 of a 9-bit index and a 7-bit sign index | 8 scale bytes): 16 blocks, qs[i] of block b = 32 b + i;
//   IQ2_S   (82-byte block: f16 d | 32 index low bytes | 32 sign bytes | 8 qh bytes | 8 scale bytes): 32 blocks, low byte (32 b + i) & 0xff,
//           qh[ib] = 0x55 * (32 b >> 8): all four entries of a sub-block get the block's two high index bits.
// The eight floats of entry i of block b are the bytes of entry e = 32 b + i: the words 2e (weights 0 .. 3) and 2e + 1 (4 .. 7).
// Every four consecutive floats are one table word, byte j = float j.
//
// The two 1-bit i-quants index one grid of 2048 entries of eight values -1 / 0 / +1; it is read through IQ1_S's dequantizer
//   IQ1_S   (50-byte block: f16 d | 32 index low bytes | 8 u16 of four 3-bit high index parts, a 3-bit scale and the delta sign): 64 blocks,
//           d = 8.0, low byte (32 b + i) & 0xff, qh[ib] = h | h << 3 | h << 6 | h << 9 with h = 32 b >> 8, scale bits 0, delta +:
// every float is 8 * (g + 0.125) = 8 g + 1, so the table is used only if every float is exactly -7, 1 or 9.  The words are IQ2's pair
// form with int8 bytes (0xff, 0x00, 0x01); the kernel library enables IQ1_S and IQ1_M on it.
static bool derive_iq1_grid(std::vector<uint32_t> & grid) {
    const struct ggml_type_traits * tt = ggml_get_type_traits(GGML_TYPE_IQ1_S);
    const size_t bs = 50, nblk = 64;
    if (!tt || !tt->to_float || tt->blck_size != 256 || tt->type_size != bs) return false;
    std::vector<uint8_t> blocks(nblk * bs, 0);
    for (size_t b = 0; b < nblk; ++b) {
        uint8_t * blk = blocks.data() + b * bs;
        blk[0] = 0x00;  blk[1] = 0x48;                               // f16 8.0, little-endian
        for (int i = 0; i < 32; ++i) blk[2 + i] = (uint8_t) ((32 * b + i) & 0xff);
        const unsigned h = (unsigned) ((32 * b) >> 8), qh = h | h << 3 | h << 6 | h << 9;
        for (int ib = 0; ib < 8; ++ib) { blk[34 + 2 * ib] = (uint8_t) (qh & 0xff);  blk[35 + 2 * ib] = (uint8_t) (qh >> 8); }
    }
    std::vector<float> out(nblk * 256);
    tt->to_float(blocks.data(), out.data(), (int64_t) out.size());
    grid.assign(nblk * 64, 0);
    for (size_t w = 0; w < grid.size(); ++w)
        for (int j = 0; j < 4; ++j) {
            const float v = out[4 * w + j];
            if (v != -7.0f && v != 1.0f && v != 9.0f) return false;
            grid[w] |= (v == -7.0f ? 0xffu : v == 9.0f ? 0x01u : 0x00u) << (8 * j);
        }
    return true;
}

bool derive_codebook(enum ggml_type type, std::vector<uint32_t> & grid) {
    if (type == GGML_TYPE_IQ1_S) return derive_iq1_grid(grid);
    const struct ggml_type_traits * tt = ggml_get_type_traits(type);
    const bool xxs = type == GGML_TYPE_IQ3_XXS, iq3 = xxs || type == GGML_TYPE_IQ3_S, xs = type == GGML_TYPE_IQ2_XS;
    const size_t bs = xxs ? 98 : iq3 ? 110 : xs ? 74 : 82, nblk = xxs ? 4 : iq3 ? 8 : xs ? 16 : 32;
    if (!tt || !tt->to_float || tt->blck_size != 256 || tt->type_size != bs) return false;
    std::vector<uint8_t> blocks(nblk * bs, 0);
    for (size_t b = 0; b < nblk; ++b) {
        uint8_t * blk = blocks.data() + b * bs;
        blk[0] = 0x00;  blk[1] = xxs ? 0x44 : iq3 ? 0x3c : 0x48;     // f16 4.0 / 1.0 / 8.0, little-endian
        if (iq3) {
            for (int i = 0; i < 64; ++i) blk[2 + i] = (uint8_t) (64 * b + i);
            if (!xxs && b >= 4) memset(blk + 66, 0xff, 8);
        } else {
            for (int i = 0; i < 32; ++i) {
                const unsigned e = (unsigned) (32 * b + i);
                if (xs) { blk[2 + 2 * i] = (uint8_t) (e & 0xff);  blk[3 + 2 * i] = (uint8_t) (e >> 8); }
                else      blk[2 + i] = (uint8_t) (e & 0xff);
            }
            if (!xs) memset(blk + 66, (int) (0x55 * ((32 * b) >> 8)), 8);
        }
    }
    std::vector<float> out(nblk * 256);
    tt->to_float(blocks.data(), out.data(), (int64_t) out.size());
    grid.assign(nblk * 64, 0);
    for (size_t w = 0; w < grid.size(); ++w)
        for (int j = 0; j < 4; ++j) {
            const float v = out[4 * w + j];
            if (!(v >= 1.0f && v <= 255.0f) || v != (float) (int) v) return false;
            grid[w] |= (uint32_t) (int) v << (8 * j);
        }
    return true;
}

// every device gets all five grids; a type counts as supported only if all of them took it (the last one serves IQ1_S and IQ1_M)
void set_codebooks() {
    const enum ggml_type types[5] = { GGML_TYPE_IQ3_XXS, GGML_TYPE_IQ3_S, GGML_TYPE_IQ2_XS, GGML_TYPE_IQ2_S, GGML_TYPE_IQ1_S };
    for (int k = 0; k < 5; ++k) {
        g_codebook_ok[k] = false;
        if (!qmm_set_codebook || g_ndev == 0) continue;              // a kernel library without the entry point: the types stay with the CPU
        std::vector<uint32_t> grid;
        if (!derive_codebook(types[k], grid)) {
            GGML_LOG_WARN("MI355X: no usable grid from ggml's %s dequantizer; the type stays on the CPU\n", ggml_type_name(types[k]));
            continue;
        }
        bool ok = true;
        for (int i = 0; i < g_ndev && ok; ++i)
            if (qmm_set_codebook(g_devs[i].qmm, (int) types[k], grid.data(), (int) grid.size())) {
                GGML_LOG_WARN("MI355X: %s: %s; the type stays on the CPU\n", ggml_type_name(types[k]), qmm_last_error());
                ok = false;
            }
        g_codebook_ok[k] = ok;
    }
}

// ----------------------------------------------------------------------------------------------- timing (GGML_MI355X_TIMING=1)

void graph_timer::begin(const ggml_cgraph * cgraph) {
    t_enter = wall_us();
    bool one = true;
    for (int i = 0; i < cgraph->n_nodes && one; ++i)
        if (cgraph->nodes[i]->op == GGML_OP_MUL_MAT && cgraph->nodes[i]->ne[2] == 1 && cgraph->nodes[i]->ne[1] > 1) one = false;
    host_timer::flush(one);
}
void graph_timer::analyzed(qmm_ctx * q) {
    t_analyzed = wall_us();
    if (!ev_t0) { ev_t0 = qmm_event_create_timing(q); ev_t1 = qmm_event_create_timing(q); }
    if (ev_t0 && ev_t1) qmm_event_record(q, ev_t0, qmm_stream(q));
}
void graph_timer::issued(qmm_ctx * q) {
    if (ev_t0 && ev_t1) qmm_event_record(q, ev_t1, qmm_stream(q));
    t_issued = wall_us();
}
void graph_timer::end(qmm_ctx * q, const ggml_cgraph * cgraph) {
    if (!ev_t0 || !ev_t1) return;
    float ms = 0.0f;
    int64_t n_tok = 1;                                   // tokens of the ubatch = ne[1] of the widest 2-D activation in the graph
    for (int i = 0; i < cgraph->n_nodes; ++i)
        if (cgraph->nodes[i]->op == GGML_OP_MUL_MAT && cgraph->nodes[i]->ne[2] == 1) n_tok = std::max<int64_t>(n_tok, cgraph->nodes[i]->ne[1]);
    if (qmm_event_elapsed_ms(q, ev_t0, ev_t1, &ms)) return;
    const double t_done = wall_us();
    if (n_tok == 1) {
        ms_tg += ms; graphs_tg++;
        if (t_exit > 0) us_outside += t_enter - t_exit;
        us_analyze += t_analyzed - t_enter;  us_issue += t_issued - t_analyzed;  us_wait += t_done - t_issued;
        t_exit = t_done;
        t_exit_pp = 0;
    } else {
        t_exit = 0; ms_pp += ms; graphs_pp++; tokens_pp += n_tok; if (ms_pp_min == 0 || ms < ms_pp_min) ms_pp_min = ms;
        if (graphs_pp > 1) {                                // (the first prompt graph also re-lays weights at their first use: not a sample)
            if (t_exit_pp > 0 && graphs_pp > 2) { pp_outside += t_enter - t_exit_pp; pp_outside_n++; }
            pp_analyze += t_analyzed - t_enter;  pp_issue += t_issued - t_analyzed;  pp_wait += t_done - t_issued;
        }
        t_exit_pp = t_done;
    }
}
void graph_timer::report(qmm_ctx * q, const char * name) {
    if (!ev_t0) return;
    fprintf(stderr, "MI355X timing %s: tg graphs %lld stream_ms %.3f | pp graphs %lld tokens %lld stream_ms %.3f min_ms %.3f\n", name,
            (long long) graphs_tg, ms_tg, (long long) graphs_pp, (long long) tokens_pp, ms_pp, ms_pp_min);
    for (int i = 0; i < host_timer::N; ++i)
        if (host_timer::tg_calls[i]) fprintf(stderr, "MI355X timing %s: %s in front of a one-token graph: %.2f calls, %.1f us each, %.1f us per graph\n", name, host_timer::name(i),
                                             host_timer::tg_calls[i] / (double) std::max<int64_t>(graphs_tg, 1), host_timer::tg_us[i] / (double) host_timer::tg_calls[i],
                                             host_timer::tg_us[i] / (double) std::max<int64_t>(graphs_tg, 1));
    if (graphs_tg > 1)
        fprintf(stderr, "MI355X timing %s: host us per tg graph: outside graph_compute %.1f | reader analysis %.1f | issue loop %.1f | waiting in synchronize %.1f\n", name,
                us_outside / (double) (graphs_tg - 1), us_analyze / (double) graphs_tg, us_issue / (double) graphs_tg, us_wait / (double) graphs_tg);
    for (int i = 0; i < host_timer::N && graphs_pp > 0; ++i)
        if (host_timer::pp_calls[i]) fprintf(stderr, "MI355X timing %s: %s in front of a prompt graph: %.2f calls, %.1f us each, %.1f us per graph\n", name, host_timer::name(i),
                                             host_timer::pp_calls[i] / (double) std::max<int64_t>(graphs_pp - 2, 1), host_timer::pp_us[i] / (double) host_timer::pp_calls[i],
                                             host_timer::pp_us[i] / (double) std::max<int64_t>(graphs_pp - 2, 1));
    if (graphs_pp > 1)
        fprintf(stderr, "MI355X timing %s: host us per pp graph: outside graph_compute %.1f (between consecutive prompt graphs) | reader analysis %.1f | issue loop %.1f | waiting in synchronize %.1f\n",
                name, pp_outside / (double) std::max<int64_t>(pp_outside_n, 1), pp_analyze / (double) (graphs_pp - 1), pp_issue / (double) (graphs_pp - 1),
                pp_wait / (double) (graphs_pp - 1));
    qmm_event_destroy(q, ev_t0);
    qmm_event_destroy(q, ev_t1);
}

// ----------------------------------------------------------------------------------------------- backend (stream)

const char * backend_get_name(ggml_backend_t backend) { return ((mi355x_backend_ctx *) backend->context)->name.c_str(); }

void backend_free(ggml_backend_t backend) {
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    if (ctx->ev_copy) qmm_event_destroy(ctx->dev->qmm, ctx->ev_copy);
    ctx->timer.report(ctx->dev->qmm, ctx->name.c_str());
    if (ctx->hoist_buf) {
        qmm_synchronize(ctx->dev->qmm, qmm_stream(ctx->dev->qmm));
        qmm_free(ctx->dev->qmm, ctx->hoist_buf);
    }
    delete ctx;
    delete backend;
}

// ---- asynchronous transfers and events: everything a backend does is ordered on its context's stream, so
// these are the stream-ordered forms of set/get/cpy (ggml-backend-impl.h:93-95) and record/wait (:114-116).
// graph_compute itself still ends with a stream synchronize (that is where a bad expert id is reported).
bool on_device(const struct ggml_tensor * t, const mi355x_device_ctx * dev) {
    ggml_backend_buffer_t b = t->view_src ? t->view_src->buffer : t->buffer;
    return b && b->buft->iface.get_name == buft_get_name && b->buft->context == (void *) dev;
}
void backend_set_tensor_async(ggml_backend_t backend, struct ggml_tensor * tensor, const void * data, size_t offset, size_t size) {
    host_timer timer_(3);
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    GGML_ASSERT(on_device(tensor, ctx->dev) && "set_tensor_async: tensor is not in this device's buffer type");
    ctx->dev->enq++;
    if (mi355x_buffer_ctx * bc = our_buffer_ctx(tensor)) planar_release(bc, (const char *) tensor->data + offset, size, true, qmm_stream(ctx->dev->qmm));
    if (qmm_memcpy_h2d_async(ctx->dev->qmm, (char *) tensor->data + offset, data, size, qmm_stream(ctx->dev->qmm)))
        GGML_ABORT("MI355X set_tensor_async: %s", qmm_last_error());
}
void backend_get_tensor_async(ggml_backend_t backend, const struct ggml_tensor * tensor, void * data, size_t offset, size_t size) {
    host_timer timer_(4);
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    GGML_ASSERT(on_device(tensor, ctx->dev) && "get_tensor_async: tensor is not in this device's buffer type");
    ctx->dev->enq++;
    if (mi355x_buffer_ctx * bc = our_buffer_ctx(tensor)) planar_release(bc, (const char *) tensor->data + offset, size, false, qmm_stream(ctx->dev->qmm));
    if (qmm_memcpy_d2h_async(ctx->dev->qmm, data, (const char *) tensor->data + offset, size, qmm_stream(ctx->dev->qmm)))
        GGML_ABORT("MI355X get_tensor_async: %s", qmm_last_error());
}
ggml_guid_t backend_guid() {
    static ggml_guid guid = { 0x4d, 0x49, 0x33, 0x35, 0x35, 0x58, 0x2d, 0x67, 0x66, 0x78, 0x39, 0x35, 0x30, 0x2d, 0x71, 0x6d };
    return &guid;
}
bool backend_cpy_tensor_async(ggml_backend_t backend_src, ggml_backend_t backend_dst, const struct ggml_tensor * src, struct ggml_tensor * dst) {
    host_timer timer_(5);
    if (!ggml_guid_matches(backend_src->guid, backend_guid()) || !ggml_guid_matches(backend_dst->guid, backend_guid())) return false;
    auto * sctx = (mi355x_backend_ctx *) backend_src->context;
    auto * dctx = (mi355x_backend_ctx *) backend_dst->context;
    if (!on_device(src, sctx->dev) || !on_device(dst, dctx->dev) || !ggml_is_contiguous(src) || !ggml_is_contiguous(dst)) return false;
    if (mi355x_buffer_ctx * bc = our_buffer_ctx(src)) planar_release(bc, (const char *) src->data, ggml_nbytes(src), false, qmm_stream(sctx->dev->qmm));
    if (mi355x_buffer_ctx * bc = our_buffer_ctx(dst)) planar_release(bc, (const char *) dst->data, ggml_nbytes(src), true, qmm_stream(dctx->dev->qmm));
    qmm_ctx * dq = dctx->dev->qmm;
    void * dst_stream = qmm_stream(dq);
    dctx->dev->enq++;
    if (sctx->dev != dctx->dev) {            // the copy runs on the destination's stream, behind what the source has queued
        if (!sctx->ev_copy) sctx->ev_copy = qmm_event_create(sctx->dev->qmm);
        if (!sctx->ev_copy || qmm_event_record(sctx->dev->qmm, sctx->ev_copy, qmm_stream(sctx->dev->qmm)) ||
            qmm_stream_wait_event(dq, dst_stream, sctx->ev_copy))
            GGML_ABORT("MI355X cpy_tensor_async: %s", qmm_last_error());
    }
    if (qmm_memcpy_d2d(dq, dst->data, src->data, ggml_nbytes(src), dst_stream)) GGML_ABORT("MI355X cpy_tensor_async: %s", qmm_last_error());
    return true;
}
void backend_event_record(ggml_backend_t backend, ggml_backend_event_t event) {
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    if (qmm_event_record(ctx->dev->qmm, (qmm_event *) event->context, qmm_stream(ctx->dev->qmm)))
        GGML_ABORT("MI355X event_record: %s", qmm_last_error());
}
void backend_event_wait(ggml_backend_t backend, ggml_backend_event_t event) {
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    ctx->dev->enq++;
    if (qmm_stream_wait_event(ctx->dev->qmm, qmm_stream(ctx->dev->qmm), (qmm_event *) event->context))
        GGML_ABORT("MI355X event_wait: %s", qmm_last_error());
}

void backend_synchronize(ggml_backend_t backend) {
    host_timer timer_(6);
    auto * ctx = (mi355x_backend_ctx *) backend->context;
    const uint64_t queued = ctx->dev->enq.load();
    if (queued == ctx->dev->enq_synced.load()) return;       // nothing queued by this module since the last wait on this stream
    if (qmm_synchronize(ctx->dev->qmm, qmm_stream(ctx->dev->qmm)))
        GGML_LOG_ERROR("MI355X synchronize: %s\n", qmm_last_error());
    { std::lock_guard<std::mutex> lock(ctx->dev->ring_mu); ctx->dev->staged_pending = false; }
    ctx->dev->enq_synced.store(queued);
}

const ggml_backend_i backend_iface = {
    /* .get_name           = */ backend_get_name,
    /* .free               = */ backend_free,
    /* .set_tensor_async   = */ backend_set_tensor_async,
    /* .get_tensor_async   = */ backend_get_tensor_async,
    /* .cpy_tensor_async   = */ backend_cpy_tensor_async,
    /* .synchronize        = */ backend_synchronize,
    /* .graph_plan_create  = */ nullptr,
    /* .graph_plan_free    = */ nullptr,
    /* .graph_plan_update  = */ nullptr,
    /* .graph_plan_compute = */ nullptr,
    /* .graph_compute      = */ backend_graph_compute,
    /* .event_record       = */ backend_event_record,
    /* .event_wait         = */ backend_event_wait,
};

// ----------------------------------------------------------------------------------------------- device

const char * dev_get_name(ggml_backend_dev_t dev) { return ((mi355x_device_ctx *) dev->context)->name.c_str(); }
const char * dev_get_description(ggml_backend_dev_t dev) { return ((mi355x_device_ctx *) dev->context)->description.c_str(); }
void dev_get_memory(ggml_backend_dev_t dev, size_t * free, size_t * total) {
    qmm_device_info(((mi355x_device_ctx *) dev->context)->qmm, nullptr, 0, free, total, nullptr);
}
enum ggml_backend_dev_type dev_get_type(ggml_backend_dev_t) { return GGML_BACKEND_DEVICE_TYPE_GPU; }
void dev_get_props(ggml_backend_dev_t dev, struct ggml_backend_dev_props * props) {
    props->name = dev_get_name(dev);
    props->description = dev_get_description(dev);
    props->type = GGML_BACKEND_DEVICE_TYPE_GPU;
    dev_get_memory(dev, &props->memory_free, &props->memory_total);
    props->caps = { /* async */ true, /* host_buffer */ true, /* buffer_from_host_ptr */ false, /* events */ true };
}
ggml_backend_t dev_init_backend(ggml_backend_dev_t dev, const char *) {
    auto * d = (mi355x_device_ctx *) dev->context;
    return new ggml_backend{ backend_guid(), backend_iface, dev, new mi355x_backend_ctx{ d, d->name } };
}
ggml_backend_buffer_type_t dev_get_buffer_type(ggml_backend_dev_t dev) { return &((mi355x_device_ctx *) dev->context)->buft; }

ggml_backend_buffer_type_t dev_get_host_buffer_type(ggml_backend_dev_t) { return host_buffer_type(); }

ggml_backend_event_t dev_event_new(ggml_backend_dev_t dev) {
    qmm_event * e = qmm_event_create(((mi355x_device_ctx *) dev->context)->qmm);
    if (!e) {
        GGML_LOG_ERROR("MI355X event_new: %s\n", qmm_last_error());
        return nullptr;
    }
    return new ggml_backend_event{ dev, e };
}
void dev_event_free(ggml_backend_dev_t dev, ggml_backend_event_t event) {
    qmm_event_destroy(((mi355x_device_ctx *) dev->context)->qmm, (qmm_event *) event->context);
    delete event;
}
void dev_event_synchronize(ggml_backend_dev_t dev, ggml_backend_event_t event) {
    if (qmm_event_synchronize(((mi355x_device_ctx *) dev->context)->qmm, (qmm_event *) event->context))
        GGML_ABORT("MI355X event_synchronize: %s", qmm_last_error());
}

bool dev_supports_op(ggml_backend_dev_t, const struct ggml_tensor * op) {
    // a row-split tensor has no address of its own (split_buffer_get_base): only the quantized MUL_MAT knows how to read one, as
    // src0.  Answering "no" here is also what keeps llama.cpp from placing norm weights in the split buffer type
    // (weight_buft_supported, src/llama-model.cpp:123-242; ggml-cuda.cu:2972-2982 has the same gate).  A BF16 weight is refused there too:
    // llama.cpp then places it whole in the device's own buffer type, where the BF16 kernels read it.
    for (int i = 0; i < GGML_MAX_SRC; ++i) {
        const ggml_tensor * s = op->src[i];
        if (s && s->buffer && buft_is_split(s->buffer->buft) && !(op->op == GGML_OP_MUL_MAT && i == 0 && type_supported(s->type) && !bf16_weight(s))) return false;
    }
    switch (op->op) {
        case GGML_OP_NONE: case GGML_OP_RESHAPE: case GGML_OP_VIEW: case GGML_OP_PERMUTE: case GGML_OP_TRANSPOSE:
            return true;
        case GGML_OP_MUL_MAT:    return glue_op(op) ? supports_glue(op) : supports_mul_mat(op);
        case GGML_OP_MUL_MAT_ID: return supports_mul_mat_id(op);
        case GGML_OP_FLASH_ATTN_EXT: return supports_flash_attn(op);
        default: return supports_glue(op);
    }
}
bool dev_supports_buft(ggml_backend_dev_t dev, ggml_backend_buffer_type_t buft) {
    if (buft_is_split(buft)) return true;                             // any device can be the root of a split MUL_MAT
    return buft->iface.get_name == buft_get_name && buft->context == dev->context;
}

const ggml_backend_device_i device_iface = {
    /* .get_name             = */ dev_get_name,
    /* .get_description      = */ dev_get_description,
    /* .get_memory           = */ dev_get_memory,
    /* .get_type             = */ dev_get_type,
    /* .get_props            = */ dev_get_props,
    /* .init_backend         = */ dev_init_backend,
    /* .get_buffer_type      = */ dev_get_buffer_type,
    /* .get_host_buffer_type = */ dev_get_host_buffer_type,
    /* .buffer_from_host_ptr = */ nullptr,
    /* .supports_op          = */ dev_supports_op,
    /* .supports_buft        = */ dev_supports_buft,
    /* .offload_op           = */ nullptr,
    /* .event_new            = */ dev_event_new,
    /* .event_free           = */ dev_event_free,
    /* .event_synchronize    = */ dev_event_synchronize,
};

// ----------------------------------------------------------------------------------------------- reg

const char * reg_get_name(ggml_backend_reg_t) { return GGML_MI355X_BACKEND_NAME; }
size_t reg_get_device_count(ggml_backend_reg_t) { return (size_t) g_ndev; }
ggml_backend_dev_t reg_get_device(ggml_backend_reg_t, size_t index) { return index < (size_t) g_ndev ? &g_devices[index] : nullptr; }
void * reg_get_proc_address(ggml_backend_reg_t, const char * name) {
    if (strcmp(name, "ggml_backend_split_buffer_type") == 0) return (void *) split_buffer_type;    // llama.cpp -sm row
    // void (*)(int on): multi-node launches on (1) / one launch per node (0) / back to GGML_MI355X_FUSE (-1); lets one process
    // compare both schedules of the same graph (tests/cpp/test_graph_fuzz.cpp)
    if (strcmp(name, "ggml_backend_mi355x_set_fuse") == 0) return (void *) set_fuse;
    return nullptr;
}

const ggml_backend_reg_i reg_iface = { reg_get_name, reg_get_device_count, reg_get_device, reg_get_proc_address };

} // namespace

using namespace mi355x;

extern "C" {

ggml_backend_reg_t ggml_backend_mi355x_reg(void) {
    static ggml_backend_reg reg = { GGML_BACKEND_API_VERSION, reg_iface, nullptr };
    static std::once_flag once;                                     // the reference guards its reg init too (ggml-hexagon.cpp:5953-5955)
    std::call_once(once, [] {
        const int n_phys = qmm_device_count();
        // GGML_MI355X_VIRTUAL_DEVICES=n registers n logical devices over the physical ones (round robin): lets the row split
        // be exercised on a one-GPU box (tests/test_gpu_split_buffer.py); each logical device has its own context and stream
        const int n = sw().virtual_devices > 0 && n_phys > 0 ? sw().virtual_devices : n_phys;
        for (int i = 0; i < n && g_ndev < GGML_MI355X_MAX_DEVICES; ++i) {
            qmm_ctx * q = qmm_create(i % n_phys);
            if (!q) {
                GGML_LOG_WARN("MI355X: skipping HIP device %d: %s\n", i, qmm_last_error());
                continue;
            }
            mi355x_device_ctx & d = g_devs[g_ndev];
            d.ordinal = i % n_phys;
            d.qmm = q;
            d.name = std::string(GGML_MI355X_BACKEND_NAME) + std::to_string(g_ndev);
            char nm[128] = { 0 };
            int cus = 0;
            qmm_device_info(q, nm, sizeof(nm), nullptr, nullptr, &cus);
            d.description = std::string(nm) + " (gfx950, " + std::to_string(cus) + " CUs)";
            d.buft_name = d.name;
            d.prefill_bf16 = sw().prec_bf16;
            g_devices[g_ndev] = ggml_backend_device{ device_iface, &reg, &d };
            d.buft = ggml_backend_buffer_type{ buft_iface, &g_devices[g_ndev], &d };
            ++g_ndev;
        }
        set_codebooks();
        GGML_LOG_INFO("MI355X backend: %d device(s); quantized MUL_MAT / MUL_MAT_ID (Q4_0 Q8_0 Q4_K Q5_K Q6_K)%s\n", g_ndev,
                      !sw().glue ? "" : " and the glue ops of a transformer layer");
    });
    return &reg;
}

int ggml_backend_mi355x_get_device_count(void) {
    ggml_backend_mi355x_reg();
    return g_ndev;
}

const char * ggml_backend_mi355x_get_devname(size_t dev_num) {
    ggml_backend_mi355x_reg();
    return dev_num < (size_t) g_ndev ? g_devs[dev_num].name.c_str() : "unknown";
}

ggml_backend_buffer_type_t ggml_backend_mi355x_buffer_type(size_t dev_num) {
    ggml_backend_mi355x_reg();
    return dev_num < (size_t) g_ndev ? &g_devs[dev_num].buft : nullptr;
}

ggml_backend_t ggml_backend_mi355x_init(size_t dev_num) {
    ggml_backend_mi355x_reg();
    if (dev_num >= (size_t) g_ndev) {
        GGML_LOG_ERROR("%s: invalid device %zu (have %d)\n", __func__, dev_num, g_ndev);
        return nullptr;
    }
    return dev_init_backend(&g_devices[dev_num], nullptr);
}

bool ggml_backend_is_mi355x(ggml_backend_t backend) { return backend != nullptr && ggml_guid_matches(backend->guid, backend_guid()); }

static int ggml_backend_mi355x_score(void) { return qmm_device_count() > 0 ? 100 : 0; }

} // extern "C"

GGML_BACKEND_DL_IMPL(ggml_backend_mi355x_reg)
GGML_BACKEND_DL_SCORE_IMPL(ggml_backend_mi355x_score)