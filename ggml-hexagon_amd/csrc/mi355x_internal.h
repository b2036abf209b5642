// mi355x_internal.h — what the plugin's source files share: the context structs, the switches, the timers and every function
// one file defines and another calls.  The files, by concern (ggml-mi355x.cpp includes the other six: one translation unit):
//   ggml-mi355x.cpp     backend (stream) interface, device, registry, the exported entry points
//   mi355x_buffers.cpp  device buffer type, pinned host buffer type, planar-weight bookkeeping
//   mi355x_split.cpp    row split: the split buffer type, compute_mul_mat_split*, the RCCL exchange
//   mi355x_alias.cpp    aliasing and hoisting rules (ranges_overlap ... hoist_elsewhere)
//   mi355x_graph.cpp    the graph pass: op gates, compute_glue, flash attention, analyze_readers, graph_compute
//   mi355x_sites.cpp    the fusion sites: one matcher per motif, the sites (match, alias decisions, issue), the dispatch by op
//   mi355x_mulmat.cpp   what issues MUL_MAT and MUL_MAT_ID: the group with its hoists and folds, the broadcast form, the expert pair
// Only ggml headers and the C-ABI are included; all HIP lives in libggml_mi355x_qmm.so.
#pragma once

#include "ggml-mi355x.h"
#include "ggml-backend-impl.h"
#include "ggml-impl.h"
#include "ggml_mi355x_qmm.h"
#include "ggml_mi355x_ops.h"
// the module must load against a kernel library that has no qmm_set_codebook (ggml opens backends with RTLD_NOW): a weak reference, null then
#pragma weak qmm_set_codebook
// ... or no qmm_rope_kq_store (the one-launch rope + store on a quantized K cache): null then, and rope(k) and its CPY run as their own nodes
#pragma weak qmm_rope_kq_store_supported
#pragma weak qmm_rope_kq_store
#include "qmm_switches.h"
#include "qmm_matvec_plan.h"

#include <algorithm>
#include <array>
#include <cstdio>
#include <cstdlib>
#include <chrono>
#include <cstring>
#include <atomic>
#include <map>
#include <set>
#include <mutex>
#include <string>
#include <vector>

namespace mi355x {

// ----------------------------------------------------------------------------------------------- switches
// The module's switches (qmm_switches.h), read once at first use.  Nothing else in the module looks at the environment.
struct plugin_switches {
    bool glue, fuse, attn_rope, repack, staged_set;                    // off only when set to 0
    bool chain, rccl, timing;                                          // on when set to a non-zero number
    bool no_pinned, debug;                                             // on by presence
    bool router_norm_off, prep_norm_off, router_logits_off, moe_swiglu_off, moe_combine_norm_off;
    bool prec_set, prec_bf16, prec_q8;                                 // GGML_MI355X_PREC present at all / asks for bf16 / for the Q8-exact mode
    int  virtual_devices;                                              // <= 0: the physical devices
};
plugin_switches read_plugin_switches();
inline const plugin_switches & sw() { static const plugin_switches s = read_plugin_switches(); return s; }
extern int g_fuse_override;            // -1: the environment decides; 0 / 1: set through the "ggml_backend_mi355x_set_fuse" proc address (tests)
inline bool fuse_off() { return g_fuse_override >= 0 ? g_fuse_override == 0 : !sw().fuse; }
inline bool dbg() { return sw().debug; }

// ----------------------------------------------------------------------------------------------- contexts
struct mi355x_device_ctx {
    int         ordinal = 0;
    qmm_ctx *   qmm = nullptr;
    std::string name;
    std::string description;
    ggml_backend_buffer_type buft{};
    std::string buft_name;
    // row split: staging for the copy of src1 and for this device's slice of dst when another device is the root of the op
    void *      stage_x = nullptr;
    size_t      stage_x_bytes = 0;
    void *      stage_d = nullptr;
    size_t      stage_d_bytes = 0;
    qmm_event * ev_done = nullptr;       // this device's slice has landed in the root's dst
    qmm_event * ev_ready = nullptr;      // (as root) src1 is ready on the root's stream
    std::vector<void *> retired;         // staging blocks outgrown while queued work may still read them: freed behind the next synchronize
    // Small set_tensor calls (the per-token inputs llama.cpp writes in front of every graph: token ids, positions, the KQ mask, the
    // output ids) go through a pinned ring and an asynchronous copy on the device's stream instead of a blocking copy each: the call
    // returns when the bytes are in the ring; everything queued later on the stream sees them, and every other way to the memory
    // (get_tensor, cpy_tensor, memset, clear: they use the NULL stream) settles the stream first.  GGML_MI355X_STAGED_SET=0: off.
    char *      ring = nullptr;
    size_t      ring_bytes = 0, ring_pos = 0;
    bool        staged_pending = false;
    std::mutex  ring_mu;
    // what this module has queued on the device's stream / what a synchronize has waited for: ggml_backend_sched synchronizes a backend
    // in front of every split input and behind every graph (six calls per generated token, five of them with nothing queued since the
    // last one); a wait on an idle stream still costs ~9 us of host time (round 3, GGML_MI355X_TIMING), so those return at once
    std::atomic<uint64_t> enq{0}, enq_synced{0};
    // prompt batches already run in QMM_PREC_BF16 (GGML_MI355X_PREC=bf16, or a first prompt met a weight block beyond the f16 range)
    bool        prefill_bf16 = false;
};

// SURVEY 8f-2, weight repack: Q4_0 / Q8_0 / Q6_K weight tensors are re-laid into aligned planes (qmm_repack_rows) the first time
// a MUL_MAT / MUL_MAT_ID reads them, in place, row by row: sizes and strides do not change, so nothing of ggml-alloc's view moves.
// (The AMX buffer type converts inside set_tensor and has no get_tensor, ggml/src/ggml-cpu/amx/amx.cpp; here llama.cpp's pipelined
// loader writes tensors in arbitrary byte chunks, so the conversion waits for the first use instead, and get_tensor, cpy_tensor and
// partial writes convert a tensor BACK to GGUF wire layout first: what leaves the buffer is always wire bytes.)
struct planar_rec { int wire_type; int64_t K, rows, row_bytes; size_t bytes; };
struct mi355x_buffer_ctx {
    mi355x_device_ctx * dev;
    void *              base;
    std::mutex                          mu;
    std::map<const char *, planar_rec>  planar;     // by the tensor's first byte
    std::set<const char *>              wire_only;  // weights that went back to wire layout for good (a view cut their rows)
};

// GGML_MI355X_TIMING=1: host wall time inside the module's transfer / synchronize entry points (what of libllama's time between two
// graphs is spent here), summed per entry point
inline double wall_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
struct host_timer {
    static constexpr int N = 8;
    static inline double us[N] = {}, pend_us[N] = {}, tg_us[N] = {}, pp_us[N] = {}; // all calls; calls since the last graph_compute; calls in front of one-token / prompt graphs
    static inline long long calls[N] = {}, pend_calls[N] = {}, tg_calls[N] = {}, pp_calls[N] = {};
    static inline int pp_seen = 0;
    static void flush(bool one_token) {
        for (int i = 0; i < N; ++i) {
            if (one_token) { tg_us[i] += pend_us[i]; tg_calls[i] += pend_calls[i]; }
            else if (pp_seen >= 2) { pp_us[i] += pend_us[i]; pp_calls[i] += pend_calls[i]; }      // (in front of the first two prompt graphs: the model's upload, first-use initialisations)
            pend_us[i] = 0; pend_calls[i] = 0;
        }
        if (!one_token) ++pp_seen;
    }
    static const char * name(int i) { static const char * n[N] = { "set_tensor", "get_tensor", "cpy_tensor", "set_tensor_async", "get_tensor_async", "cpy_tensor_async", "synchronize", "event" }; return n[i]; }
    int slot; double t0;
    explicit host_timer(int s) : slot(s), t0(sw().timing ? wall_us() : 0) {}
    ~host_timer() {
        if (t0 > 0) {
            const double dt = wall_us() - t0;
            us[slot] += dt; calls[slot]++; pend_us[slot] += dt; pend_calls[slot]++;
        }
    }
};
// ... and per graph_compute call: stream time of every graph (an event pair around its launches), summed per kind of graph, and where
// the HOST's time goes (wall clock, us): between two graph_compute calls (libllama: graph build, scheduler, input copies, sampling-free
// bookkeeping), in the reader analysis, in the issue loop, waiting in synchronize.  graph_compute calls begin / analyzed / issued / end
// in that order, and none of them with timing off; report() prints the sums when the backend is freed.
struct graph_timer {
    qmm_event * ev_t0 = nullptr, * ev_t1 = nullptr;
    double      ms_tg = 0, ms_pp = 0, ms_pp_min = 0;      // (min: the warm-up pass also repacks weights at their first use)
    int64_t     graphs_tg = 0, graphs_pp = 0, tokens_pp = 0;
    double      us_outside = 0, us_analyze = 0, us_issue = 0, us_wait = 0, t_exit = 0;       // around one-token graphs
    double      pp_outside = 0, pp_analyze = 0, pp_issue = 0, pp_wait = 0, t_exit_pp = 0;   // the same for prompt graphs
    int64_t     pp_outside_n = 0;
    double      t_enter = 0, t_analyzed = 0, t_issued = 0;                                   // of the call in flight
    void begin(const ggml_cgraph * cgraph);
    void analyzed(qmm_ctx * q);
    void issued(qmm_ctx * q);
    void end(qmm_ctx * q, const ggml_cgraph * cgraph);
    void report(qmm_ctx * q, const char * name);          // ... and destroys the events
};

struct mi355x_backend_ctx {
    mi355x_device_ctx * dev;
    std::string         name;
    qmm_event *         ev_copy = nullptr;   // cpy_tensor_async: "src is ready" on the source backend's stream
    // per-graph reader analysis (graph_compute): for every candidate tensor, who reads its memory in this graph
    struct reader_info { const ggml_tensor * t; int uses; int last_reader; bool glue_only; };
    std::vector<reader_info>         readers;
    uint64_t                         readers_sig = 0;        // signature of the graph `readers` was computed for (analyze_readers)
    int                              readers_sig_nodes = -1;
    // results of hoisted MUL_MATs that could not be written in place (their block of the compute buffer is still in use at
    // the earlier point): they live in `hoist_buf` and every reader gets the pointer swapped in to_qt
    struct redirect { const ggml_tensor * t; char * data; int last_reader; };
    std::vector<redirect>            redirects;
    void *                           hoist_buf = nullptr;
    size_t                           hoist_bytes = 0, hoist_used = 0;
    std::map<uintptr_t, uintptr_t>   later_ranges;   // analyze_readers: union of the byte ranges of the nodes behind the one looked at
    std::vector<const ggml_tensor *> skipped;
    std::vector<char>                done;
    std::vector<const ggml_tensor *> deferred;       // per node: the SILU whose result this MUL consumes in the same launch
    graph_timer                      timer;          // GGML_MI355X_TIMING=1
};

constexpr int LOOKAHEAD = 12;      // nodes scanned for MUL_MATs on the same src1 (q .. rope .. k .. rope .. v; gate, silu, up)

// what analyze_readers recorded for `t`; NULL when it is no candidate of this graph
inline const mi355x_backend_ctx::reader_info * find_reader(const mi355x_backend_ctx * ctx, const ggml_tensor * t) {
    const auto & rd = ctx->readers;
    auto it = std::lower_bound(rd.begin(), rd.end(), t, [](const mi355x_backend_ctx::reader_info & x, const ggml_tensor * y) { return x.t < y; });
    return it != rd.end() && it->t == t ? &*it : nullptr;
}
inline float rms_eps(const ggml_tensor * rn) { float eps; memcpy(&eps, rn->op_params, sizeof(float)); return eps; }
inline const ggml_tensor * root_of(const ggml_tensor * t) { return t->view_src ? t->view_src : t; }      // the tensor whose memory a view shows
struct sm_params { float scale, max_bias; };
inline sm_params soft_max_params(const ggml_tensor * sm) { sm_params p; memcpy(&p, sm->op_params, sizeof(p)); return p; }
// the status of a C-ABI launch that returned rc; a failure is logged as fmt (the names, then the library's error)
template <class... A> inline enum ggml_status launched(int rc, const char * fmt, A... names) {
    if (rc) GGML_LOG_ERROR(fmt, names..., qmm_last_error());
    return rc ? GGML_STATUS_FAILED : GGML_STATUS_SUCCESS;
}
// bytes from the first to the last float of N rows of `width` floats, `ld` floats apart
inline size_t rows_extent(int64_t N, int64_t ld, int64_t width) { return (size_t) ((N - 1) * ld + width) * sizeof(float); }

// ----------------------------------------------------------------------------------------------- ggml-mi355x.cpp
extern mi355x_device_ctx   g_devs[GGML_MI355X_MAX_DEVICES];
extern ggml_backend_device g_devices[GGML_MI355X_MAX_DEVICES];
extern int                 g_ndev;

// ----------------------------------------------------------------------------------------------- mi355x_buffers.cpp
extern const ggml_backend_buffer_type_i buft_iface;
const char * buft_get_name(ggml_backend_buffer_type_t buft);
ggml_backend_buffer_type_t host_buffer_type();
void settle(mi355x_device_ctx * d);
void planar_release(mi355x_buffer_ctx * bc, const char * p, size_t size, bool overwritten, void * stream);
mi355x_buffer_ctx * our_buffer_ctx(const ggml_tensor * t);
int dev_type(const ggml_tensor * t);
int weight_type(mi355x_backend_ctx * ctx, const ggml_tensor * t);
// the block types a quantized K cache comes in without flash attention (-ctk q8_0 / q4_0 / q4_1 / q5_0 / q5_1; IQ4_NL has no store on the
// device): kq reads a permuted view of such a cache as its src0
inline bool kcache_block_type(enum ggml_type t) {
    return t == GGML_TYPE_Q8_0 || t == GGML_TYPE_Q4_0 || t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1;
}

// ----------------------------------------------------------------------------------------------- mi355x_split.cpp
bool buft_is_split(ggml_backend_buffer_type_t buft);
inline bool is_split(const struct ggml_tensor * t) { return t->buffer && buft_is_split(t->buffer->buft); }
ggml_backend_buffer_type_t split_buffer_type(int main_device, const float * tensor_split);
bool grow(mi355x_device_ctx * d, void *& p, size_t & have, size_t need);
void free_retired();
enum ggml_status compute_mul_mat_split_group(mi355x_backend_ctx * ctx, ggml_tensor * const * nodes, int n_nodes, char * done);

// ----------------------------------------------------------------------------------------------- mi355x_alias.cpp
// (the three smallest are inline: the node loop asks them of every node)
// byte range a tensor occupies (views: the viewed bytes)
inline bool ranges_overlap(const ggml_tensor * x, const ggml_tensor * y) {
    if (!x->data || !y->data) return false;
    const char * x0 = (const char *) x->data, * y0 = (const char *) y->data;
    return x0 < y0 + ggml_nbytes(y) && y0 < x0 + ggml_nbytes(x);
}
inline bool bytes_overlap(const void * a, size_t an, const void * b, size_t bn) {
    const char * a0 = (const char *) a, * b0 = (const char *) b;
    return a && b && a0 < b0 + bn && b0 < a0 + an;
}
inline bool is_noop(const ggml_tensor * node) {
    return ggml_is_empty(node) || node->op == GGML_OP_NONE || node->op == GGML_OP_RESHAPE || node->op == GGML_OP_VIEW ||
           node->op == GGML_OP_PERMUTE || node->op == GGML_OP_TRANSPOSE;
}
bool early_write_ok(const ggml_tensor * late, std::initializer_list<const ggml_tensor *> operands, const ggml_tensor * inplace_ok = nullptr,
                    bool attn_q = false);
bool can_hoist(const ggml_tensor * t, const std::vector<const ggml_tensor *> & skipped);
void * hoist_elsewhere(mi355x_backend_ctx * ctx, const ggml_tensor * d);

// ----------------------------------------------------------------------------------------------- mi355x_graph.cpp
bool type_supported(enum ggml_type t);
extern bool g_codebook_ok[5];                                        // IQ3_XXS, IQ3_S, IQ2_XS, IQ2_S, IQ1_S and IQ1_M: every device holds the grid (mi355x_graph.cpp)
bool bf16_weight(const struct ggml_tensor * w);
bool is_ours(const struct ggml_tensor * t);
bool supports_mul_mat(const struct ggml_tensor * op);
bool supports_mul_mat_id(const struct ggml_tensor * op);
bool supports_glue(const ggml_tensor * node);
bool supports_flash_attn(const ggml_tensor * node);
int  glue_op(const ggml_tensor * node);
qmm_tensor to_qt(const ggml_tensor * t, const mi355x_backend_ctx * ctx);
int  op_compute(mi355x_backend_ctx * ctx, int op, const qmm_tensor * s0, const qmm_tensor * s1, const qmm_tensor * s2, const qmm_tensor * d);
enum ggml_status compute_glue(mi355x_backend_ctx * ctx, const ggml_tensor * node, int op, const ggml_tensor * s0, const ggml_tensor * s1, const ggml_tensor * s2);
enum { ATTN_DECODE = 1, ATTN_PREFILL = 2 };
int  issue_attention(mi355x_backend_ctx * ctx, const qmm_tensor & q, const qmm_tensor & k, const qmm_tensor & v, const qmm_tensor & m, const qmm_tensor & d,
                     float scale, const char * what, const char * name, bool probe_prefill);
enum ggml_status backend_graph_compute(ggml_backend_t backend, struct ggml_cgraph * cgraph);

// ----------------------------------------------------------------------------------------------- mi355x_mulmat.cpp
bool group_member(const ggml_tensor * t, const ggml_tensor * b, bool split);
// ----------------------------------------------------------------------------------------------- mi355x_sites.cpp
int  fused_pair(const ggml_tensor * n0, const ggml_tensor * n1, const ggml_tensor ** other);
struct mul_mat_call;

// ---- one graph_compute call (analysis / plan / issue apart) -----------------------------------------------------------
// analyze_readers() is the analysis; graph_pass holds what the launch sites share.  A fusion site (mi355x_sites.cpp) has three steps:
//   match   a match_* member, const: it reads the graph, done[] and the reader analysis and fills a record of node indices (plus the
//           variant chosen); it launches nothing and marks nothing.  Each motif has one matcher, shared by the sites that contain it.
//   alias   early_write_ok / can_hoist / hoist_elsewhere on the matched nodes, in a fixed order: hoist_elsewhere is the one step with a
//           side effect (it claims scratch and adds a redirect that every later to_qt follows, also when the library then declines).
//   issue   operands through to_qt, the library's *_supported probe, the one call through launched(), the debug line, done[] from the record.
// offer_to_sites(i, gop) offers glue node i to the sites that can start at its op (the table and its order: at its definition).  It and
// every site_*(i) return 1 when node i was issued (or held back), possibly together with later nodes marked in done[]; 0 when no
// pattern is there (the caller issues the node alone); -1 when a launch failed.
struct graph_pass {
    mi355x_backend_ctx * ctx;
    ggml_cgraph * cgraph;
    int n_nodes;
    std::vector<char> & done;
    std::vector<const ggml_tensor *> & deferred;
    // handed from a site to the MUL_MAT behind it (always the next live node that is issued):
    // RMS_NORM -> MUL(w), with `add` the residual ADD in front of it (prompt batches), held back for the `readers` MUL_MATs that read it ...
    struct norm_req { const ggml_tensor * rn = nullptr, * mul = nullptr, * w = nullptr; int readers = 0; const ggml_tensor * add = nullptr; };
    norm_req pending_norm;
    // ... and silu(gate) * up held back for the ffn_down `mm`, which forms the product in its activation prep (prompt batches)
    struct swiglu_src { const float * gate = nullptr; const float * up = nullptr; int64_t ld_gate = 0, ld_up = 0; const ggml_tensor * mm = nullptr; };
    swiglu_src pending_swiglu;
    const mi355x_backend_ctx::reader_info * info(const ggml_tensor * t) const { return find_reader(ctx, t); }
    bool single_use(const ggml_tensor * t) const { const auto * r = info(t); return r && r->uses == 1; }
    int next_live(int j) const { while (j < n_nodes && (done[j] || is_noop(cgraph->nodes[j]))) ++j; return j; }     // the first node from j on that still runs
    struct reader_group { int n = 0; int at[4] = { 0, 0, 0, 0 }; bool all = false; };
    reader_group scan_reader_group(const ggml_tensor * b, int start, int cap) const;
    // mi355x_sites.cpp.  The match records hold node indices, -1 where a part is absent or nothing matched
    struct attn_chain    { int kq = -1, sm = -1, kqv = -1, pm = -1, ct = -1; float scale = 0; };
    struct add_norm      { int add = -1, rn = -1, mul = -1; const ggml_tensor * w = nullptr; };
    enum router_form     { ROUTER_NONE = 0, ROUTER, ROUTER_LOGITS, ROUTER_LOGITS_NORM };       // what the launch computes besides the router itself
    struct router_match  { int nrm = -1, nmul = -1, lgt = -1, sm = -1, argsort = -1, get_rows = -1, sum_rows = -1, div = -1;
                           const ggml_tensor * nwgt = nullptr; int64_t n_used = 0; router_form form = ROUTER_NONE; };
    struct combine_match { int U = 0; int adds[63]; };                                        // U used experts (0: no match), their U - 1 ADDs
    struct rope_kv_match { int rk = -1, ck = -1, cv = -1; };                                  // rope(k), its store, v's store
    attn_chain    match_attention(int kq, int from, int last) const;
    add_norm      match_add_norm(int ja, const ggml_tensor * operand) const;
    router_match  match_router(int entry, std::vector<const ggml_tensor *> & skipped) const;
    combine_match match_moe_combine(int i) const;
    rope_kv_match match_rope_kv(int i) const;
    struct add_norm_operands { qmm_tensor a, b, w, sum, d; };
    add_norm_operands marshal_add_norm(const ggml_tensor * add, const ggml_tensor * mul, const ggml_tensor * w) const;
    enum ggml_status launch_add_rms_norm(const add_norm_operands & o, const ggml_tensor * add, const ggml_tensor * rn);     // (also fold_norm's way out)
    int issue_router(int entry, const router_match & r);
    int offer_to_sites(int i, int gop);
    int site_deferred_silu_mul(int i);
    int site_hold_silu(int i);
    int site_add_rms_norm(int i);
    int site_rms_norm_mul(int i);
    int site_attention(int i);
    int site_kqv_into_merged_heads(int i);
    int site_moe_combine(int i);
    int site_moe_router(int i);
    int site_rope_kv_attention(int i);
    // mi355x_mulmat.cpp: node i's own launch (GGML_OP_MUL_MAT on a quantized or BF16 weight, GGML_OP_MUL_MAT_ID) and the steps it is made of
    enum ggml_status issue_mul_mat(int i);
    enum ggml_status issue_mul_mat_id(int i);
    void form_group(int i, mul_mat_call & c);
    enum ggml_status fold_norm(int i, mul_mat_call & c);
    void fold_swiglu(int i, mul_mat_call & c);
    void fold_residual(int i, mul_mat_call & c);
    enum ggml_status launch(int i, const mul_mat_call & c);
    enum ggml_status issue_mul_mat_broadcast(int i);
    struct swiglu_match { int silu = -1, mul = -1; };
    swiglu_match find_swiglu(int i0, int i1, std::vector<const ggml_tensor *> * between) const;
    int issue_moe_pair_swiglu(int i, int twin, int type);
};

} // namespace mi355x
