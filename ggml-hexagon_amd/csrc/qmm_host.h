// qmm_host.h — host-side context and error plumbing shared by the launchers.
#pragma once

#include "../../include/ggml_mi355x_qmm.h"
#include "qmm_switches.h"
#include "qmm_types.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

namespace qmm { struct ChainStep; struct ChainSync; }

struct qmm_ctx {
    int         device = 0;
    hipStream_t stream = nullptr;
    int         cus = 0;
    int         act_mode = QMM_ACT_REF;
    int         prec = QMM_PREC_F16_Q8;
    int         mv_bpc = 1;          // mat-vec blocks per CU (tuning knob, GGML_MI355X_MV_BPC)
    int         mv_kmix = 2;         // one mixed-type mat-vec launch for K-quant groups of different types (GGML_MI355X_MV_KMIX=0: off; 1: not for groups that also hold Q8_0 matrices)
    int         mm_group = 1;        // prefill: one tiled launch for same-type matrices that share src1 (GGML_MI355X_MM_GROUP=0: off)
    int         skinny = 1;          // few-token split-K MFMA kernel (GGML_MI355X_SKINNY=0 turns it off)
    int         skinny_max_n = 64;   // ... used for 8 < N <= this, and up to skinny_max_n_few when the matrix has no more
    int         skinny_max_n_few = 128;  //     32-row groups than the chip has CUs (GGML_MI355X_SKINNY_MAXN sets both)
    // workspace of the batched path (16-bit activations, row scales, split-K slabs, MoE lists); grown on demand, sized once per call
    void *      ws = nullptr;
    size_t      ws_bytes = 0;
    int         splitk_combine = 0;  // GGML_MI355X_SPLITK_COMBINE=1: split-K ranges combined inside the launch (splitk_finish_wave) instead of by splitk_reduce_kernel.
                                     // Bit-identical, measured a wash on llama3-8b at 512 tokens (wo 46.1 -> 43.9 us, q/k/v 72.4 -> 73.0, ffn_down 105.5 -> 107.1): the
                                     // slabs' traffic stays, and the last arriver's four dependent read trips cost what the reduce launch cost.  Opt-in.
    int *       kcnt = nullptr;      // its arrival counters (zero between launches), one per (row tile, token tile, wave)
    int64_t     kcnt_n = 0;
    int *       flag = nullptr;      // device word set by kernels that meet an expert id out of range
    int64_t     id_calls = 0, id_checked = 0;       // MUL_MAT_ID launches issued / covered by the last look at `flag` (qmm_synchronize reads the word only behind such a launch: a blocking 4-byte copy per synchronize cost llama.cpp's token loop ~70 us per token)
    int64_t     mfma_calls = 0, mfma_checked = 0;   // prefill calls issued / covered by the last non-finite check (qmm_synchronize)
    bool        wide_attr_set = false;
    int         wide = 1;            // 256-token tiles for large Q4_K prefill launches (GGML_MI355X_WIDE=0: off)
    int         r64 = 2;             // Q4_K prefill, 64 rows per wave + LDS DMA (mfma_r64_q4k_kernel): bit 0 = in place of the 256 x 128 kernel, bit 1 = in place of the 256 x 256 one (GGML_MI355X_R64)
    int         r64s = 1;            // ... with the K-step's instruction stream placed by hand (mfma_r64s_q4k_kernel, qmm_mfma_r64s.hiph) where the 256 x 256 r64 kernel would run (GGML_MI355X_R64S=0: the compiler-scheduled kernel)
    int         mv_onepass = 1;      // GGML_MI355X_MV_ONEPASS=0: fused-norm mat-vecs stage through stage_rms_norm + quantize_rows again (A/B runs)
    int         prep_reg = 1;        // GGML_MI355X_PREP_REG=0: prep_act_kernel (LDS staging) for Q8_K rows too (A/B runs, parity tests)
    int         regb_q23 = 1;        // GGML_MI355X_REGB_Q23=0: Q2_K / Q3_K prefill on the LDS-tile kernel again (A/B runs)
    int         splitk = 1;          // split K over workgroups when a MUL_MAT has too few tiles (GGML_MI355X_SPLITK=0: off)
    // chains (qmm_chain.hiph): while recording, one-token MUL_MAT groups are collected instead of launched
    int         chain_enabled = 1;   // GGML_MI355X_CHAIN=0: qmm_chain_begin records nothing, every group is its own launch
    bool        chain_on = false;
    std::vector<qmm::ChainStep> * chain = nullptr;
    qmm::ChainSync * chain_sync = nullptr;      // device: arrival counters, generation, error word
    int         chain_launches = 0;  // persistent launches issued so far (tests / bench read it through qmm_chain_stats)
    int         chain_steps = 0;
    uint64_t *  chain_dbg = nullptr;  // qmm_chain_debug: device buffer the next persistent launches stamp their phases into
    bool        chain_attr_set = false;      // the kernel's dynamic-LDS limit has been raised on this device
    int         chain_checked = 0;   // chain_launches when the error word was last read
    hipStream_t chain_stream = nullptr;         // stream of the recorded steps
    bool        codebook[5] = { false, false, false, false, false };   // qmm_set_codebook: this context has the grid of IQ3_XXS / IQ3_S / IQ2_XS / IQ2_S / IQ1_S and IQ1_M (codebook_slot; until then the type is refused)
    char        name[128] = {0};
    // qmm_trace_begin / qmm_trace_end: while set, every kernel launch of the MUL_MAT path, of the glue launches behind qmm_op_compute /
    // qmm_op_add_rms_norm (run_glue of qmm_ops.hip) and of the attention entry points (qmm_attn.hiph) appends its label here (host side only; bench.py buckets its roofline by the kernels a call actually
    // issued, not by a replica of the dispatch rules; tests/test_gpu_glue_ops.py asserts the branch each of its cases was written for).
    // The glue labels, one per launch, name the kernel and the branch taken: the table GLUE_LABELS of qmm_glue_plan.h.
    // The attention labels are the plan's (qmm_attn_plan.h), spelled as rocprofv3 prints the kernels:
    //   attn_decode_short_kernel<D,fresh,width>   attn_decode_kernel<D,fresh>   attn_decode_split_kernel<D> then attn_combine_kernel   attn_prefill_kernel<D>
    //   attn_rows_decode_kernel<D> (a cut cache: then attn_combine_kernel)   attn_rows_prefill_kernel<D>      (QMM_TENSOR_KV_ROWS: FLASH_ATTN_EXT's operands)
    // A Q8_0 K cache (qmm_kcache.hiph; labels of qmm_kcache_plan.h): cpy_q8_0_quantize_kernel, cpy_q8_0_unpack_kernel<f32|f16>,
    //   attn_kq8_decode_kernel<D> (a cut cache: then attn_combine_kernel); the prompt form: cpy_q8_0_unpack_kernel<f16> then attn_prefill_kernel<D>
    // A K cache in T = q4_0 | q4_1 | q5_0 | q5_1 (qmm_kblk.hiph; labels of qmm_kblk_plan.h): cpy_T_quantize_kernel, cpy_T_unpack_kernel<f32|f16>,
    //   attn_kblk_decode_kernel<T,D> (a cut cache: then attn_combine_kernel); the prompt form: cpy_T_unpack_kernel<f16> then attn_prefill_kernel<D>
    // qmm_rope_kq_store (qmm_ropekq.hiph; label of qmm_ropekq_plan.h), T = q8_0 | q4_0 | q4_1 | q5_0 | q5_1: rope_kq_store_kernel<T,true|false> (true: the v part goes through tiles)
    // Untraced, a launch pays one pointer test.
    std::string * trace = nullptr;

    // `st` is used verbatim: NULL is HIP's default stream (what torch's default stream is), not ours
    hipStream_t s(void * st) const { return (hipStream_t) st; }
};

// launches what a recording context has collected (qmm_chain_begin); every entry point that queues other work calls it first, so
// stream order is the order of the calls whether or not a chain is being recorded.  Defined in qmm_api.hip.
int qmm_internal_chain_flush(qmm_ctx * c);
// the glue translation unit's copy of the codebook type's grid (qmm_device.hiph), on the current device.  Defined in qmm_ops.hip.
int qmm_internal_ops_codebook(int type, const uint32_t * entries, int n);
#define QMM_CHAIN_FLUSH(c)                                                      \
    do {                                                                        \
        if ((c)->chain_on) { int rc_ = qmm_internal_chain_flush(c); if (rc_) return rc_; } \
    } while (0)

#define QMM_TRACE(c, ...)                                                                   \
    do {                                                                                    \
        if ((c)->trace) { char b_[96]; snprintf(b_, sizeof(b_), __VA_ARGS__); (c)->trace->append(b_).push_back(';'); } \
    } while (0)

namespace qmm {

inline std::string & last_error() {
    static thread_local std::string e;
    return e;
}

inline int fail(int code, const char * fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    last_error() = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                       \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess) return ::qmm::fail(QMM_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

// IQ3_XXS / IQ3_S / IQ2_XS / IQ2_S / IQ1_S / IQ1_M before qmm_set_codebook: every launch is refused, nothing is computed
// (IQ1_S and IQ1_M index one grid: one slot, set through either id)
inline int codebook_slot(int type) { return type == T_IQ3_S ? 1 : type == T_IQ2_XS ? 2 : type == T_IQ2_S ? 3 : type_ternary(type) ? 4 : 0; }
inline int need_codebook(const qmm_ctx * c, int type, const char * who) {
    if (!type_codebook(type) || c->codebook[codebook_slot(type)]) return QMM_OK;
    return fail(QMM_EUNSUPPORTED, "%s: type %d needs its codebook first (qmm_set_codebook)", who, type);
}

// grows the context workspace; synchronizes the device when it has to reallocate
inline int ensure_ws(qmm_ctx * c, size_t bytes) {
    if (bytes <= c->ws_bytes) return QMM_OK;
    HIP_TRY(hipDeviceSynchronize());
    if (c->ws) HIP_TRY(hipFree(c->ws));
    c->ws = nullptr;
    c->ws_bytes = 0;
    const size_t gran = (size_t) 32 << 20;
    const size_t want = (bytes + gran - 1) / gran * gran;
    HIP_TRY(hipMalloc(&c->ws, want));
    c->ws_bytes = want;
    return QMM_OK;
}

} // namespace qmm
