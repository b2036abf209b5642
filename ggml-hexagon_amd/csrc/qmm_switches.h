// qmm_switches.h — the one list of GGML_MI355X_* environment switches: name, kind, default, one line of text.  Host only, nothing
// from HIP or ggml: the kernel library (qmm_create, qmm_ops.hip, qmm_comm.hip), the plugin and a plain g++ test all read the
// environment through this header and nowhere else.  INTEGRATION.md's table lists the same switches in the same order.
#pragma once

#include <cstdlib>
#include <cstring>

#define QMM_SWITCH_PREFIX "GGML_MI355X_"
#define QMM_SWITCH_ENV(NAME) QMM_SWITCH_PREFIX #NAME      // the variable's full name, for messages

// kinds:  ATOI     value = atoi(text), the default when unset
//         OFF0     1 unless set to a text whose atoi is 0 (unset, empty-but-nonzero, "1", "2": on)
//         PRESENT  1 when the variable exists at all, whatever it holds ("0" included)
//         STR      the text itself, NULL when unset
// X(NAME, kind, default, text); [lib] = read by the kernel library on every qmm_create (or once per process: ATTN_*, RCCL_LIB),
// [plugin] = read once by the ggml backend module at its first use
#define QMM_SWITCHES(X)                                                                                                              \
    X(PREC,                 STR,     0, "[lib+plugin] prefill numerics: bf16 (or 0) = bf16, q8 (or 2) = Q8-exact int8 MFMA for Q2_K .. Q6_K and IQ4_XS, anything else = f16 on Q8 activations (the default)") \
    X(ACT_MODE,             ATOI,    0, "[lib] Q8_0 activation rounding: 0 = quantize_row_q8_0_ref form, non-zero = x86 AVX2 form") \
    X(SPLITK,               ATOI,    1, "[lib] split K over workgroups when a prefill MUL_MAT has too few tiles; 0 = off, n > 1 caps the factor") \
    X(SPLITK_COMBINE,       ATOI,    0, "[lib] 1 = split-K ranges combined inside the launch instead of by a reduce kernel (measured a wash)") \
    X(SKINNY,               ATOI,    1, "[lib] few-token split-K MFMA kernel; 0 = off")                                            \
    X(SKINNY_MAXN,          ATOI,    0, "[lib] upper batch bound of the few-token kernel (accepted from 9 up; unset = 64, 128 for matrices with few row groups)") \
    X(MM_GROUP,             ATOI,    1, "[lib] one prefill launch per same-type group on one src1; 0 = one per matrix")              \
    X(MV_KMIX,              ATOI,    2, "[lib] mixed-type mat-vec launch: 0 = off, 1 = K-quant groups only, 2 = also groups with Q8_0 matrices") \
    X(MV_BPC,               ATOI,    1, "[lib] mat-vec blocks per CU (accepted in 1..8)")                                            \
    X(MV_ONEPASS,           ATOI,    1, "[lib] 0 = mat-vecs with a folded RMS norm stage through stage_rms_norm + quantize_rows again") \
    X(REGB_Q23,             ATOI,    1, "[lib] 0 = Q2_K / Q3_K prefill on the LDS-tile kernel instead of their register-B units")   \
    X(WIDE,                 ATOI,    1, "[lib] 256-token tiles for large Q4_K prefill launches; 0 = off")                            \
    X(R64,                  ATOI,    2, "[lib] Q4_K prefill through the 64-rows-per-wave kernel: bit 0 = for 256 x 128, bit 1 = for 256 x 256") \
    X(R64S,                 ATOI,    1, "[lib] 0 = the compiler-scheduled 64-rows-per-wave kernel instead of the hand-placed one")  \
    X(PREP_REG,             ATOI,    1, "[lib] 0 = the LDS-staged activation prep for Q8_K rows too")                                \
    X(ABLATE,               ATOI,    0, "[lib] development ablation word of the MFMA kernels (g_mfma_dbg); written only when set") \
    X(ATTN_SHORT,           OFF0,    1, "[lib] 0 = the general few-token attention kernel at every cache length")                    \
    X(ATTN_SPLIT,           OFF0,    1, "[lib] 0 = no split of long KV ranges over workgroups in the few-token attention")          \
    X(RCCL_LIB,             STR,     0, "[lib] path of the RCCL library to load in front of the default names")                      \
    X(CHAIN,                ATOI,    0, "[lib+plugin] plugin: non-zero = one-token MUL_MAT groups as persistent launches; library: 0 = qmm_chain_begin records nothing (unset: records)") \
    X(GLUE,                 OFF0,    1, "[plugin] 0 = offload the quantized MUL_MAT / MUL_MAT_ID only")                              \
    X(FUSE,                 OFF0,    1, "[plugin] 0 = one launch per graph node (ggml_backend_mi355x_set_fuse overrides)")          \
    X(ATTN_ROPE,            OFF0,    1, "[plugin] 0 = rope + KV store and the few-token attention as two launches")                  \
    X(REPACK,               OFF0,    1, "[plugin] 0 = keep Q4_0 / Q8_0 / Q6_K weights in GGUF wire layout")                          \
    X(STAGED_SET,           OFF0,    1, "[plugin] 0 = small set_tensor calls as blocking copies")                                    \
    X(RCCL,                 ATOI,    0, "[plugin] non-zero = the row split exchanges through RCCL instead of peer copies + events") \
    X(TIMING,               ATOI,    0, "[plugin] non-zero = stream and host time per graph, printed when the backend is freed")    \
    X(NO_PINNED,            PRESENT, 0, "[plugin] pageable host buffers")                                                            \
    X(DEBUG,                PRESENT, 0, "[plugin] one stderr line per group formed, fusion taken or declined, redirect")            \
    X(VIRTUAL_DEVICES,      STR,     0, "[plugin] n > 0 = n logical devices over the physical ones (row split on one GPU)")         \
    X(ROUTER_NORM_OFF,      PRESENT, 0, "[plugin] the MoE router launch without the RMS norm in front of its logits")               \
    X(PREP_NORM_OFF,        PRESENT, 0, "[plugin] prompt batches without the residual add + RMS norm folded into the activation prep") \
    X(ROUTER_LOGITS_OFF,    PRESENT, 0, "[plugin] the MoE router without its logits' product")                                      \
    X(MOE_SWIGLU_OFF,       PRESENT, 0, "[plugin] the expert pair without the SwiGLU")                                               \
    X(MOE_COMBINE_NORM_OFF, PRESENT, 0, "[plugin] the MoE combine without the residual add and RMS norm behind it")

namespace qmm_sw {

enum kind { ATOI, OFF0, PRESENT, STR };
enum id {
#define X(NAME, KIND, DEF, TEXT) SW_##NAME,
    QMM_SWITCHES(X)
#undef X
    SW_COUNT
};
struct desc { const char * name; kind k; int def; const char * text; };
inline const desc table[SW_COUNT] = {
#define X(NAME, KIND, DEF, TEXT) { QMM_SWITCH_ENV(NAME), KIND, DEF, TEXT },
    QMM_SWITCHES(X)
#undef X
};

// the one parse of GGML_MI355X_PREC
inline bool prec_is_bf16(const char * s) { return s && (!strcmp(s, "bf16") || !strcmp(s, "0")); }
inline bool prec_is_q8(const char * s) { return s && (!strcmp(s, "q8") || !strcmp(s, "2")); }

inline int parse(id i, const char * e) {
    const desc & d = table[i];
    switch (d.k) {
        case OFF0:    return !(e && atoi(e) == 0);
        case PRESENT: return e != nullptr;
        case STR:     return d.def;
        default:      break;
    }
    if (!e) return d.def;
    const int v = atoi(e);
    if (i == SW_MV_BPC && (v < 1 || v > 8)) return d.def;
    if (i == SW_SKINNY_MAXN && v < 9) return d.def;
    return v;
}

// one reading of the environment
struct values {
    int          v[SW_COUNT];
    const char * s[SW_COUNT];       // the variable's text, NULL when unset (any kind)
    int          operator[](id i) const { return v[i]; }
    bool         is_set(id i) const { return s[i] != nullptr; }
    const char * str(id i) const { return s[i]; }
};
inline values read() {
    values r;
    for (int i = 0; i < SW_COUNT; ++i) {
        r.s[i] = getenv(table[i].name);
        r.v[i] = parse((id) i, r.s[i]);
    }
    return r;
}
inline int         read_one(id i) { return parse(i, getenv(table[i].name)); }
inline const char * read_str(id i) { return getenv(table[i].name); }

} // namespace qmm_sw
