// qmm_matvec_plan.h — the one launch plan of the few-token (N <= QMM_MATVEC_MAX_N) mat-vec paths: the LDS layout of the staged
// activations, the activation family of a weight type, the LDS fit estimates, and for a group call, a chain step or a few-pair
// MUL_MAT_ID which kernel runs with which template arguments, grid, block and LDS bytes, or why the call is refused.  Plain C++
// (no HIP, no ggml; a host compiler alone reads it, like qmm_prefill_plan.h).  The kernels take their LDS offsets from the same
// size functions; the launchers (mul_mat_group_impl, chain_step_plain, qmm_moe.hiph) execute a plan: run_matvec maps its kind, type, ntok and ex to
// the kernel instantiation and launches it, nothing else is decided there; the plugin
// asks the same fit predicates before it hands a norm or a SwiGLU to the library.
#pragma once

#include "../../include/ggml_mi355x_qmm.h"
#include "qmm_types.h"

#include <cstdio>

namespace qmm {

constexpr int MV_MAX_GROUP = 4;                              // matrices of one launch (MatvecGroup)
constexpr int MOE_MATVEC_MAX_PAIRS = 16;                     // (token, slot) pairs up to which MUL_MAT_ID runs as mat-vecs

// LDS of a workgroup: what a launch may ask for, and what the estimates made ahead of a launch (fusion sites, sub-batches) keep to
constexpr size_t MV_LDS_LAUNCH = 160 * 1024;
constexpr size_t MV_LDS_FIT    = 150 * 1024;

// ---------------------------------------------------------------------------------------------- activation staging sizes

// activations per int16 block sum of a type's mat-vec unit (MvUnit<T>::BSG; Q8_K activations only)
QMM_HD constexpr int mv_bsg(int type) { return type_base(type) == T_Q4_K || type_base(type) == T_Q5_K ? 32 : 16; }

// ntok rows of K staged for matvec_kernel<type>: int8 values, f32 block scales, then int16 block sums (Q8_K) or f32 sy (Q8_1).
// A weight type stands for its activation format (T_Q8_0 itself: the plain Q8_0 fields).
QMM_HD constexpr size_t mv_act_bytes(int type, int ntok, int K) {
    const int act = type_act(type);
    size_t b = (size_t) ntok * K + (size_t) ntok * (K / (act == T_Q8_K ? 256 : 32)) * 4;
    if (act == T_Q8_K) b += (size_t) ntok * (K / mv_bsg(type)) * 2;
    if (act == T_Q8_1) b += (size_t) ntok * (K / 32) * 4;            // sy per block
    return (b + 15) & ~(size_t) 15;
}
// ... for matvec_kmix_kernel and the chain's K-quant steps: Q8_K with block sums per 16 (behind them, with Q8_0 matrices in the
// group, the fields of mv_act_bytes(T_Q8_0P))
QMM_HD constexpr size_t mv_kmix_act_bytes(int ntok, int K) {
    return ((size_t) ntok * K + (size_t) ntok * (K / 256) * 4 + (size_t) ntok * (K / 16) * 2 + 15) & ~(size_t) 15;
}

// ---------------------------------------------------------------------------------------------- families

enum { CHAIN_FAM_NONE = -1, CHAIN_FAM_Q8_0 = 0, CHAIN_FAM_Q8_K = 1 };

// the mixed-type launch takes K-quant matrices (Q8_K activations) and, staged a second time, Q8_0 matrices
constexpr bool mv_kmix_kquant(int t) { return t == T_Q4_K || t == T_Q5_K || t == T_Q6_K || t == T_Q6_KP; }
constexpr bool mv_kmix_q80(int t) { return t == T_Q8_0 || t == T_Q8_0P; }
// a chain step takes the wire forms of the north-star formats, by activation format
constexpr int chain_family(int t) {
    return t == T_Q4_K || t == T_Q5_K || t == T_Q6_K ? CHAIN_FAM_Q8_K : t == T_Q4_0 || t == T_Q8_0 ? CHAIN_FAM_Q8_0 : CHAIN_FAM_NONE;
}
// the staged fields of a chain step.  The Q8_0 arm is mv_act_bytes(T_Q8_0, ntok, K) written out: matvec_chain_kernel takes its
// offset from here, and through the call hipcc places one scalar add of that kernel differently
QMM_HD constexpr size_t chain_act_bytes(int fam, int ntok, int K) {
    return fam == CHAIN_FAM_Q8_K ? mv_kmix_act_bytes(ntok, K) : (((size_t) ntok * K + (size_t) ntok * (K / 32) * 4 + 15) & ~(size_t) 15);
}
// two spellings of one layout give the same bytes for every K = step, 2 step, .. 32768 (32: K off the multiples of 256 too) and 1 .. 8 rows
template <typename F, typename G> constexpr bool mv_same_bytes(F f, G g, int step) {
    for (int K = step; K <= 32768; K += step) for (int n = 1; n <= QMM_MATVEC_MAX_N; ++n) if (f(n, K) != g(n, K)) return false;
    return true;
}
static_assert(mv_same_bytes([](int n, int K) { return chain_act_bytes(CHAIN_FAM_Q8_0, n, K); }, [](int n, int K) { return mv_act_bytes(T_Q8_0, n, K); }, 32), "one Q8_0 layout");

// ---------------------------------------------------------------------------------------------- fit estimates

inline bool mv_fits_plain(int64_t N, int64_t K) { return (size_t) N * K * 5 / 4 + 4096 <= MV_LDS_FIT; }
inline bool mv_fits_norm(int64_t N, int64_t K) { return (size_t) N * K * 4 + (size_t) N * K * 11 / 8 + 4096 <= MV_LDS_FIT; }
inline bool mv_fits_swiglu(int64_t N, int64_t K, bool norm) { return (size_t) N * K * 5 / 4 + (norm ? (size_t) N * K * 4 : 0) + 4096 <= MV_LDS_FIT; }
inline bool mv_fits_mixed(int64_t N, int64_t K) { return (size_t) N * K * 11 / 8 + 4096 <= MV_LDS_FIT; }
inline bool mv_fits_mixed_q80(int64_t N, int64_t K) { return (size_t) N * K * 21 / 8 + 4096 <= MV_LDS_FIT; }
// one token of a chain step, with the result slab of the persistent kernel behind the activations
inline bool chain_step_fits(int fam, int64_t K, bool norm, size_t slab) {
    return chain_act_bytes(fam, 1, (int) K) + (norm ? (size_t) K * 4 : 0) + slab + 1024 <= MV_LDS_FIT;
}
// the SwiGLU fold pairs the rows of two matrices of one type and shape
inline bool mv_swiglu_pair(int type0, int64_t M0, int type1, int64_t M1) { return type0 == type1 && M0 == M1; }

// ---------------------------------------------------------------------------------------------- one launch

// what the decision reads from the context (matvec_rules() in qmm_api.hip fills it from qmm_ctx)
struct MatvecRules { int cus, mv_bpc, mv_kmix, mv_onepass, act_mode; };

enum { MV_PER_TYPE,      // matvec_kernel<type, ntok, ex>
       MV_MIXED,         // matvec_kmix_kernel<ntok, ex>
       MV_MIXED_Q80 };   // matvec_kmix_kernel<ntok, ex, true>

inline int mv_kind_of(const int * type, int n) {
    for (int i = 1; i < n; ++i) if (type[i] != type[0]) return MV_MIXED;
    return MV_PER_TYPE;
}

struct MatvecLaunch {
    int    error;                     // QMM_OK, or the launch is refused (text() is then the message)
    int    kind, type;
    int    n, idx[MV_MAX_GROUP];      // the matrices: indices into the call's list
    int    row_end[MV_MAX_GROUP];     // ... and their cumulative row counts
    int    n0, ntok;                  // tokens n0 .. n0 + ntok - 1
    bool   ex;                        // the instantiation that honours residuals / norm / swiglu
    size_t lds;
    int    K, waves, blocks, act_arg;
    // the trace label (or the refusal); formatted on demand: this runs a few hundred times per generated token
    void text(char * b, size_t len) const {
        if (error && kind == MV_MIXED_Q80 && lds <= MV_LDS_LAUNCH) snprintf(b, len, "mixed-format matvec: up to 4 tokens");
        else if (error) snprintf(b, len, kind == MV_PER_TYPE ? "matvec: %d tokens x K=%d needs %zu B of LDS" : "mixed-type matvec: %d tokens x K=%d needs %zu B of LDS", ntok, K, lds);
        else if (kind == MV_PER_TYPE) snprintf(b, len, "matvec_kernel<%d,%d,%s>", type, ntok, ex ? "true" : "false");
        else snprintf(b, len, kind == MV_MIXED_Q80 ? "matvec_kmix_kernel<%d,%s,q8_0>" : "matvec_kmix_kernel<%d,%s>", ntok, ex ? "true" : "false");
    }
};

// n matrices (idx: their places in the call's list, nullptr = 0 .. n - 1; cumulative rows row_end) on rows n0 .. n0 + ntok - 1 of K as one launch
// of `kind`; res: the call's residual pointers by place in that list, or nullptr
inline MatvecLaunch matvec_launch(const MatvecRules & r, int kind, int type, const int * idx, const int * row_end, int n, int K, int n0, int ntok, bool norm, int swiglu,
                                  const float * const * res) {
    MatvecLaunch l;
    l.kind = kind;  l.type = type;  l.n = n;  l.n0 = n0;  l.ntok = ntok;  l.K = K;
    l.ex = norm || swiglu;
    for (int k = 0; k < n; ++k) { l.idx[k] = idx ? idx[k] : k; l.row_end[k] = row_end[k]; l.ex = l.ex || (res && res[l.idx[k]]); }
    l.lds = (kind == MV_PER_TYPE ? mv_act_bytes(type, ntok, K) : mv_kmix_act_bytes(ntok, K)) + (norm ? (size_t) ntok * K * 4 : 0) +
            (kind == MV_MIXED_Q80 ? mv_act_bytes(T_Q8_0P, ntok, K) : 0);
    l.error = l.lds > MV_LDS_LAUNCH || (kind == MV_MIXED_Q80 && ntok > 4) ? QMM_EUNSUPPORTED : QMM_OK;
    const int total = kind == MV_PER_TYPE && swiglu ? row_end[0] : row_end[n - 1];
    // one block per CU (the activation vector is quantized once per CU); 16 waves per block unless there are
    // fewer rows than that per CU.  Every wave gets a contiguous chunk of rows (+-1 row balance).
    const int per_cu = (total + r.cus - 1) / r.cus;
    l.waves  = per_cu > 8 ? 16 : per_cu > 4 ? 8 : 4;
    l.blocks = (total + l.waves - 1) / l.waves;
    if (l.blocks > r.cus * r.mv_bpc) l.blocks = r.cus * r.mv_bpc;
    l.act_arg = r.act_mode | (r.mv_onepass ? 0 : 256);
    return l;
}

// ---------------------------------------------------------------------------------------------- a group call

// the validation of a qmm_mul_mat_group_ex call with few-token extras, whatever N: QMM_OK, or the error code with its message
inline int matvec_extras_check(const qmm_weight * ws, int nw, int64_t K, int64_t N, const qmm_mv_extra * ex, char * msg, size_t len) {
    auto refuse = [&](int code, const char * fmt, long long a, long long b) { snprintf(msg, len, fmt, a, b); return code; };
    const bool norm = ex->norm_w != nullptr;
    if (N > QMM_MATVEC_MAX_N || nw > MV_MAX_GROUP) return refuse(QMM_EUNSUPPORTED, "qmm_mul_mat_group_ex: batches of <= %lld tokens, <= %lld matrices", QMM_MATVEC_MAX_N, MV_MAX_GROUP);
    if (norm && ((uintptr_t) ex->norm_w % 16 || ex->norm_eps < 0.0f)) return refuse(QMM_EINVAL, "qmm_mul_mat_group_ex: norm weight must be 16-byte aligned, eps >= 0", 0, 0);
    if (norm && !mv_fits_norm(N, K)) return refuse(QMM_EUNSUPPORTED, "qmm_mul_mat_group_ex: %lld rows of %lld do not fit LDS with the norm", N, K);
    if (ex->swiglu && ((ex->swiglu != 1 && ex->swiglu != 2) || nw != 2 || !mv_swiglu_pair(ws[0].type, ws[0].M, ws[1].type, ws[1].M) || ws[0].M <= 0 || ex->residual[0] || ex->residual[1] ||
                       !mv_fits_swiglu(N, K, norm)))
        return refuse(QMM_EUNSUPPORTED, "qmm_mul_mat_group_ex: swiglu wants two matrices of one type and shape, no residuals, all tokens in one launch", 0, 0);
    return QMM_OK;
}

struct MatvecPlan {
    int          n, next;             // launches; the first matrix they do not cover (== nw: the call is done, else plan again from there)
    MatvecLaunch launch[QMM_MATVEC_MAX_N];
};

// The plan for the matrices ws[0 .. nw - 1] (their type and M) that share N <= QMM_MATVEC_MAX_N rows of K, from matrix `first` on: the
// whole group as one mixed-type launch, or the run of same-type matrices that starts at `first` (up to MV_MAX_GROUP with rows; its
// tokens in sub-batches where they do not fit LDS together).  ex: nullptr for a plain call, else checked by matvec_extras_check.
inline MatvecPlan matvec_group_plan(const MatvecRules & r, const qmm_weight * ws, int nw, int64_t K, int64_t N, const qmm_mv_extra * ex, int first = 0) {
    MatvecPlan p;
    p.n = 0;  p.next = nw;
    const bool norm = ex && ex->norm_w;
    const int swiglu = ex ? ex->swiglu : 0;
    int idx[MV_MAX_GROUP], row_end[MV_MAX_GROUP], n = 0, rows = 0;
    auto launch = [&](int kind, int64_t n0, int64_t ntok) {
        p.launch[p.n++] = matvec_launch(r, kind, ws[first].type, idx, row_end, n, (int) K, (int) n0, (int) ntok, norm, swiglu, ex ? ex->residual : nullptr);
    };
    if (first == 0 && nw >= 2 && nw <= MV_MAX_GROUP && r.mv_kmix) {
        // K-quant matrices of different types share the Q8_K activations: one mixed-type launch for the whole group
        bool kq = true, mixed = false;
        int n_k = 0, n_80 = 0;                                    // K-quant matrices (Q8_K activations), Q8_0 matrices (Q8_0 activations)
        for (int i = 0; i < nw; ++i) {
            n_k += mv_kmix_kquant(ws[i].type);  n_80 += mv_kmix_q80(ws[i].type);
            kq = kq && (mv_kmix_kquant(ws[i].type) || mv_kmix_q80(ws[i].type)) && ws[i].M > 0;
            mixed = mixed || ws[i].type != ws[0].type;
            idx[i] = i;  row_end[i] = rows += (int) ws[i].M;
        }
        // both activation formats in one group (Mixtral's q in Q4_K with k / v in Q8_0): one launch that stages the row twice
        const bool q80 = n_80 > 0;
        if (q80) kq = kq && n_k > 0 && r.mv_kmix > 1 && N <= 4 && !norm && !swiglu && mv_fits_mixed_q80(N, K);
        if (kq && mixed && mv_fits_mixed(N, K)) { n = nw; launch(q80 ? MV_MIXED_Q80 : MV_MIXED, 0, N); return p; }
        rows = 0;
    }
    // one launch per run of same-type weights (they share the in-kernel activation quantization)
    for (p.next = first; p.next < nw && ws[p.next].type == ws[first].type && n < MV_MAX_GROUP; ++p.next)
        if (ws[p.next].M > 0) { idx[n] = p.next; row_end[n++] = rows += (int) ws[p.next].M; }
    // tokens that do not fit LDS together are processed in sub-batches
    int64_t n_at_once = N;
    while (n_at_once > 1 && !mv_fits_plain(n_at_once, K)) n_at_once = (n_at_once + 1) / 2;
    for (int64_t n0 = 0; n > 0 && n0 < N; n0 += n_at_once) launch(MV_PER_TYPE, n0, (N - n0) < n_at_once ? (N - n0) : n_at_once);
    return p;
}

// ---------------------------------------------------------------------------------------------- MUL_MAT_ID on a few pairs

enum { MOE_MV_SINGLE, MOE_MV_PAIR, MOE_MV_SWIGLU };        // one expert tensor; two on the same rows; two with the SwiGLU folded

inline bool moe_runs_as_matvec(int64_t n_used, int64_t n_tokens) { return n_used > 0 && n_tokens > 0 && n_used * n_tokens <= MOE_MATVEC_MAX_PAIRS; }

struct MoeMatvecPlan {
    int      form, type;
    size_t   lds;
    unsigned grid[3], block;
    void text(char * b, size_t len) const { snprintf(b, len, form == MOE_MV_SWIGLU ? "matvec_id_swiglu_kernel<%d>" : "matvec_id_kernel<%d>", type); }
};

// matvec_id_kernel<type> / matvec_id_swiglu_kernel<type> on P (token, slot) pairs of M rows each: x = pair, y = row chunks, z = tensor
inline MoeMatvecPlan moe_matvec_plan(int cus, int form, int type, int K, int M, int P) {
    MoeMatvecPlan p;
    p.form = form;  p.type = type;
    p.lds = mv_act_bytes(type, 1, K);
    const int nw = 8, nm = form == MOE_MV_PAIR ? 2 : 1;
    int by = (M + nw - 1) / nw;
    const int cap = (2 * cus + P * nm - 1) / (P * nm);
    if (by > cap) by = cap;
    if (by < 1) by = 1;
    p.grid[0] = (unsigned) P;  p.grid[1] = (unsigned) by;  p.grid[2] = (unsigned) nm;
    p.block = nw * 64;
    return p;
}

} // namespace qmm
