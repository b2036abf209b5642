// qmm_prefill_plan.h — the one launch plan of the prefill (N > QMM_MATVEC_MAX_N) path: for a weight type, the shapes of a run and
// the context's switches it decides the kernel with its template arguments, grid, block and LDS bytes, the split-K factor, the
// operand layout, the activation prep and its key, whether a run of matrices is one launch, and the workspace layout.  Plain C++
// (no HIP, no ggml; a host compiler alone reads it, like qmm_switches.h).  prefill_group_plan lists the launches of a whole
// qmm_mul_mat_group call: its runs, which of them prepare the operand, and the call's workspace.  The launchers (qmm_prefill.hiph,
// qmm_moe.hiph) execute a plan and decide nothing; only what depends on pointers stays with them.
#pragma once

#include "../../include/ggml_mi355x_qmm.h"
#include "qmm_types.h"

#include <cstddef>
#include <cstdio>

namespace qmm {

// what the decision reads from the context (prefill_rules() in qmm_prefill.hiph fills it from qmm_ctx)
struct PrefillRules {
    int     cus, prec;
    int     skinny, skinny_max_n, skinny_max_n_few;
    int     splitk, splitk_combine;
    int64_t kcnt_n;
    int     wide, r64, r64s, prep_reg, regb_q23, mm_group;
};

enum : unsigned { PF_GATHER = 1,      // MUL_MAT_ID: rows gathered per expert, scattered stores (N = the (token, slot) pairs)
                  PF_SWIGLU = 2,      // the prep forms silu(x) * x2 (qmm_mul_mat_swiglu_in)
                  PF_NORM   = 4 };    // the prep forms rms_norm(x [+ add]) * w (qmm_mul_mat_group_ex)

enum PrefillKernel { PK_NONE, PK_LDS_TILE, PK_SKINNY, PK_REGB, PK_WIDE, PK_R64_4, PK_R64_8, PK_R64S,
                     PK_Q8X };         // QMM_PREC_Q8_EXACT: mfma_q8x_kernel<T> (qmm_mfma_q8x.hiph)

struct PrefillPlan {
    // a run of 2..4 matrices that cannot be one launch: prefill_group_plan lists each matrix with a plan of its own (the first prepares
    // the operand); of this plan only the prep fields (the same for every matrix of a run: one key) and ws_total (the largest) count
    bool     per_matrix;
    // the MFMA launch.  ta / tb: mfma_kernel<T, ta>, mfma_skinny_kernel<T, ta, tb>, mfma_regb_kernel<T, ta, tb> (Q4_K: mfma_regb_q4k_kernel<ta, tb>)
    int      kernel, ta, tb;
    bool     f16;             // f16 MFMA on Q8-quantized activations (the kernels' and the prep's F16 argument), else bf16
    unsigned grid[3], block;
    size_t   lds;
    int      ksplit;          // > 1: K is split over this many workgroups per tile, partial tiles go to the slabs at o_part
    int      wide;            // 256-token tiles; ksplit then counts for 256 x 256 tiles
    int      frag_major;      // layout of the operand: 0 = rows of Kp, 1 = fragment-major (frag_major_chunk)
    int      tiles_x, n_tiles_y, mtot;
    bool     rows_vec4;       // every matrix has M % 4 == 0 (with aligned destinations: float4 stores in the reduce / combine)
    bool     combine_ok;      // the shapes allow split-K combined by the launch itself; the destination pointers decide the rest
    bool     reduce;          // splitk_reduce_kernel behind the launch (unless combined)
    char     label[48];
    // the activation prep
    int      act, perm;       // prep_act_kernel<act, f16, perm> / prep_act_q8k_kernel<perm, ...>
    bool     prep_reg;        // prep_act_q8k_kernel (registers) instead of prep_act_kernel (LDS staging)
    bool     prep_q8x;        // prep_act_q8x_kernel: the Q8_K rows themselves, int8 [N, K] at o_xh and d f32 [N, K / 256] at o_scale
    bool     prep_x2, prep_norm;   // the prep forms the SwiGLU product / the RMS norm (never for gathered rows)
    unsigned prep_grid, prep_block;
    size_t   prep_lds;
    int      prep_tpw;
    int      Kp, key;
    const char * unsupported; // the prep cannot do what the flags ask: the message
    char     prep_label[40];
    // workspace, bytes from the run's base
    size_t   o_xh, o_scale, o_part, o_gather, o_dst_off, o_seg_start, o_seg_count, o_n_live, ws_total;
};

inline int mfma_kpad(int64_t K) { return (int) ((K + 127) / 128 * 128); }
inline int mfma_npad(int64_t N) { return (int) ((N + 127) / 128 * 128); }

inline bool mfma_regb_supports(const PrefillRules & r, int type) {
    type = type_base(type);                                      // planar rows (Q4_0P / Q8_0P / Q6_KP) run the same kernels
    return r.prec == QMM_PREC_F16_Q8 && (type == T_Q4_K || type == T_Q5_K || type == T_Q6_K || type == T_Q4_0 || type == T_Q8_0 ||
                                         type == T_Q4_1 || type == T_Q5_0 || type == T_Q5_1 || type == T_IQ4_NL || type == T_IQ4_XS || ((type == T_Q2_K || type == T_Q3_K) && r.regb_q23));
}
// K elements per LDS stage of a type's kernels (MfmaBK, Regb<T>::BK)
constexpr int mfma_bk(int type) { return type_base(type) == T_Q6_K || type_base(type) == T_Q2_K || type_base(type) == T_Q3_K || type_base(type) == T_TQ2_0 ? 128 : 64; }

// k-order of the 16-bit operand (PERM of the prep kernels) from the weight type: the register-B lane orders (qmm_mfma_regb.hiph)
inline int prefill_perm(const PrefillRules & r, int type) {
    type = type_base(type);                                                  // planar rows: the same lane orders as their wire forms
    if (r.prec != QMM_PREC_F16_Q8) return 0;
    if (type == T_Q4_K || type == T_Q5_K) return 2;
    if (type == T_Q8_0) return 5;
    if (type == T_Q6_K || ((type == T_Q2_K || type == T_Q3_K) && r.regb_q23)) return 3;
    if (type == T_Q4_0 || type == T_Q4_1 || type == T_Q5_0 || type == T_Q5_1 || type == T_IQ4_NL || type == T_IQ4_XS) return 4;
    return 0;
}

// QMM_PREC_Q8_EXACT covers the K-quant formats whose sub-block scale is an integer that can go into the weight before the int8 MFMA
// (wire layout; planar Q6_K rows, every other type and MUL_MAT_ID run as in QMM_PREC_F16_Q8): the five K-quants and IQ4_XS, i.e. every
// type with a Q8xBlock (qmm_mfma_q8x.hiph)
inline bool q8x_supports(int type, int64_t K) {
    return (type == T_Q4_K || type == T_Q5_K || type == T_Q6_K || type == T_Q2_K || type == T_Q3_K || type == T_IQ4_XS) && K > 0 && K % 256 == 0;
}
// ... and the rules such a call, or any call of another mode, is planned by
inline PrefillRules prefill_effective_rules(PrefillRules r, int type, int64_t K, bool gather) {
    if (r.prec == QMM_PREC_Q8_EXACT && (gather || !q8x_supports(type, K))) r.prec = QMM_PREC_F16_Q8;
    return r;
}
constexpr int Q8X_ROWS = 128, Q8X_TOKENS = 64;      // tile of a workgroup of mfma_q8x_kernel: 4 waves of 32 rows each on the same 64 tokens
constexpr int Q8X_KEY  = 1;                         // one operand for all its formats (the other modes' keys are 0 or >= 6)

namespace plan_detail {

// few tokens: the split-K kernel of qmm_mfma_regb.hiph, which wants the operand fragment-major
// (measured on MI355X: it wins up to 64 tokens on any matrix, and up to 128 tokens on matrices of <= 8192 rows, which give
// the tiled kernels too few workgroups to fill the chip; from 129 tokens the tiled kernel with split-K is level or ahead)
inline bool mfma_use_skinny(const PrefillRules & r, int type, int64_t N, int64_t M, int64_t n_expert = 1) {
    if (!mfma_regb_supports(r, type) || !r.skinny) return false;
    return N <= r.skinny_max_n || (N <= r.skinny_max_n_few && (M + 31) / 32 * n_expert <= r.cus);
}

// Split-K factor for the tiled register-B kernel on a plain MUL_MAT.  One 256-row x 128-token tile over K = 4096 is 27 us
// of MFMA time on its CU however few tiles there are, and 4096 x 4096 at 512 tokens is only 64 tiles; K is therefore cut
// into ranges (one workgroup each, partial tiles to the workspace, splitk_reduce_kernel adds them) until the launch has
// about as many workgroups as the chip has CUs.  Each extra range costs one more N x M f32 slab to write and read.
// 256 x 256 tiles (mfma_regb_q4k_wide_kernel) for a launch of `row_tiles` 256-row tiles: only where they fill the chip as well as
// the 256 x 128 tiles do, i.e. the launch has at least 0.8 workgroups per CU without cutting K (ffn_gate + ffn_up of an 8B / 70B model as
// one launch).  Measured where that does not hold: 22016 rows (7B gate+up) are 172 tiles on 256 CUs, pp512 43.8k -> 39.4k; ffn_down
// with K cut 8 ways ties (76.4 vs 77.6 us) and doubles the reduce.
inline bool mfma_use_wide(const PrefillRules & r, int type, int64_t row_tiles, int64_t K, int64_t N) {
    if (!r.wide || type != T_Q4_K || r.prec != QMM_PREC_F16_Q8 || N < 256 || mfma_npad(N) % 256 || K % 256) return false;
    const int64_t tiles = row_tiles * ((N + 255) / 256);
    return tiles * 10 >= (int64_t) r.cus * 8;
}
// ... for a launch of `row_tiles` 256-row tiles (one matrix, or all matrices of a group)
inline int mfma_splitk(const PrefillRules & r, int64_t row_tiles, bool wide, int64_t K, int64_t N) {
    const int64_t tiles = row_tiles * (wide ? (N + 255) / 256 : (N + 127) / 128);
    if (!r.splitk || tiles * 10 >= (int64_t) r.cus * 8) return 1;
    int64_t s = r.cus / tiles;
    if (s > 8) s = 8;
    if (r.splitk > 1 && s > r.splitk) s = r.splitk;       // (GGML_MI355X_SPLITK=n caps the factor; for experiments)
    if (s > K / 512) s = K / 512;
    return s < 2 ? 1 : (int) s;
}

// the activation prep: format, k-order, kernel; and what the prepared operand depends on besides src1 itself (the key)
inline void plan_prep(PrefillPlan & p, const PrefillRules & r, int type, int64_t K, int64_t N, unsigned flags) {
    const bool f16 = r.prec == QMM_PREC_F16_Q8, gather = flags & PF_GATHER;
    const bool x2 = !gather && (flags & PF_SWIGLU), norm = !gather && (flags & PF_NORM);
    const int tb = type_base(type);
    p.f16 = f16;  p.prep_x2 = x2;  p.prep_norm = norm;
    p.act  = type_act(type) != T_Q8_K ? T_Q8_0 : T_Q8_K;     // Q8_1's int8 and d are Q8_0's; its s is implied in the GEMM by the weights' m
    p.perm = prefill_perm(r, type);
    p.Kp   = mfma_kpad(K);
    p.prep_grid = gather ? (unsigned) N : (unsigned) mfma_npad(N);
    p.prep_reg  = p.act == T_Q8_K && r.prep_reg && f16 && K % 1024 == 0 && p.Kp == K && K <= 32768 && tb != T_IQ4_XS;      // (IQ4_XS: PERM 4)
    p.unsupported = nullptr;
    if (x2 && !f16) p.unsupported = "SwiGLU input: only in the default (f16 on Q8 activations) prefill mode";
    if (p.prep_reg) {
        const int tasks = (int) (K / 1024), nw = tasks < 16 ? (tasks < 4 ? 4 : tasks) : 16;
        p.prep_tpw = (tasks + nw - 1) / nw;
        p.prep_block = nw * 64;
        p.prep_lds = 0;
        if (norm && (x2 || p.prep_tpw != 1)) p.unsupported = "prefill with a fused norm: K <= 16384, no SwiGLU input";
        snprintf(p.prep_label, sizeof(p.prep_label), norm ? "prep_act_q8k_kernel<%d,norm>" : "prep_act_q8k_kernel<%d>", p.perm);
    } else {
        p.prep_tpw = 0;
        p.prep_block = 256;
        p.prep_lds = f16 ? (size_t) K + (size_t) (K / 32) * 4 + 64 : 0;
        if (norm && !p.unsupported) p.unsupported = "prefill with a fused norm: Q8_K-activation formats with K % 1024 == 0 only";
        snprintf(p.prep_label, sizeof(p.prep_label), "prep_act_kernel<%d>", p.act);
    }
}
// activation format and k-order follow from the weight type (Q5_K shares Q4_K's); the layout from the kernel choice.
// Round 3: Q6_K's order (PERM 3, 128-blocks) is Q4_K's (PERM 2, 64-blocks) written out over two blocks: both put source group
// 8 (kk & 1) + 16 h + 32 (kk >> 1) at position 16 kk + 8 h, and the formula is 64-periodic.  Row-major operands of a K % 128 == 0
// row are therefore the same bytes, and attn_v in Q6_K beside attn_q / attn_k in Q4_K (half of Q4_K_M's layers) needs no prep of
// its own (7.5 us per such layer).  (Not the fragment-major layout of the few-token kernel, whose chunk index depends on the block.)
inline int plan_key(const PrefillRules & r, int type, int perm, bool skinny, int64_t K) {
    if (r.prec != QMM_PREC_F16_Q8) return 0;
    const bool as_q4k = type == T_Q5_K || (perm == 3 && !skinny && K > 0 && K % 128 == 0);
    return 2 * (1 + (as_q4k ? T_Q4_K : type_base(type))) + (skinny ? 1 : 0);
}

// which of the kernels and which tile, for a launch whose ksplit / wide / frag_major are set
inline void plan_kernel(PrefillPlan & p, const PrefillRules & r, int type, const int64_t * M, int n, int64_t N, int64_t n_expert, unsigned flags) {
    const int64_t M0 = M[0];
    const int nty = mfma_npad(N) / 128;                      // 128-token tiles of the (worst-case) token range
    int64_t tiles_x = 0, mtot = 0;
    p.rows_vec4 = true;
    for (int i = 0; i < n; ++i) { tiles_x += (M[i] + 255) / 256; mtot += M[i]; p.rows_vec4 = p.rows_vec4 && M[i] % 4 == 0; }
    p.tiles_x = (int) tiles_x;  p.n_tiles_y = nty;  p.mtot = (int) mtot;
    p.combine_ok = p.reduce = false;
    p.ta = p.tb = 0;
    auto set = [&](int kernel, int64_t gx, int64_t gy, int64_t gz, unsigned block, size_t lds) {
        p.kernel = kernel;  p.grid[0] = (unsigned) gx;  p.grid[1] = (unsigned) gy;  p.grid[2] = (unsigned) gz;  p.block = block;  p.lds = lds;
    };
    if (!mfma_regb_supports(r, type)) {
        // 64-row tiles when 128-row tiles would leave CUs idle
        const bool small = (int64_t) ((M0 + 127) / 128) * nty * n_expert < r.cus;
        p.ta = small ? 64 : 128;
        set(PK_LDS_TILE, (M0 + p.ta - 1) / p.ta, nty, n_expert, 512, (size_t) 2 * (p.ta + 128) * mfma_bk(type) * 2);
        snprintf(p.label, sizeof(p.label), "mfma_kernel<%d,%d>", type, p.ta);
        return;
    }
    // tile choice = chip fill: 256 rows x 128 tokens (8 waves, two per SIMD) when that gives (almost) every CU a workgroup,
    // else 128 x 128, else 128 x 64 / 128 x 32 (the weight unpack is then repeated 2x / 4x, on CUs that would otherwise idle).
    // n_tiles_y counts 128-token tiles of the (worst-case) token range.
    const int ksplit = p.ksplit = n_expert == 1 ? p.ksplit : 1;
    const int64_t wg_256 = tiles_x * nty * n_expert;
    const int64_t wg_128 = (int64_t) ((M0 + 127) / 128) * nty * n_expert;
    const bool tile_256 = n > 1 || ksplit > 1 || wg_256 * 10 >= (int64_t) r.cus * 8;
    const bool q4k_tiled = type == T_Q4_K && !p.frag_major && n_expert == 1;
    // split-K combined by the launch itself (splitk_finish_wave) where the 256 x 128 kernels run with <= 4 ranges and every store is a
    // whole, aligned float4: no splitk_reduce_kernel behind it
    p.combine_ok = ksplit > 1 && ksplit <= 4 && r.splitk_combine && !p.frag_major && !(flags & PF_GATHER) && n_expert == 1 && !p.wide &&
                   !(type == T_Q4_K && (r.r64 & 1)) && tiles_x * nty * 8 <= r.kcnt_n && p.rows_vec4 && N * mtot * 4 < ((int64_t) 1 << 32);
    p.reduce = ksplit > 1 && !p.frag_major;
    auto regb = [&](int nw, int bn, int rows, int ty) {
        p.ta = nw;  p.tb = bn;
        const size_t lds = (size_t) 2 * bn * mfma_bk(type) * 2;
        set(PK_REGB, n > 1 ? tiles_x : (M0 + rows - 1) / rows, ty, n_expert * ksplit, nw * 64, lds < 2048 ? 2048 : lds);
        snprintf(p.label, sizeof(p.label), "mfma_regb_kernel<%d,%d,%d>", type, nw, bn);
    };
    if (q4k_tiled && r.r64 >= 2 && p.wide) {
        set(r.r64s ? PK_R64S : PK_R64_8, tiles_x, (nty + 1) / 2, ksplit, 256, 0);
        snprintf(p.label, sizeof(p.label), r.r64s ? "mfma_r64s_q4k_kernel<2>" : "mfma_r64_q4k_kernel<8>");
    } else if (q4k_tiled && (r.r64 & 1) && !p.wide && tile_256) {
        set(PK_R64_4, tiles_x, nty, ksplit, 256, 0);
        snprintf(p.label, sizeof(p.label), "mfma_r64_q4k_kernel<4>");
    } else if (q4k_tiled && p.wide) {
        set(PK_WIDE, tiles_x, (nty + 1) / 2, ksplit, 512, (size_t) 2 * 256 * 64 * 2);
        snprintf(p.label, sizeof(p.label), "mfma_regb_q4k_wide_kernel<8>");
    } else if (p.frag_major) {
        p.ta = 8;  p.tb = N <= 32 ? 1 : 2;                   // (16 waves per group measured no better, Q6_K worse)
        set(PK_SKINNY, (M0 + 31) / 32, (N + 32 * p.tb - 1) / (32 * p.tb), n_expert, 8 * 64, 0);
        snprintf(p.label, sizeof(p.label), "mfma_skinny_kernel<%d,%d,%d>", type, p.ta, p.tb);
    }
    else if (tile_256)                                    regb(8, 128, 256, nty);
    else if (wg_128 >= r.cus && mfma_bk(type) != 128)     regb(4, 128, 128, nty);       // (Q6_K and the other 128-wide units: this shape spills, 4.5x slower)
    else if (2 * wg_128 >= r.cus / 2)                     regb(4, 64, 128, 2 * nty);
    else                                                  regb(4, 32, 128, 4 * nty);
}

// QMM_PREC_Q8_EXACT on a supported type: the Q8_K rows as they are (prep_act_q8x_kernel, four rows per workgroup), then one
// mfma_q8x_kernel<T> launch per matrix over 128-row x 64-token tiles.  No split-K, no LDS; a group is one launch per matrix on one prep.
inline PrefillPlan plan_q8x(int type, const int64_t * M, int n, int64_t K, int64_t N, unsigned flags) {
    PrefillPlan p = {};
    p.act = T_Q8_K;  p.Kp = (int) K;  p.key = Q8X_KEY;  p.ksplit = 1;  p.prep_q8x = true;
    p.prep_grid = (unsigned) ((N + 3) / 4);  p.prep_block = 256;
    snprintf(p.prep_label, sizeof(p.prep_label), "prep_act_q8x_kernel");
    if (flags & (PF_SWIGLU | PF_NORM)) p.unsupported = "SwiGLU input / fused norm: only in the default (f16 on Q8 activations) prefill mode";
    p.rows_vec4 = true;
    for (int i = 0; i < n; ++i) { p.tiles_x += (int) ((M[i] + Q8X_ROWS - 1) / Q8X_ROWS);  p.mtot += (int) M[i];  p.rows_vec4 = p.rows_vec4 && M[i] % 4 == 0; }
    p.n_tiles_y = (int) ((N + Q8X_TOKENS - 1) / Q8X_TOKENS);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t) 255; return o; };
    p.o_xh = take((size_t) N * K);  p.o_scale = take((size_t) N * (K / 256) * 4);  p.o_part = off;
    p.ws_total = off + 256;
    if (n > 1) { p.per_matrix = true;  p.kernel = PK_NONE;  return p; }
    p.kernel = PK_Q8X;  p.ta = type;
    p.grid[0] = (unsigned) p.tiles_x;  p.grid[1] = (unsigned) p.n_tiles_y;  p.grid[2] = 1;  p.block = 256;
    snprintf(p.label, sizeof(p.label), "mfma_q8x_kernel<%d>", type);
    return p;
}

} // namespace plan_detail

// the prep key of one matrix alone: prefill_group_plan cuts a group into runs of one type and one key
inline int prefill_prep_key(const PrefillRules & r0, int type, int64_t M, int64_t K, int64_t N) {
    const PrefillRules r = prefill_effective_rules(r0, type, K, false);
    if (r.prec == QMM_PREC_Q8_EXACT) return Q8X_KEY;
    return plan_detail::plan_key(r, type, prefill_perm(r, type), plan_detail::mfma_use_skinny(r, type, N, M), K);
}

// The plan for one run: n = 1..4 matrices of one weight type with M[i] rows on one src1 of N tokens (rows of K), or, with PF_GATHER,
// one expert tensor of n_expert matrices on N (token, slot) pairs.
// Plain MUL_MATs that share src1 and the weight type (attn_q / attn_k / attn_v at prefill): one launch of the tiled kernel
// over the row tiles of all of them and one reduce, instead of a launch (and, with split-K, a reduce) per matrix; the 1024-row
// matrices alone are 16 tiles each.  Falls back to one call per matrix where the few-token kernel or a smaller tile applies.
inline PrefillPlan prefill_plan(const PrefillRules & r0, int type, const int64_t * M, int n, int64_t K, int64_t N, int64_t n_expert, unsigned flags) {
    using namespace plan_detail;
    PrefillPlan p = {};
    const bool gather = flags & PF_GATHER;
    const PrefillRules r = prefill_effective_rules(r0, type, K, gather);
    if (r.prec == QMM_PREC_Q8_EXACT) return plan_q8x(type, M, n, K, N, flags);
    plan_prep(p, r, type, K, N, flags);
    const bool skinny = mfma_use_skinny(r, type, N, M[0], n_expert);
    p.key = gather ? 0 : prefill_prep_key(r, type, M[0], K, N);
    p.ksplit = 1;
    if (n > 1) {
        int64_t row_tiles = 0;
        for (int i = 0; i < n; ++i) row_tiles += (M[i] + 255) / 256;
        const bool may = n <= 4 && r.mm_group && N > r.skinny_max_n_few;
        p.wide   = may && mfma_use_wide(r, type, row_tiles, K, N);
        p.ksplit = mfma_splitk(r, row_tiles, p.wide, K, N);
        const int64_t tiles = row_tiles * (p.wide ? (N + 255) / 256 : (N + 127) / 128);
        p.per_matrix = !(may && mfma_regb_supports(r, type) && (p.ksplit > 1 || tiles * 10 >= (int64_t) r.cus * 8));
        if (p.per_matrix) {
            p.kernel = PK_NONE;
            for (int i = 0; i < n; ++i) {
                const size_t t = prefill_plan(r, type, M + i, 1, K, N, 1, flags).ws_total;
                if (t > p.ws_total) p.ws_total = t;
            }
            return p;
        }
    } else if (!gather) {
        p.frag_major = skinny;
        const bool wide = mfma_use_wide(r, type, (M[0] + 255) / 256, K, N);
        if (mfma_regb_supports(r, type) && !skinny) p.ksplit = mfma_splitk(r, (M[0] + 255) / 256, wide, K, N);
        p.wide = !skinny && wide;
    } else {
        p.frag_major = skinny;
    }
    plan_kernel(p, r, type, M, n, N, n_expert, flags);
    // workspace: the 16-bit operand, the row scales, then the split-K slabs (plain MUL_MAT) or the expert lists (MUL_MAT_ID)
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = (off + bytes + 255) & ~(size_t) 255; return o; };
    if (gather) {
        const size_t rows = (size_t) N + 128;
        p.o_xh = take(rows * p.Kp * 2);  p.o_scale = take(rows * 4);  p.o_gather = take((size_t) N * 8);  p.o_dst_off = take((size_t) N * 8);
        p.o_seg_start = take((size_t) n_expert * 4);  p.o_seg_count = take((size_t) n_expert * 4);  p.o_n_live = take(4);
        p.ws_total = off;
    } else {
        const size_t Np = (size_t) mfma_npad(N);
        p.o_xh = take(Np * p.Kp * 2);  p.o_scale = take(Np * 4);  p.o_part = off;
        p.ws_total = off + (p.ksplit > 1 ? (size_t) p.ksplit * N * p.mtot * sizeof(float) : 0) + 256;
    }
    return p;
}

// The launches of one plain MUL_MAT group call (nw matrices on one src1 of N > QMM_MATVEC_MAX_N tokens), in issue order on one stream.
// An entry is one MFMA launch (with its reduce) over matrices first .. first + n - 1 of the group, behind the activation prep of its
// plan when `prep` is set; otherwise it reads the operand the entry before it left in the workspace (same key = same bytes).
//   - matrices without rows are skipped;
//   - a run is up to 4 adjacent matrices of one type; if a member's prep key differs from the first's, the first matrix alone;
//   - a run whose plan is per_matrix becomes one entry per matrix, each planned alone with the same flags;
//   - an entry prepares unless the entry before it has its key (keys A, B, A: three preps; all entries share the workspace from its start);
//   - more than PREFILL_MAX_RUNS runs (counted before per_matrix runs expand) are refused: `error` is the message, nothing is listed.
// ws_total: the largest of the entries' plans, what the call needs before its first launch.
constexpr int PREFILL_MAX_RUNS = 8;
struct PrefillEntry { int first, n; bool prep; PrefillPlan plan; };
struct PrefillGroupPlan {
    int          n;
    size_t       ws_total;
    const char * error;
    PrefillEntry e[PREFILL_MAX_RUNS * 4];
};

inline void prefill_group_plan(PrefillGroupPlan & g, const PrefillRules & r, const qmm_weight * ws, int nw, int64_t K, int64_t N, unsigned flags) {
    g.n = 0;  g.ws_total = 0;  g.error = nullptr;
    int runs = 0, last_key = -1;
    auto add = [&](int first, int n, const PrefillPlan & p) {
        g.e[g.n++] = { first, n, p.key != last_key, p };
        last_key = p.key;
        if (p.ws_total > g.ws_total) g.ws_total = p.ws_total;
    };
    for (int i = 0; i < nw;) {
        if (ws[i].M == 0) { ++i; continue; }
        int64_t M[4] = { ws[i].M };
        const int key = prefill_prep_key(r, ws[i].type, ws[i].M, K, N);
        int j = i + 1;
        while (j < nw && j - i < 4 && ws[j].type == ws[i].type && ws[j].M > 0) { M[j - i] = ws[j].M; ++j; }
        for (int k = i + 1; k < j; ++k) if (prefill_prep_key(r, ws[k].type, ws[k].M, K, N) != key) j = i + 1;
        if (runs++ == PREFILL_MAX_RUNS) { g.n = 0;  g.ws_total = 0;  g.error = "too many runs in one group";  return; }
        const PrefillPlan p = prefill_plan(r, ws[i].type, M, j - i, K, N, 1, flags);
        if (!p.per_matrix) add(i, j - i, p);
        else for (int k = i; k < j; ++k) add(k, 1, prefill_plan(r, ws[i].type, M + (k - i), 1, K, N, 1, flags));
        i = j;
    }
}

} // namespace qmm
