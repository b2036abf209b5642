// qmm_bf16_plan.h — the one launch plan of MUL_MAT on BF16 weights (GGML_TYPE_BF16 = 30, kernels in qmm_bf16.hiph): which calls the
// two kernels take (the surface), and for a shape which kernel runs with which template arguments, grid, block and LDS bytes, how
// the tokens of a few-token call are cut into launches, the split-K factor with its workspace, and the trace label.  Plain C++ (no
// HIP, no ggml; a host compiler alone reads it, like qmm_attn_plan.h).  The kernels take their tile constants from here; run_bf16
// (qmm_bf16.hiph) executes a plan and decides nothing.
//
// Arithmetic of both kernels, the CPU backend's (vec_dot_type of BF16 is BF16, ggml_vec_dot_bf16): src1 rounded to bf16 (nearest
// even, subnormals kept), the weights' 16 bits as they are, products and sums in f32.  No precision or activation mode enters.
#pragma once

#include "../../include/ggml_mi355x_qmm.h"

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace qmm {

constexpr int T_BF16 = 30;                                   // ggml's enum value; not a member of the quantized type table (type_known)
constexpr int BF16_K_STEP = 32;                              // K comes in whole K-steps of the MFMA kernel
constexpr int BF16_MAX_GROUP = 4;                            // matrices of one mat-vec launch (MV_MAX_GROUP)

// ---------------------------------------------------------------------------------------------- the surface

inline size_t bf16_row_size(int64_t K) { return K > 0 && K % BF16_K_STEP == 0 ? (size_t) K * 2 : 0; }

// what every matrix of a call has to satisfy; nullptr, or why the call is refused
inline const char * bf16_weight_refusal(const void * w, int64_t w_row_bytes, int64_t K, int64_t M, int64_t ldd) {
    if (K <= 0 || K % BF16_K_STEP) return "BF16 weights: K must be a multiple of 32";
    if (K > INT32_MAX || M > INT32_MAX) return "BF16 weights: K and M must fit 31 bits";
    if (w_row_bytes < K * 2) return "BF16 weights: weight row stride < row size";
    if ((uintptr_t) w % 16 || w_row_bytes % 16) return "BF16 weights: rows must start on 16-byte boundaries (base and row stride)";
    if (M < 0 || ldd < M) return "BF16 weights: ldd < M";
    return nullptr;
}
// ... and src1, by the rules of the quantized types
inline const char * bf16_src1_refusal(const float * x, int64_t K, int64_t N, int64_t ldx) {
    if ((uintptr_t) x % 16 || ldx % 4 || ldx < K) return "BF16 weights: src1 must be 16-byte aligned with ldx % 4 == 0 and ldx >= K";
    if (N > (int64_t) 65535 * 64) return "BF16 weights: more tokens than the grid of one launch holds";
    return nullptr;
}

// ---------------------------------------------------------------------------------------------- few tokens: the streaming mat-vec

// bf16_matvec_kernel<NT, STAGED>: a workgroup rounds NT rows of src1 to bf16 once and keeps them in LDS; each wave then streams whole
// weight rows, 16 bytes (8 weights) per lane and load, BF16_MV_LOADS independent loads in flight per lane.
constexpr int    BF16_MV_LOADS = 4;
// the staged rows of one launch.  Eight tokens of K = 4096 fit (64 KiB); eight of K = 14336 (224 KiB) do not fit a CU's LDS at all
// and go out as two launches of four.  One row beyond the budget (K > 65536) is not staged: each lane rounds the values it needs.
constexpr size_t BF16_MV_STAGE_BYTES = (size_t) 128 * 1024;
constexpr size_t BF16_LDS_UNASKED = (size_t) 64 * 1024;      // what a kernel may ask for without its limit being raised

struct Bf16MvLaunch {
    int      n0, ntok;            // tokens n0 .. n0 + ntok - 1
    bool     staged;
    size_t   lds;
    bool     lds_attr;            // lds is past BF16_LDS_UNASKED: the executor raises the kernel's limit first
    unsigned blocks, block;
    char     label[40];
};
struct Bf16MvPlan {
    int          n;
    Bf16MvLaunch launch[QMM_MATVEC_MAX_N];
};

// rows: the rows of all matrices of the launch together; N <= QMM_MATVEC_MAX_N tokens of K
inline Bf16MvPlan bf16_matvec_plan(int cus, int64_t rows, int64_t K, int64_t N) {
    Bf16MvPlan p = {};
    int64_t at_once = (int64_t) (BF16_MV_STAGE_BYTES / ((size_t) K * 2));
    const bool staged = at_once >= 1;
    if (at_once > N) at_once = N;
    if (!staged) at_once = 1;
    // one workgroup per CU at the most (the rows are staged once per workgroup), 16 waves unless a CU has fewer rows than that
    const int64_t per_cu = (rows + cus - 1) / cus;
    const int waves = per_cu > 8 ? 16 : per_cu > 4 ? 8 : 4;
    int64_t blocks = (rows + waves - 1) / waves;
    if (blocks > cus) blocks = cus;
    if (blocks < 1) blocks = 1;
    for (int64_t n0 = 0; n0 < N; n0 += at_once) {
        Bf16MvLaunch & l = p.launch[p.n++];
        l.n0 = (int) n0;  l.ntok = (int) (N - n0 < at_once ? N - n0 : at_once);
        l.staged = staged;
        l.lds = staged ? (size_t) l.ntok * K * 2 : 0;
        l.lds_attr = l.lds > BF16_LDS_UNASKED;
        l.blocks = (unsigned) blocks;  l.block = (unsigned) waves * 64;
        snprintf(l.label, sizeof(l.label), "bf16_matvec_kernel<%d,%s>", l.ntok, staged ? "true" : "false");
    }
    return p;
}

// ---------------------------------------------------------------------------------------------- prompt batches: bf16 MFMA

// bf16_mfma_kernel<TILE>: a workgroup of 4 waves owns TILE weight rows x TILE tokens; both operands go through LDS as bf16 in
// BF16_K_STEP-deep steps (src1 rounded on its way in), two buffers so that the next step's global loads run under the MFMAs.
// LDS rows are BF16_MM_LD elements apart (80 bytes: the 16-byte fragment reads of 32 rows spread over all banks).
constexpr int BF16_MM_LD = BF16_K_STEP + 8;
constexpr size_t bf16_mm_lds(int tile) { return (size_t) 2 * 2 * tile * BF16_MM_LD * 2; }     // buffers x operands x rows x pitch x 2 B

struct Bf16MmPlan {
    int      tile;                // 64: one 32 x 32 MFMA tile per wave; 128: 2 x 2 of them, where 128 x 128 tiles still give every CU one
    unsigned grid[2], block;      // x: row tiles, y: token tiles
    size_t   lds;                 // static in the kernel; here for the record
    int      ksplit;              // always 1: every output element is one workgroup's sum over K in k order ...
    size_t   ws_bytes;            // ... so there is no workspace and nothing to reduce
    char     label[32];
};

inline Bf16MmPlan bf16_mfma_plan(int cus, int64_t M, int64_t N) {
    Bf16MmPlan p = {};
    // the large tile reads LDS half as often per MFMA, but a grid that leaves CUs idle costs more than that: 4096 rows x 512 tokens are
    // 128 large tiles on 256 CUs (measured 93 TFLOP/s) against 512 small ones
    p.tile = M > 64 && N > 64 && ((M + 127) / 128) * ((N + 127) / 128) >= cus ? 128 : 64;
    p.grid[0] = (unsigned) ((M + p.tile - 1) / p.tile);  p.grid[1] = (unsigned) ((N + p.tile - 1) / p.tile);
    p.block = 256;
    p.lds = bf16_mm_lds(p.tile);
    p.ksplit = 1;  p.ws_bytes = 0;
    snprintf(p.label, sizeof(p.label), "bf16_mfma_kernel<%d>", p.tile);
    return p;
}

} // namespace qmm
