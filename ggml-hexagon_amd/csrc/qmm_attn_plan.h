// qmm_attn_plan.h — the one launch plan of the attention launches (qmm_attn.hiph): which shapes the two families take, and for a
// shape and the two switches which of the five kernels (at the end of the file: which of the two for V with cache positions as rows,
// qmm_attn_rows.hiph) runs with which template arguments, grid, block and LDS bytes, whether
// the LDS limit of the kernel has to be raised, and for a cache cut into pieces their number, length, workspace and the merge
// launch.  Plain C++ (no HIP, no ggml; a host compiler alone reads it, like qmm_prefill_plan.h and qmm_matvec_plan.h).  The
// kernels take their tile constants from here; run_attn executes a plan and decides nothing.
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdio>

namespace qmm {

// attn_prefill_kernel: tokens per workgroup, K rows / V columns per tile, kv columns per chunk
constexpr int AP_TN = 64, AP_KT = 64, AP_CH = 512;

// ---------------------------------------------------------------------------------------------- shapes

// where the few-token and the prompt-batch family differ: the multiple n_kv comes in (also its least value) and the upper limits
struct AttnLimits {
    int     kv_step;
    int64_t D, Dv, n_kv, N;           // Dv 0: V rows as wide as K rows (Dv == D)
};
constexpr AttnLimits ATTN_DECODE_LIMITS  = { 8, 256, 1024, 16384, 8 };
constexpr AttnLimits ATTN_PREFILL_LIMITS = { 32, 128, 0, 1 << 20, 1 << 20 };

// q [D, N, H] on K [D, n_kv, Hk] and V^T [n_kv, Dv, Hk]: grouped-query heads, H a grid dimension
inline bool attn_shape_ok(const AttnLimits & l, int64_t D, int64_t Dv, int64_t n_kv, int64_t N, int64_t H, int64_t Hk) {
    if ((D != 64 && D != 128 && D != 256) || D > l.D) return false;
    if (l.Dv ? Dv < 1 || Dv > l.Dv : Dv != D) return false;
    if (Hk <= 0 || H % Hk || H > 65535) return false;
    return N >= 1 && N <= l.N && n_kv >= l.kv_step && n_kv % l.kv_step == 0 && n_kv <= l.n_kv;
}

// ---------------------------------------------------------------------------------------------- one launch

// GGML_MI355X_ATTN_SHORT=0: the general kernel at every n_kv; GGML_MI355X_ATTN_SPLIT=0: one workgroup per (head, token) at every n_kv (A/B runs)
struct AttnRules { bool short_on, split_on; };

enum AttnKernel { AK_SHORT,       // attn_decode_short_kernel<D, fresh, width>: scores and probabilities both in LDS, n_kv <= width
                  AK_GENERAL,     // attn_decode_kernel<D, fresh>
                  AK_SPLIT,       // attn_decode_split_kernel<D> over S pieces of the cache, then attn_combine_kernel
                  AK_PREFILL,     // attn_prefill_kernel<D>
                  AK_ROWS_DECODE,     // attn_rows_decode_kernel<D>: V rows are cache positions; a cut cache also runs attn_combine_kernel
                  AK_ROWS_PREFILL };  // attn_rows_prefill_kernel<D>

struct AttnPlan {
    int      kernel, D, width;    // width 0: the kernel has no such argument
    bool     fresh;               // the batch's own K / V rows come with the launch (qmm_attn_decode_rope)
    int      N;
    unsigned grid[3], block;
    size_t   lds;
    bool     lds_attr;            // lds is past the 64 KiB a kernel may ask for unasked: the executor raises the kernel's limit first
    int      S, chunk;            // AK_SPLIT, AK_ROWS_DECODE (S 0: one piece of chunk = n_kv): pieces per (head, token) and kv columns per piece, ...
    size_t   ws_bytes;            // ... (max, sum, output row) of each piece, f32
    unsigned grid2[2], block2;    // ... and the merge launch
    char     label[48], label2[24];
    bool     mask_f16;            // AK_ROWS_*: the mask holds f16 values (a kernel argument, not an instantiation)
};

// N <= 8 tokens of H heads on a cache of n_kv columns; fresh: D <= 128 (qmm_attn_decode_rope_supported)
inline AttnPlan attn_decode_plan(const AttnRules & r, int D, int Dv, int n_kv, int N, int H, bool fresh) {
    AttnPlan p = {};
    p.D = D;  p.fresh = fresh;  p.N = N;
    p.grid[0] = (unsigned) H;  p.grid[1] = (unsigned) N;  p.grid[2] = 1;  p.block = 1024;
    // fresh rows: the roped q row in f32, then the N new K rows and the N new V rows in f16
    const size_t fresh_bytes = fresh ? (size_t) D * 4 + (size_t) N * (D + Dv) * 2 : 0;
    const char * const fr = fresh ? "true" : "false";
    if (!fresh && r.split_on && n_kv >= 1024 && D <= 128) {
        // kv range over S workgroups per (head, token), then the merge (long caches: one workgroup per head is latency-bound)
        p.kernel = AK_SPLIT;
        p.S = n_kv / 256 < 16 ? n_kv / 256 : 16;
        p.chunk = ((n_kv + p.S - 1) / p.S + 7) / 8 * 8;
        p.ws_bytes = (size_t) H * N * p.S * (Dv + 2) * sizeof(float);
        p.grid[2] = (unsigned) p.S;
        p.lds = (size_t) p.chunk * 4;
        p.grid2[0] = (unsigned) H;  p.grid2[1] = (unsigned) N;  p.block2 = 256;
        snprintf(p.label, sizeof(p.label), "attn_decode_split_kernel<%d>", D);
        snprintf(p.label2, sizeof(p.label2), "attn_combine_kernel");
    } else if (r.short_on && n_kv <= 1024 && D <= 128 && Dv <= 128) {
        p.kernel = AK_SHORT;
        p.width = n_kv <= 256 ? 256 : n_kv <= 512 ? 512 : 1024;
        p.lds = (size_t) n_kv * 8 + fresh_bytes;
        snprintf(p.label, sizeof(p.label), "attn_decode_short_kernel<%d,%s,%d>", D, fr, p.width);
    } else {
        p.kernel = AK_GENERAL;
        p.lds = (size_t) n_kv * 4 + fresh_bytes;
        snprintf(p.label, sizeof(p.label), "attn_decode_kernel<%d,%s>", D, fr);
    }
    p.lds_attr = p.lds > 64 * 1024;
    return p;
}

// a prompt batch: one workgroup per (AP_TN tokens, head); the score rows of a chunk, then a tile that holds
// 64 K rows of D + 8 halves and later D V^T rows of 64 + 8 halves, D <= 128
inline AttnPlan attn_prefill_plan(int D, int n_kv, int N, int H) {
    AttnPlan p = {};
    p.kernel = AK_PREFILL;  p.D = D;  p.N = N;
    p.grid[0] = (unsigned) ((N + AP_TN - 1) / AP_TN);  p.grid[1] = (unsigned) H;  p.grid[2] = 1;  p.block = 256;
    p.lds = (size_t) AP_TN * ((n_kv < AP_CH ? n_kv : AP_CH) + 4) * 4 + (size_t) 128 * (AP_KT + 8) * 2;
    p.lds_attr = p.lds > 64 * 1024;
    snprintf(p.label, sizeof(p.label), "attn_prefill_kernel<%d>", D);
    return p;
}

// ---------------------------------------------------------------------------------------------- V with cache positions as rows
// The operands of GGML_OP_FLASH_ATTN_EXT (QMM_TENSOR_KV_ROWS on v, include/ggml_mi355x_ops.h): V is [Dv, n_kv, Hk], strided like K,
// and the mask may be f16.  Two kernels of their own beside the ones above (whose plans and bits stay as they are); D = Dv in
// {64, 128}; n_kv in whole K tiles of the prompt kernel (llama.cpp pads the cache to 256 with flash attention).
constexpr AttnLimits ATTN_ROWS_DECODE_LIMITS  = { AP_KT, 128, 0, 16384, 8 };
constexpr AttnLimits ATTN_ROWS_PREFILL_LIMITS = { AP_KT, 128, 0, 1 << 20, 1 << 20 };

// N <= 8 tokens: attn_rows_decode_kernel<D>, one workgroup of 16 waves per (head, token) and, from 1024 cache rows on (as the cut of
// attn_decode_plan), per piece of the cache, merged by attn_combine_kernel.  LDS: the piece's scores, then one row of D partial sums per wave.
inline AttnPlan attn_rows_decode_plan(const AttnRules & r, int D, int n_kv, int N, int H, bool mask_f16) {
    AttnPlan p = {};
    p.kernel = AK_ROWS_DECODE;  p.D = D;  p.N = N;  p.mask_f16 = mask_f16;
    p.grid[0] = (unsigned) H;  p.grid[1] = (unsigned) N;  p.grid[2] = 1;  p.block = 1024;
    p.chunk = n_kv;
    if (r.split_on && n_kv >= 1024) {
        p.S = n_kv / 256 < 16 ? n_kv / 256 : 16;
        p.chunk = ((n_kv + p.S - 1) / p.S + 7) / 8 * 8;
        p.ws_bytes = (size_t) H * N * p.S * (D + 2) * sizeof(float);
        p.grid[2] = (unsigned) p.S;
        p.grid2[0] = (unsigned) H;  p.grid2[1] = (unsigned) N;  p.block2 = 256;
        snprintf(p.label2, sizeof(p.label2), "attn_combine_kernel");
    }
    p.lds = (size_t) p.chunk * 4 + (size_t) 16 * D * 4;
    p.lds_attr = p.lds > 64 * 1024;
    snprintf(p.label, sizeof(p.label), "attn_rows_decode_kernel<%d>", D);
    return p;
}

// a prompt batch: attn_rows_prefill_kernel<D>, the grid and the LDS image of attn_prefill_plan (the V tile is transposed on its way into LDS)
inline AttnPlan attn_rows_prefill_plan(int D, int n_kv, int N, int H, bool mask_f16) {
    AttnPlan p = attn_prefill_plan(D, n_kv, N, H);
    p.kernel = AK_ROWS_PREFILL;  p.mask_f16 = mask_f16;
    snprintf(p.label, sizeof(p.label), "attn_rows_prefill_kernel<%d>", D);
    return p;
}

} // namespace qmm
