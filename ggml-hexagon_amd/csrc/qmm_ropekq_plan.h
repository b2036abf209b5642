// qmm_ropekq_plan.h — the launch plan of qmm_rope_kq_store (qmm_ropekq.hiph): rope(q), rope(k) quantized straight into a K cache of Q8_0,
// Q4_0, Q4_1, Q5_0 or Q5_1 blocks, and v into the F16 V cache, as one launch (what qmm_rope_kv_store is on an F16 K cache; on a quantized
// one the same work was qmm_rope_kv_store(q, v), ROPE(k) and CPY f32 -> type).  Which operands the entry point takes, and for operands it
// takes the kernel's template arguments, grid, block and LDS bytes, under which trace label.  Plain C++ (no HIP, no ggml; a host compiler
// alone reads it), built on qmm_glue_plan.h (sup_rope, sup_rope_kv_store's q and v rules, glue_rope_kv_store_plan's q and v index spaces),
// qmm_kcache_plan.h and qmm_kblk_plan.h (the block layouts and their contiguity), whose tables stay as they are.  The kernel takes its
// constants from here; the host side in qmm_ropekq.hiph executes a plan and decides nothing.
// An F16 k_dst is qmm_rope_kv_store's; IQ4_NL, a quantized V and the one-launch rope + store + attention are outside this surface.
#pragma once

#include "qmm_kblk_plan.h"

namespace qmm {

// A workgroup of the K part stages one token's roped K (H_kv heads of D f32 values) in LDS before it cuts it into blocks: at most this many
// values, 32 KiB, which with the v part's tile stays inside the 64 KiB a kernel may use unasked (llama3-8b / 70b and mixtral: 1024;
// D = 256 with 32 kv heads: 8192)
constexpr int64_t ROPEKQ_MAX_ROW = 8192;
constexpr unsigned ROPEKQ_BLOCK = 256;

constexpr bool ropekq_code(int type) { return type == G_Q8_0 || kblk_code(type); }
constexpr int  ropekq_block(int type) { return type == G_Q8_0 ? KQ8_BLOCK : kblk_block(type); }
inline const char * ropekq_name(int type) { return type == G_Q8_0 ? "q8_0" : kblk_name(type); }

// qmm_rope_kq_store_supported.  q, pos, ff, q_dst and the optional v / v_dst: what sup_rope_kv_store takes without a k pair.  k: f32
// [D, H_kv, N] in rows of whole blocks, dense, on 4-byte boundaries, agreeing with q in ne[0], ne[2] and ne[3]; k_dst: one of the five
// block types, k's extents, contiguous in its blocks, on a 2-byte boundary
inline bool ropekq_takes_store(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst, const qmm_tensor * k,
                              const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst) {
    if (!k || !k_dst || !ropekq_code(k_dst->type)) return false;
    if (!sup_rope_kv_store(q, pos, ff, q_dst, nullptr, nullptr, v, v_dst)) return false;
    if (k->type != G_F32 || !same_shape(k, k_dst) || nelements(k) <= 0 || !fits_u32(k)) return false;
    if (k->ne[0] % KQ8_QK || k->nb[0] != 4 || !strides_aligned(k, 4) || !data_aligned(k, 4)) return false;
    if (k->ne[0] != q->ne[0] || k->ne[2] != q->ne[2] || k->ne[3] != q->ne[3]) return false;
    if (!(k_dst->type == G_Q8_0 ? kq8_contiguous(k_dst) : kblk_contiguous(k_dst)) || !data_aligned(k_dst, 2)) return false;
    if (k->ne[0] * k->ne[1] > ROPEKQ_MAX_ROW) return false;
    return nelements(q) / 2 + nelements(k) / 2 + (v ? nelements(v) : 0) < ((int64_t) 1 << 31);
}

// rope_kq_store_kernel<T, VT>: the grid is the concatenation of
//   q_blocks  rope_pair_heads<float> over q, a thread per (pair, ROPE_HC heads, token) as in rope_store_kernel
//   k_blocks  one workgroup per token of k: its H_kv x D values roped into LDS, then cut into blocks
//   v_blocks  VT: one 32 x 32 tile each (v is a 2-D transpose large enough for tiles); otherwise an element per thread
struct RopeKqPlan {
    int      type;                // k_dst's block type
    bool     vt;
    unsigned grid, block;
    unsigned q_blocks, k_blocks, v_blocks, tiles0;      // tiles0: VT, tiles along v's ne0
    size_t   lds;                 // dynamic: the staged token
    char     label[48];
};

inline RopeKqPlan rope_kq_store_plan(const qmm_tensor * q, const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst) {
    RopeKqPlan p = {};
    p.type = k_dst->type;  p.block = ROPEKQ_BLOCK;
    p.q_blocks = (rope_heads_threads(q) + ROPEKQ_BLOCK - 1) / ROPEKQ_BLOCK;
    p.k_blocks = (unsigned) (k->ne[2] * k->ne[3]);
    if (v && transpose_2d(v, v_dst, 32)) {
        p.vt = true;
        p.tiles0 = (unsigned) ((v->ne[0] + 31) / 32);
        p.v_blocks = p.tiles0 * (unsigned) ((v->ne[1] + 31) / 32);
    } else if (v) {
        p.v_blocks = ((unsigned) nelements(v) + ROPEKQ_BLOCK - 1) / ROPEKQ_BLOCK;
    }
    p.grid = p.q_blocks + p.k_blocks + p.v_blocks;
    p.lds = (size_t) (k->ne[0] * k->ne[1]) * sizeof(float);
    snprintf(p.label, sizeof(p.label), "rope_kq_store_kernel<%s,%s>", ropekq_name(p.type), p.vt ? "true" : "false");
    return p;
}

} // namespace qmm
