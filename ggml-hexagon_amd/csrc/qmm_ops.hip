// qmm_ops.hip — the per-layer glue ops around the quantized MUL_MAT path (include/ggml_mi355x_ops.h).
// gfx950 only, no CPU path.  Every kernel is HBM-bound elementwise / row work except the small F16 attention matmuls,
// which run on v_mfma_f32_32x32x16_f16.  Semantics follow the ggml CPU backend; each kernel cites the function it restates.
// Parity: the reference's tests/test-backend-ops.cpp (built unmodified into oracle/_ref) against the CPU backend.
// The file holds the kernels, run_glue and the C entry points.  Which operands an entry point takes, and for operands it takes which
// kernel runs with which template arguments, grid, block, LDS bytes and trace label, is decided by qmm_glue_plan.h; run_glue launches
// a plan and decides nothing; an entry point is its context check, the support predicate, the chain flush, the plan and the run.
// The attention launches (AttnArgs, AttnFresh, the five attn_* kernels, qmm_attn_decode / _decode_rope / _prefill and their
// _supported predicates) are a section of their own, qmm_attn.hiph, included below in front of the entry points; what they launch
// for a shape is decided by qmm_attn_plan.h.  What a Q8_0 K cache adds (CPY into and out of block_q8_0 rows, attention on them) is the
// section behind it, qmm_kcache.hiph, decided by qmm_kcache_plan.h: QMM_OP_CPY and the attention entry points branch there first; a K cache
// in Q4_0 / Q4_1 / Q5_0 / Q5_1 is the section behind that one, qmm_kblk.hiph (qmm_kblk_plan.h), reached the same way.

#include "qmm_host.h"
#include "qmm_glue_plan.h"
#include "qmm_device.hiph"

#include <hip/hip_fp16.h>
#include <cmath>

using namespace qmm;

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef float    f32x16v __attribute__((ext_vector_type(16)));

struct Shape {           // extents and byte strides of one operand
    int64_t ne[4];
    int64_t nb[4];
};
Shape shape_of(const qmm_tensor * t) {
    Shape s;
    for (int i = 0; i < 4; ++i) { s.ne[i] = t->ne[i]; s.nb[i] = t->nb[i]; }
    return s;
}

// wave_sum / wave_max: the DPP reductions of qmm_device.hiph (no LDS-permute traffic; the __shfl_xor butterflies this file began
// with cost ~0.3 us per reduction: 16 us of the 37 us of attn_prefill_kernel's last token tile were its per-row soft-max)
// sum over an aligned group of 8 lanes, result in all 8
__device__ __forceinline__ float sum8(float v) {
    v += dpp_mov<DPP_QUAD_X1>(v);
    v += dpp_mov<DPP_QUAD_X2>(v);
    v += dpp_mov<DPP_ROW_HALF_MIRROR>(v);
    return v;
}
// block-wide reductions (up to 16 waves) through 16 floats of LDS
template <bool MAX> __device__ __forceinline__ float block_reduce(float v, float * red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    const int nw = blockDim.x >> 6;
    float r = red[0];
    for (int i = 1; i < nw; ++i) r = MAX ? fmaxf(r, red[i]) : r + red[i];
    return r;
}

// 1 / sqrt(mean of squares + eps) of a row from the threads' partial sums, for the RMS-norm kernels: block_reduce's partial sums and order
// of additions; with 16 waves (four to a SIMD) the scalar tail (the wave sums out of LDS, two IEEE divisions, a square root: ~150
// dependent instructions) is run by wave 0 alone and handed over through LDS: run by every wave it cost ~1 us of the ~4.7 us launch
// (round 3, the same finding as in the mat-vec staging: profiles/tools/ex_times.py).  `red` holds 17 floats.
template <int NT> __device__ __forceinline__ float rms_scale_block(float sum, float * red, const float ne0, const float eps) {
    sum = wave_sum(sum);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (NT <= 512) {
        float r = red[0];
        for (int i = 1; i < NT / 64; ++i) r += red[i];
        return 1.0f / sqrtf(r / ne0 + eps);
    }
    if (threadIdx.x < 64) {
        float r = red[0];
        for (int i = 1; i < NT / 64; ++i) r += red[i];
        const float sc = 1.0f / sqrtf(r / ne0 + eps);
        if (threadIdx.x == 0) red[16] = sc;
    }
    __syncthreads();
    return red[16];
}

// row index -> byte offset of the row in a (possibly broadcast) operand
__device__ __forceinline__ void row_coords(uint32_t row, uint32_t ne1, uint32_t ne2, uint32_t & i1, uint32_t & i2, uint32_t & i3) {
    i1 = row % ne1;
    const uint32_t t = row / ne1;
    i2 = t % ne2;
    i3 = t / ne2;
}

// ------------------------------------------------------------------------------------------------ binary ops
// ggml_compute_forward_add/sub/mul/div (ggml-cpu/binary-ops.cpp; the DSP copy of add: kernels/ggml-dsp.c:991-1066):
// dst[i] = src0[i] op src1[i mod ne1x], src1 broadcast over every dimension it is smaller in.
template <int OP> __device__ __forceinline__ float bin(float a, float b) {
    return OP == QMM_OP_ADD ? a + b : OP == QMM_OP_SUB ? a - b : OP == QMM_OP_MUL ? a * b : a / b;
}

// one block per group of rows; vector path when every row is 16-byte aligned and src1 has full rows
template <int OP, bool VEC>
__global__ void __launch_bounds__(256)
binary_kernel(const char * __restrict__ a, const char * __restrict__ b, char * __restrict__ d, const Shape sa, const Shape sb,
              const Shape sd, const uint32_t rows) {
    const uint32_t ne0 = (uint32_t) sd.ne[0];
    const uint32_t per_row = VEC ? ne0 / 4 : ne0;
    const uint32_t rpb = per_row >= 256 ? 1 : 256 / per_row;          // rows per block for short rows
    const uint32_t tpr = per_row >= 256 ? 256 : per_row;              // threads per row
    const uint32_t lr = threadIdx.x / tpr;
    if (lr >= rpb) return;
    const uint32_t row = blockIdx.x * rpb + lr;
    if (row >= rows) return;
    uint32_t i1, i2, i3;
    row_coords(row, (uint32_t) sd.ne[1], (uint32_t) sd.ne[2], i1, i2, i3);
    const char * pa = a + i1 * sa.nb[1] + i2 * sa.nb[2] + i3 * sa.nb[3];
    const char * pb = b + (i1 % (uint32_t) sb.ne[1]) * sb.nb[1] + (i2 % (uint32_t) sb.ne[2]) * sb.nb[2] + (i3 % (uint32_t) sb.ne[3]) * sb.nb[3];
    char *       pd = d + i1 * sd.nb[1] + i2 * sd.nb[2] + i3 * sd.nb[3];
    for (uint32_t i = threadIdx.x % tpr; i < per_row; i += tpr) {
        if (VEC) {
            const float4 x = ((const float4 *) pa)[i], y = ((const float4 *) pb)[i];
            ((float4 *) pd)[i] = make_float4(bin<OP>(x.x, y.x), bin<OP>(x.y, y.y), bin<OP>(x.z, y.z), bin<OP>(x.w, y.w));
        } else {
            const float y = *(const float *) (pb + (i % (uint32_t) sb.ne[0]) * sb.nb[0]);
            ((float *) pd)[i] = bin<OP>(((const float *) pa)[i], y);
        }
    }
}

// ------------------------------------------------------------------------------------------------ unary / scale
template <int OP> __device__ __forceinline__ float una(float x, float p) {
    switch (OP) {
        case QMM_OP_SCALE:      return x * p;                                            // ggml_vec_scale_f32
        case QMM_OP_SILU:       return x / (1.0f + expf(-x));                            // ggml_silu_f32 (ggml-cpu.c)
        case QMM_OP_GELU:       return 0.5f * x * (1.0f + tanhf(0.79788456080286535587989211986876f * x * (1.0f + 0.044715f * x * x)));
        case QMM_OP_GELU_QUICK: return x * (1.0f / (1.0f + expf(-1.702f * x)));
        case QMM_OP_RELU:       return x > 0.0f ? x : 0.0f;
        case QMM_OP_TANH:       return tanhf(x);
        case QMM_OP_SIGMOID:    return 1.0f / (1.0f + expf(-x));
        case QMM_OP_NEG:        return -x;
        case QMM_OP_EXP:        return expf(x);
        default:                return x;
    }
}
// contiguous f32; MUL2: dst = f(a) * b (SwiGLU: silu(gate) * up, the two nodes build_ffn emits back to back)
template <int OP, bool MUL2>
__global__ void __launch_bounds__(256)
unary_kernel(const float * __restrict__ a, const float * __restrict__ b, float * __restrict__ d, const uint32_t n, const float p) {
    const uint32_t i4 = (blockIdx.x * 256u + threadIdx.x) * 4u;
    if (i4 + 3 < n && (((uintptr_t) a | (uintptr_t) d | (uintptr_t) b) & 15) == 0) {
        const float4 x = *(const float4 *) (a + i4);
        float4 r = make_float4(una<OP>(x.x, p), una<OP>(x.y, p), una<OP>(x.z, p), una<OP>(x.w, p));
        if (MUL2) {
            const float4 y = *(const float4 *) (b + i4);
            r.x *= y.x; r.y *= y.y; r.z *= y.z; r.w *= y.w;
        }
        *(float4 *) (d + i4) = r;
    } else {
        for (uint32_t i = i4; i < n && i < i4 + 4; ++i) d[i] = una<OP>(a[i], p) * (MUL2 ? b[i] : 1.0f);
    }
}

// ------------------------------------------------------------------------------------------------ RMS_NORM
// ggml_compute_forward_rms_norm_f32 (ggml-cpu.c:6254-6300): mean of squares over the row, y = x / sqrt(mean + eps).
// One block per row; the row stays in registers (<= 8 values per thread) or is re-read from L2.
// MUL: y *= w[i0] — the norm weight ggml_mul of build_norm, fused when the plugin sees the pair.
template <bool MUL>
__global__ void __launch_bounds__(256)
rms_norm_kernel(const char * __restrict__ x, const float * __restrict__ w, char * __restrict__ y, const Shape sx, const Shape sy, const float eps) {
    __shared__ float red[4];
    uint32_t i1, i2, i3;
    row_coords(blockIdx.x, (uint32_t) sx.ne[1], (uint32_t) sx.ne[2], i1, i2, i3);
    const float * px = (const float *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
    float *       py = (float *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]);
    const uint32_t n = (uint32_t) sx.ne[0];
    float keep[8];
    float sum = 0.0f;
    const bool in_regs = n <= 256 * 8;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const uint32_t i = threadIdx.x + j * 256;
        keep[j] = in_regs && i < n ? px[i] : 0.0f;
        sum += keep[j] * keep[j];
    }
    if (!in_regs)
        for (uint32_t i = threadIdx.x; i < n; i += 256) sum += px[i] * px[i];
    sum = block_reduce<false>(sum, red);
    const float scale = 1.0f / sqrtf(sum / (float) n + eps);
    if (in_regs) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const uint32_t i = threadIdx.x + j * 256;
            if (i < n) py[i] = MUL ? keep[j] * scale * w[i] : keep[j] * scale;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < n; i += 256) py[i] = MUL ? px[i] * scale * w[i] : px[i] * scale;
    }
}

// ggml_compute_forward_norm_f32 (ggml-cpu.c:6183-6232), the LayerNorm of GPT-2 / Falcon / Phi-style models: mean over the row,
// then the variance of the centred values, y = (x - mean) / sqrt(var + eps).  One block per row, four passes over L2.
__global__ void __launch_bounds__(256)
norm_kernel(const char * __restrict__ x, char * __restrict__ y, const Shape sx, const Shape sy, const float eps) {
    __shared__ float red[4];
    uint32_t i1, i2, i3;
    row_coords(blockIdx.x, (uint32_t) sx.ne[1], (uint32_t) sx.ne[2], i1, i2, i3);
    const float * px = (const float *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
    float *       py = (float *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]);
    const uint32_t n = (uint32_t) sx.ne[0];
    float sum = 0.0f;
    for (uint32_t i = threadIdx.x; i < n; i += 256) sum += px[i];
    float mean = block_reduce<false>(sum, red) / (float) n;
    // the CPU takes this sum in double.  One f32 sum of n values near m is good to about n ulp(n m): for a row with a mean far from zero
    // (|mean| / sigma ~ 1000) that is 1e-4 of sigma and more, which after centring is the signal.  A second pass adds the mean of what the
    // first left over: the leftovers are of the size of sigma, so their sum is exact to ~1e-7 sigma
    float rest = 0.0f;
    for (uint32_t i = threadIdx.x; i < n; i += 256) rest += px[i] - mean;
    mean += block_reduce<false>(rest, red) / (float) n;
    float sum2 = 0.0f;
    for (uint32_t i = threadIdx.x; i < n; i += 256) { const float v = px[i] - mean; sum2 += v * v; }
    const float scale = 1.0f / sqrtf(block_reduce<false>(sum2, red) / (float) n + eps);
    for (uint32_t i = threadIdx.x; i < n; i += 256) py[i] = (px[i] - mean) * scale;
}

// The same for rows of up to NT*16 floats with 16-byte aligned rows: the row is read once with float4 loads and kept in
// registers, the norm weight is requested before the reduction so its latency hides behind it.  Few rows (token generation)
// run with 1024 threads per row, many rows (prefill) with 256.
// ADD: x = a + b first, also written to `s` — the residual add that feeds the norm (ffn_inp = cur + inpSA; next layer's
// inpL = ffn_out + ffn_inp, src/llama-model.cpp:4280, 4340-4346) in the same pass.
template <bool MUL, bool ADD, int NT>
__global__ void __launch_bounds__(NT)
rms_norm_vec_kernel(const char * __restrict__ x, const char * __restrict__ b, const float * __restrict__ w, char * __restrict__ y,
                    char * __restrict__ s, const Shape sx, const Shape sb, const Shape sy, const Shape ss, const float eps) {
    __shared__ float red[17];
    uint32_t i1, i2, i3;
    row_coords(blockIdx.x, (uint32_t) sx.ne[1], (uint32_t) sx.ne[2], i1, i2, i3);
    const float4 * px = (const float4 *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
    float4 *       py = (float4 *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]);
    const uint32_t n4 = (uint32_t) sx.ne[0] / 4;
    float4 v[4], wv[4];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x + j * NT;
        v[j] = i < n4 ? px[i] : make_float4(0, 0, 0, 0);
        if (MUL) wv[j] = i < n4 ? ((const float4 *) w)[i] : make_float4(0, 0, 0, 0);
    }
    if (ADD) {
        const float4 * pb = (const float4 *) (b + i1 * sb.nb[1] + i2 * sb.nb[2] + i3 * sb.nb[3]);
        float4 *       ps = (float4 *) (s + i1 * ss.nb[1] + i2 * ss.nb[2] + i3 * ss.nb[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = threadIdx.x + j * NT;
            if (i < n4) {
                const float4 t = pb[i];
                v[j].x += t.x; v[j].y += t.y; v[j].z += t.z; v[j].w += t.w;
                ps[i] = v[j];
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += v[j].x * v[j].x + v[j].y * v[j].y + v[j].z * v[j].z + v[j].w * v[j].w;
    const float scale = rms_scale_block<NT>(sum, red, (float) sx.ne[0], eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x + j * NT;
        if (i < n4) {
            float4 r = make_float4(v[j].x * scale, v[j].y * scale, v[j].z * scale, v[j].w * scale);
            if (MUL) { r.x *= wv[j].x; r.y *= wv[j].y; r.z *= wv[j].z; r.w *= wv[j].w; }
            py[i] = r;
        }
    }
}

// ------------------------------------------------------------------------------------------------ SOFT_MAX
// ggml_compute_forward_soft_max_f32 (ggml-cpu.c:8261-8352): v = x*scale + slope(head)*mask[row % ne01]; softmax over the row.
// One block per row.  Rows up to 8192 values are staged in LDS; longer rows use dst as the staging area.
template <bool MASK_F16>
__global__ void __launch_bounds__(256)
soft_max_kernel(const float * __restrict__ x, const void * __restrict__ mask, float * __restrict__ y, const uint32_t nc, const uint32_t ne01,
                const uint32_t ne02, const float scale, const float max_bias, const float m0, const float m1, const uint32_t n_head_log2) {
    extern __shared__ float stage[];
    __shared__ float red[4];
    const uint32_t row = blockIdx.x;
    const uint32_t h = (row / ne01) % ne02;
    const float slope = max_bias > 0.0f ? (h < n_head_log2 ? powf(m0, (float) (h + 1)) : powf(m1, (float) (2 * (h - n_head_log2) + 1))) : 1.0f;
    const float * px = x + (size_t) row * nc;
    float *       py = y + (size_t) row * nc;
    const bool in_lds = nc <= 8192;
    float * v = in_lds ? stage : py;
    const size_t moff = (size_t) (row % ne01) * nc;
    float mx = -INFINITY;
    for (uint32_t i = threadIdx.x; i < nc; i += 256) {
        float t = px[i] * scale;
        if (mask) t += slope * (MASK_F16 ? __half2float(((const __half *) mask)[moff + i]) : ((const float *) mask)[moff + i]);
        v[i] = t;
        mx = fmaxf(mx, t);
    }
    mx = block_reduce<true>(mx, red);
    float sum = 0.0f;
    for (uint32_t i = threadIdx.x; i < nc; i += 256) {
        const float e = expf(v[i] - mx);          // a fully masked row (-inf everywhere) gives NaN on the CPU too
        v[i] = e;
        sum += e;
    }
    sum = block_reduce<false>(sum, red);
    const float inv = 1.0f / sum;
    for (uint32_t i = threadIdx.x; i < nc; i += 256) py[i] = v[i] * inv;
}

// Rows of up to 1024 values (attention over a prompt of that length): one WAVE per row, the row in registers (float4 per
// lane and trip), reductions on the wave only: no LDS, no barrier, four rows per workgroup.  f32 mask, no ALiBi.
template <int V4>      // float4 per lane: the row has at most 256 * V4 values
__global__ void __launch_bounds__(256)
soft_max_wave_kernel(const float * __restrict__ x, const float * __restrict__ mask, float * __restrict__ y, const uint32_t nc, const uint32_t ne01,
                     const uint32_t rows, const float scale) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    const float4 * px = (const float4 *) (x + (size_t) row * nc);
    const float4 * pm = mask ? (const float4 *) (mask + (size_t) (row % ne01) * nc) : nullptr;
    float4 *       py = (float4 *) (y + (size_t) row * nc);
    const uint32_t n4 = nc / 4;
    float4 v[V4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < V4; ++j) {
        const uint32_t i = lane + 64 * j;
        if (i < n4) {
            float4 t = px[i];
            t.x *= scale; t.y *= scale; t.z *= scale; t.w *= scale;
            if (pm) { const float4 m = pm[i]; t.x += m.x; t.y += m.y; t.z += m.z; t.w += m.w; }
            v[j] = t;
            mx = fmaxf(fmaxf(mx, fmaxf(t.x, t.y)), fmaxf(t.z, t.w));
        } else {
            v[j] = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
        }
    }
    mx = wave_max(mx);
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < V4; ++j) {
        v[j].x = expf(v[j].x - mx); v[j].y = expf(v[j].y - mx); v[j].z = expf(v[j].z - mx); v[j].w = expf(v[j].w - mx);
        sum += v[j].x + v[j].y + v[j].z + v[j].w;
    }
    sum = wave_sum(sum);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int j = 0; j < V4; ++j) {
        const uint32_t i = lane + 64 * j;
        if (i < n4) py[i] = make_float4(v[j].x * inv, v[j].y * inv, v[j].z * inv, v[j].w * inv);
    }
}

// ------------------------------------------------------------------------------------------------ ROPE
// ggml_compute_forward_rope_f32 (ggml-cpu.c:8708-8893) with rope_yarn / ggml_rope_cache_init (:8610-8648): modes "normal"
// (pairs (2p, 2p+1)) and NEOX (pairs (p, p + n_dims/2)); channels >= n_dims are copied.  theta is built by the same
// repeated f32 multiply as the CPU cache (theta *= theta_scale), so it carries the same rounding.
struct RopeParams {
    int   n_dims, neox;
    float theta_scale, freq_scale, ext_factor, attn_factor, corr0, corr1;
};
// cos / sin of pair p at position pos (rope_yarn + ggml_rope_cache_init, ggml-cpu.c:8610-8648): theta by the CPU's repeated f32 multiply
__device__ __forceinline__ void rope_cs_ff(const float pos, const uint32_t p, const RopeParams & rp, const float ffp, float & c, float & s);
__device__ __forceinline__ void rope_cs(const float pos, const uint32_t p, const RopeParams & rp, const float * __restrict__ ff, float & c, float & s) {
    rope_cs_ff(pos, p, rp, ff ? ff[p] : 1.0f, c, s);
}
// (ffp: the pair's frequency factor, already loaded)
__device__ __forceinline__ void rope_cs_ff(const float pos, const uint32_t p, const RopeParams & rp, const float ffp, float & c, float & s) {
    float theta = pos;
    if (rp.n_dims <= 128) {
        // the CPU's repeated multiply, lane p keeping step p of it: 64 straight-line steps.  (As `for (k < p)` the trip count
        // differs per lane and every step pays a compare, an exec update and a branch: 1.2 us of the decode attention's prologue)
        float t = pos;
#pragma unroll
        for (uint32_t k = 0; k < 64; ++k) { theta = k == p ? t : theta; t *= rp.theta_scale; }
    } else {
        for (uint32_t k = 0; k < p; ++k) theta *= rp.theta_scale;
    }
    const float theta_extrap = theta / ffp;
    const float theta_interp = rp.freq_scale * theta_extrap;
    float th = theta_interp, mscale = rp.attn_factor;
    if (rp.ext_factor != 0.0f) {
        const float yv = ((float) p - rp.corr0) / fmaxf(0.001f, rp.corr1 - rp.corr0);
        const float ramp_mix = (1.0f - fminf(1.0f, fmaxf(0.0f, yv))) * rp.ext_factor;
        th = theta_interp * (1.0f - ramp_mix) + theta_extrap * ramp_mix;
        mscale *= 1.0f + 0.1f * logf(1.0f / rp.freq_scale);
    }
    // th can be thousands of radians (position times the first frequencies): ocml's sinf / cosf take their large-argument
    // path there.  One reduction in double (exact to ~1e-13 rad) and the fast pair on the remainder give the same values
    // to f32 rounding at a fraction of the instructions.
    // Round 3: the reduction goes to the quadrant, |y| <= pi/4, and the pair comes from the two short polynomials libm itself uses
    // on that interval (cephes sinf / cosf, ~1 ulp): a third of the instructions of ocml's pair, which re-check the argument's range.
    const double td = (double) th;
    const double qd = rint(td * 0.6366197723675814);
    const float y = (float) fma(qd, -1.5707963267948966, td), z = y * y;
    const float ys = y + y * z * (-1.6666654611e-1f + z * (8.3321608736e-3f + z * -1.9515295891e-4f));
    const float yc = 1.0f - 0.5f * z + z * z * (4.166664568298827e-2f + z * (-1.388731625493765e-3f + z * 2.443315711809948e-5f));
    const int q = (int) (long long) qd & 3;
    c = (q == 0 ? yc : q == 1 ? -ys : q == 2 ? -yc : ys) * mscale;
    s = (q == 0 ? ys : q == 1 ? yc : q == 2 ? -ys : -yc) * mscale;
}
// one pair of one row; TD = float or __half (the K-cache store of build_attn is rope(k) -> f16)
template <typename TD>
__device__ __forceinline__ void rope_pair(const char * __restrict__ x, const int32_t * __restrict__ pos, const float * __restrict__ ff,
                                          char * __restrict__ y, const Shape & sx, const Shape & sy, const RopeParams & rp, const uint32_t gid) {
    const uint32_t half = (uint32_t) sx.ne[0] / 2;
    const uint32_t p = gid % half;
    uint32_t i1, i2, i3;
    row_coords(gid / half, (uint32_t) sx.ne[1], (uint32_t) sx.ne[2], i1, i2, i3);
    const float * px = (const float *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
    TD *          py = (TD *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]);
    const uint32_t i0 = 2 * p;
    if (i0 >= (uint32_t) rp.n_dims) {             // pass-through channels
        py[i0] = (TD) px[i0];
        py[i0 + 1] = (TD) px[i0 + 1];
        return;
    }
    float c, s;
    rope_cs((float) pos[i2], p, rp, ff, c, s);
    const uint32_t ia = rp.neox ? p : i0, ib = rp.neox ? p + rp.n_dims / 2 : i0 + 1;
    const float x0 = px[ia], x1 = px[ib];
    py[ia] = (TD) (x0 * c - x1 * s);
    py[ib] = (TD) (x0 * s + x1 * c);
}
__global__ void __launch_bounds__(256)
rope_kernel(const char * __restrict__ x, const int32_t * __restrict__ pos, const float * __restrict__ ff, char * __restrict__ y,
            const Shape sx, const Shape sy, const RopeParams rp, const uint32_t total_pairs) {
    const uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid < total_pairs) rope_pair<float>(x, pos, ff, y, sx, sy, rp, gid);
}

// ------------------------------------------------------------------------------------------------ CPY / CONT / DUP
// ggml_compute_forward_dup (ggml-cpu.c): element i of src (in src's index order) goes to element i of dst (in dst's
// index order); shapes may differ, element counts agree.  F32 / F16 either side.
template <typename T> __device__ __forceinline__ float ld_as_f32(const char * p);
template <> __device__ __forceinline__ float ld_as_f32<float>(const char * p) { return *(const float *) p; }
template <> __device__ __forceinline__ float ld_as_f32<__half>(const char * p) { return __half2float(*(const __half *) p); }
template <typename T> __device__ __forceinline__ void st_from_f32(char * p, float v);
template <> __device__ __forceinline__ void st_from_f32<float>(char * p, float v) { *(float *) p = v; }
template <> __device__ __forceinline__ void st_from_f32<__half>(char * p, float v) { *(__half *) p = __float2half(v); }

__device__ __forceinline__ size_t elem_offset(uint32_t i, const Shape & s) {
    const uint32_t i0 = i % (uint32_t) s.ne[0];
    uint32_t t = i / (uint32_t) s.ne[0];
    const uint32_t i1 = t % (uint32_t) s.ne[1];
    t /= (uint32_t) s.ne[1];
    const uint32_t i2 = t % (uint32_t) s.ne[2], i3 = t / (uint32_t) s.ne[2];
    return (size_t) i0 * s.nb[0] + (size_t) i1 * s.nb[1] + (size_t) i2 * s.nb[2] + (size_t) i3 * s.nb[3];
}
template <typename TS, typename TD>
__global__ void __launch_bounds__(256)
cpy_kernel(const char * __restrict__ x, char * __restrict__ y, const Shape sx, const Shape sy, const uint32_t n) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    st_from_f32<TD>(y + elem_offset(i, sy), ld_as_f32<TS>(x + elem_offset(i, sx)));
}
// 2-D transpose through LDS for the case the scalar kernel does worst: src is walked along its dim 1 (stride one element)
// while dst rows are dense — the V-cache store of build_attn (v_cur^T [n_tokens, n_embd] -> rows of the transposed cache).
// src element (i0, i1) at x + i0*sx0 + i1*sx1 with sx1 == sizeof(TS); dst element at y + i0*sizeof(TD) + i1*sy1.
template <typename TS, typename TD>
__global__ void __launch_bounds__(256)
cpy_transpose_kernel(const char * __restrict__ x, char * __restrict__ y, const uint32_t ne0, const uint32_t ne1, const int64_t sx0,
                     const int64_t sy1) {
    __shared__ float tile[32][33];
    const uint32_t b0 = blockIdx.x * 32, b1 = blockIdx.y * 32;
    const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;          // 32 x 8
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i0 = b0 + ty + j * 8, i1 = b1 + tx;                 // consecutive threads walk src's dense direction
        if (i0 < ne0 && i1 < ne1) tile[ty + j * 8][tx] = ld_as_f32<TS>(x + (size_t) i0 * sx0 + (size_t) i1 * sizeof(TS));
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i0 = b0 + tx, i1 = b1 + ty + j * 8;                 // ... and dst's dense direction
        if (i0 < ne0 && i1 < ne1) st_from_f32<TD>(y + (size_t) i0 * sizeof(TD) + (size_t) i1 * sy1, tile[tx][ty + j * 8]);
    }
}

// What follows the q/k/v projections of a few-token batch in build_attn (src/llama-graph.cpp:1306-1365), as ONE launch:
//   rope(q) -> f32            rope(k) -> the f16 K cache (ggml_rope_ext + ggml_cpy(k_cur, k_cache_view))
//   v       -> the f16 (transposed) V cache (ggml_cpy(v_cur^T, v_cache_view))
// The grid is the concatenation of the three index spaces; k and v parts are optional (nk = 0 / nv = 0).
// the same for ROPE_HC heads of one (pair, token): cos / sin (the double-precision reduction and two polynomials, ~150 instructions) once for
// all of them; round 3: one thread per (pair, head, token) made the 512-token launch ALU-bound at 14.5 us for 22 MB of traffic
template <typename TD>
__device__ __forceinline__ void rope_pair_heads(const char * __restrict__ x, const int32_t * __restrict__ pos, const float * __restrict__ ff,
                                                char * __restrict__ y, const Shape & sx, const Shape & sy, const RopeParams & rp, const uint32_t gid) {
    const uint32_t half = (uint32_t) sx.ne[0] / 2, ne1 = (uint32_t) sx.ne[1], nch = (ne1 + ROPE_HC - 1) / ROPE_HC;
    const uint32_t p = gid % half;
    uint32_t c1, i2, i3;
    row_coords(gid / half, nch, (uint32_t) sx.ne[2], c1, i2, i3);
    const uint32_t i0 = 2 * p, h0 = c1 * ROPE_HC, h1 = h0 + ROPE_HC < ne1 ? h0 + ROPE_HC : ne1;
    const bool pass = i0 >= (uint32_t) rp.n_dims;                // pass-through channels
    float c = 1.0f, s = 0.0f;
    if (!pass) rope_cs((float) pos[i2], p, rp, ff, c, s);
    const uint32_t ia = pass || !rp.neox ? i0 : p, ib = pass || !rp.neox ? i0 + 1 : p + rp.n_dims / 2;
    for (uint32_t i1 = h0; i1 < h1; ++i1) {
        const float * px = (const float *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
        TD *          py = (TD *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]);
        const float x0 = px[ia], x1 = px[ib];
        if (pass) { py[ia] = (TD) x0; py[ib] = (TD) x1; }
        else      { py[ia] = (TD) (x0 * c - x1 * s); py[ib] = (TD) (x0 * s + x1 * c); }
    }
}
struct RopeStoreArgs {
    const char * q; char * qd; const char * k; char * kd; const char * v; char * vd;
    const int32_t * pos; const float * ff;
    Shape sq, sqd, sk, skd, sv, svd;
    RopeParams rp;
    uint32_t nq, nk, nv;          // threads for q, for k (rope_heads_threads: a thread takes a pair of ROPE_HC heads), elements of v
};
// VT: the v part is a 2-D transpose (v_cur^T, dense along its dim 1, into rows of the transposed cache, dense along dim 0) and
// large enough for 32 x 32 tiles through LDS: blocks behind the rope blocks take one tile each, reading along the source's dense
// direction and writing along the destination's (the element-wise form reads 4-byte values 4 KB apart)
template <bool VT>
__global__ void __launch_bounds__(256)
rope_store_kernel(const RopeStoreArgs g, const uint32_t pair_blocks, const uint32_t tiles0) {
    if (VT && blockIdx.x >= pair_blocks) {
        __shared__ float tile[32][33];
        const uint32_t t = blockIdx.x - pair_blocks, b0 = (t % tiles0) * 32, b1 = (t / tiles0) * 32;
        const uint32_t ne0 = (uint32_t) g.sv.ne[0], ne1 = (uint32_t) g.sv.ne[1];
        const uint32_t tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i0 = b0 + ty + j * 8, i1 = b1 + tx;
            if (i0 < ne0 && i1 < ne1) tile[ty + j * 8][tx] = *(const float *) (g.v + (size_t) i0 * g.sv.nb[0] + (size_t) i1 * 4);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i0 = b0 + tx, i1 = b1 + ty + j * 8;
            if (i0 < ne0 && i1 < ne1) *(__half *) (g.vd + (size_t) i0 * 2 + (size_t) i1 * g.svd.nb[1]) = __float2half(tile[tx][ty + j * 8]);
        }
        return;
    }
    uint32_t gid = blockIdx.x * 256u + threadIdx.x;
    if (gid < g.nq) { rope_pair_heads<float>(g.q, g.pos, g.ff, g.qd, g.sq, g.sqd, g.rp, gid); return; }
    gid -= g.nq;
    if (gid < g.nk) { rope_pair_heads<__half>(g.k, g.pos, g.ff, g.kd, g.sk, g.skd, g.rp, gid); return; }
    gid -= g.nk;
    if (!VT && gid < g.nv) st_from_f32<__half>(g.vd + elem_offset(gid, g.svd), ld_as_f32<float>(g.v + elem_offset(gid, g.sv)));
}

// ------------------------------------------------------------------------------------------------ GET_ROWS
// ggml_compute_forward_get_rows (ggml-cpu.c): dst[:, i10, i11, i12] = row src1[i10, i11, i12] of src0[:, :, i11, i12] as f32.
template <typename TS>
__global__ void __launch_bounds__(256)
get_rows_kernel(const char * __restrict__ x, const char * __restrict__ ids, char * __restrict__ y, const Shape sx, const Shape si, const Shape sy) {
    uint32_t i10, i11, i12;
    row_coords(blockIdx.x, (uint32_t) si.ne[0], (uint32_t) si.ne[1], i10, i11, i12);
    const int32_t r = *(const int32_t *) (ids + i10 * si.nb[0] + i11 * si.nb[1] + i12 * si.nb[2]);
    if (r < 0 || r >= sx.ne[1]) return;                      // the CPU asserts; leave the row untouched
    const char * px = x + (size_t) r * sx.nb[1] + i11 * sx.nb[2] + i12 * sx.nb[3];
    float *      py = (float *) (y + i10 * sy.nb[1] + i11 * sy.nb[2] + i12 * sy.nb[3]);
    for (uint32_t i = threadIdx.x; i < (uint32_t) sx.ne[0]; i += 256) py[i] = ld_as_f32<TS>(px + (size_t) i * sizeof(TS));
}
// quantized rows: one unit per thread, the bit-exact unpack of qmm_device.hiph
template <int T>
__global__ void __launch_bounds__(256)
get_rows_q_kernel(const uint8_t * __restrict__ x, const char * __restrict__ ids, char * __restrict__ y, const Shape sx, const Shape si, const Shape sy) {
    uint32_t i10, i11, i12;
    row_coords(blockIdx.x, (uint32_t) si.ne[0], (uint32_t) si.ne[1], i10, i11, i12);
    const int32_t r = *(const int32_t *) (ids + i10 * si.nb[0] + i11 * si.nb[1] + i12 * si.nb[2]);
    if (r < 0 || r >= sx.ne[1]) return;
    const uint8_t * px = x + (size_t) r * sx.nb[1] + i11 * sx.nb[2] + i12 * sx.nb[3];
    float *         py = (float *) (y + i10 * sy.nb[1] + i11 * sy.nb[2] + i12 * sy.nb[3]);
    const int units = (int) (sx.ne[0] / Traits<T>::UNIT_W);
    for (int u = threadIdx.x; u < units; u += 256) {
        Unit<T> un;
        un.load(px, u, (int) sx.ne[0]);
        float out[Traits<T>::UNIT_W];
        un.to_f32(u, out);
#pragma unroll
        for (int rr = 0; rr < Unit<T>::RUNS; ++rr) {
            float * o = py + Unit<T>::k_run(u, rr);
#pragma unroll
            for (int e = 0; e < Unit<T>::RUN_LEN; ++e) o[e] = out[rr * Unit<T>::RUN_LEN + e];
        }
    }
}

// ------------------------------------------------------------------------------------------------ ARGSORT, SUM_ROWS
// The two small ops of the MoE router (build_moe_ffn, src/llama-graph.cpp:842-858: ggml_top_k = argsort + view, ggml_sum_rows
// for the weight normalisation), so that a Mixtral layer stays one split.
// ggml_compute_forward_argsort_f32 (ggml-cpu.c:10199-10236) orders indices by value; here by rank: element i goes to the
// position "number of elements that sort before it" (ties by index), the same permutation whenever the values are distinct.
__global__ void __launch_bounds__(256)
argsort_kernel(const char * __restrict__ x, char * __restrict__ y, const Shape sx, const Shape sy, const int desc) {
    uint32_t i1, i2, i3;
    row_coords(blockIdx.x, (uint32_t) sx.ne[1], (uint32_t) sx.ne[2], i1, i2, i3);
    const float * px = (const float *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
    int32_t *     py = (int32_t *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]);
    const uint32_t n = (uint32_t) sx.ne[0];
    for (uint32_t i = threadIdx.x; i < n; i += 256) {
        const float v = px[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) {
            const float u = px[j];
            rank += (desc ? u > v : u < v) || (u == v && j < i);
        }
        py[rank] = (int32_t) i;
    }
}
// ggml_compute_forward_sum_rows_f32 (ggml-cpu.c): dst[0, i1, i2, i3] = sum over i0; one wave per row
__global__ void __launch_bounds__(256)
sum_rows_kernel(const char * __restrict__ x, char * __restrict__ y, const Shape sx, const Shape sy, const uint32_t rows) {
    const uint32_t row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    uint32_t i1, i2, i3;
    row_coords(row, (uint32_t) sx.ne[1], (uint32_t) sx.ne[2], i1, i2, i3);
    const float * px = (const float *) (x + i1 * sx.nb[1] + i2 * sx.nb[2] + i3 * sx.nb[3]);
    float s = 0.0f;
    for (uint32_t i = lane; i < (uint32_t) sx.ne[0]; i += 64) s += px[i];
    s = wave_sum(s);
    if (lane == 0) *(float *) (y + i1 * sy.nb[1] + i2 * sy.nb[2] + i3 * sy.nb[3]) = s;
}

// ------------------------------------------------------------------------------------------------ MUL_MAT, F16 / F32 src0
// ggml_compute_forward_mul_mat with a non-quantized src0 (ggml-cpu.c:6745-6937): the KQ and KQV products of
// build_attn_mha (src/llama-graph.cpp:1126-1213), whose src0 is a strided view of the F16 KV cache, and small F32 matrices
// (the MoE router).  dst[i13][i12][n][m] = sum_k src0[i13/r3][i12/r2][m][k] * src1[i13][i12][n][k].
//
// F16: as on the CPU (vec_dot_type of F16 is F16: src1 is rounded to f16, products accumulate in f32).  A workgroup of 4 waves
// owns 64 src0 rows x 64 src1 rows; both operands go through LDS as f16 in 32-deep K-steps and each wave drives
// v_mfma_f32_32x32x16_f16 with tokens on the MFMA row index and src0 rows on the lane index, so a lane's 16 results are
// 16 tokens of ONE dst column and every store instruction writes 128 contiguous bytes per half-wave.
struct MmArgs {
    const char * a;  const char * b;  char * d;
    int64_t a_nb1, a_nb2, a_nb3, b_nb1, b_nb2, b_nb3, d_nb1, d_nb2, d_nb3;
    int32_t M, N, K, ne12, r2, r3;
};
constexpr int MM_BK = 32, MM_LD = MM_BK + 8;      // LDS row pitch 80 B: 16-byte reads of 32 rows spread over all banks

template <bool VEC>
__global__ void __launch_bounds__(256)
mul_mat_f16_kernel(const MmArgs g) {
    __shared__ __attribute__((aligned(16))) _Float16 sa[MM_T * MM_LD];        // src0 rows (weights side)
    __shared__ __attribute__((aligned(16))) _Float16 sb[MM_T * MM_LD];        // src1 rows (tokens), rounded to f16
    const int i12 = blockIdx.z % g.ne12, i13 = blockIdx.z / g.ne12;
    const char * pa = g.a + (int64_t) (i12 / g.r2) * g.a_nb2 + (int64_t) (i13 / g.r3) * g.a_nb3;
    const char * pb = g.b + (int64_t) i12 * g.b_nb2 + (int64_t) i13 * g.b_nb3;
    char *       pd = g.d + (int64_t) i12 * g.d_nb2 + (int64_t) i13 * g.d_nb3;
    const int m0 = blockIdx.x * MM_T, n0 = blockIdx.y * MM_T;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int lr = tid >> 2, lk = (tid & 3) * 8;                               // staging: row lr, 8 consecutive k from lk
    f32x16v acc = {0};
    for (int k0 = 0; k0 < g.K; k0 += MM_BK) {
        h16x8 va = {0}, vb = {0};
        const int k = k0 + lk;
        if (m0 + lr < g.M) {
            const char * p = pa + (int64_t) (m0 + lr) * g.a_nb1 + (int64_t) k * 2;
            if (VEC && k + 8 <= g.K) {
                va = *(const h16x8 *) p;
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) if (k + e < g.K) va[e] = ((const _Float16 *) p)[e];
            }
        }
        if (n0 + lr < g.N) {
            const float * p = (const float *) (pb + (int64_t) (n0 + lr) * g.b_nb1) + k;
            if (VEC && k + 8 <= g.K) {
                const float4 x = ((const float4 *) p)[0], y = ((const float4 *) p)[1];
                vb = h16x8{ (_Float16) x.x, (_Float16) x.y, (_Float16) x.z, (_Float16) x.w, (_Float16) y.x, (_Float16) y.y, (_Float16) y.z, (_Float16) y.w };
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) if (k + e < g.K) vb[e] = (_Float16) p[e];
            }
        }
        __syncthreads();                                                        // previous K-step's fragment reads are done
        *(h16x8 *) &sa[lr * MM_LD + lk] = va;
        *(h16x8 *) &sb[lr * MM_LD + lk] = vb;
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < MM_BK; kk += 16) {
            const h16x8 fa = *(const h16x8 *) &sb[(wn + (lane & 31)) * MM_LD + kk + (lane >> 5) * 8];     // tokens: MFMA rows
            const h16x8 fb = *(const h16x8 *) &sa[(wm + (lane & 31)) * MM_LD + kk + (lane >> 5) * 8];     // src0 rows: MFMA columns
            acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc, 0, 0, 0);
        }
    }
    const int m = m0 + wm + (lane & 31);
    if (m < g.M) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int n = n0 + wn + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
            if (n < g.N) *(float *) (pd + (int64_t) n * g.d_nb1 + (int64_t) m * 4) = acc[r];
        }
    }
}

// The router of a mixture-of-experts block after its logits (build_moe_ffn, src/llama-graph.cpp:818-858), one launch instead of
// five: probs = soft_max(logits); ids = argsort(probs, descending) (top-k = its first n_used entries); weights = probs[ids[:n_used]]
// normalised by their sum (ggml_get_rows, ggml_sum_rows, ggml_div).  One wave per token, lane e holds expert e (n_expert <= 64).
// (the body: one wave, lane e holds the logit of expert e; shared by moe_router_kernel and moe_router_logits_kernel)
__device__ __forceinline__ void router_of_logits(const float x, const int lane, const int n_expert, const int n_used, const int normalise,
                                                 int32_t * __restrict__ ids_row, float * __restrict__ weights_row) {
    const float mx = wave_max(x);
    const float e = lane < n_expert ? expf(x - mx) : 0.0f;
    // soft_max_wave_kernel's arithmetic AND its order of additions: there lane g holds four consecutive values and adds them left to
    // right before the wave reduction; a sum taken in any other order may differ in the last bit, and a last bit of a router weight is
    // enough to flip an int8 rounding one layer further down (round 3: `llama-e2e layers` showed the one-launch router and the five
    // per-node launches 2e-2 of an rms apart on one element of a later layer; the dense models agreed bit for bit)
    const float e0 = __shfl(e, (4 * lane) & 63, 64), e1 = __shfl(e, (4 * lane + 1) & 63, 64), e2 = __shfl(e, (4 * lane + 2) & 63, 64), e3 = __shfl(e, (4 * lane + 3) & 63, 64);
    const float g4 = lane < 16 ? ((e0 + e1) + e2) + e3 : 0.0f;
    const float p = e * (1.0f / wave_sum(g4));                     // exp(x - max) * (1 / sum)
    int rank = 0;
    for (int j = 0; j < n_expert; ++j) {
        const float u = __shfl(p, j, 64);
        rank += u > p || (u == p && j < lane);
    }
    if (lane < n_expert) ids_row[rank] = lane;
    const bool sel = lane < n_expert && rank < n_used;
    // sum_rows_kernel adds the selected weights with the weight of rank r on lane r: the same placement here
    float byrank = 0.0f;
    for (int r = 0; r < n_used; ++r) {
        const int src = __ffsll((long long) __ballot(lane < n_expert && rank == r)) - 1;     // (every rank below n_expert has exactly one owner)
        const float v = __shfl(p, src & 63, 64);
        if (lane == r) byrank = v;
    }
    const float sum = wave_sum(byrank);
    if (sel) weights_row[rank] = normalise ? p / sum : p;
}
__global__ void __launch_bounds__(256)
moe_router_kernel(const char * __restrict__ logits, char * __restrict__ ids, char * __restrict__ weights, const int64_t l_nb1, const int64_t i_nb1,
                  const int64_t w_nb1, const int n_expert, const int n_used, const int n_tokens, const int normalise) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= n_tokens) return;
    const float x = lane < n_expert ? ((const float *) (logits + (int64_t) t * l_nb1))[lane] : -INFINITY;
    router_of_logits(x, lane, n_expert, n_used, normalise, (int32_t *) (ids + (int64_t) t * i_nb1), (float *) (weights + (int64_t) t * w_nb1));
}

// The router WITH its logits for a few tokens (round 3: 32 of Mixtral's ~390 launches per generated token): logits = gate_inp x
// (F32 [K, n_expert], build_moe_ffn's first MUL_MAT) and everything moe_router_kernel does, one workgroup per token.  Eight groups of
// DOT_T = 128 threads take eight experts side by side, each group exactly as mul_mat_dot_block_kernel takes one dst element (the same
// shares, the same wave reduction, the same order of the wave sums), so the logits row it writes is the per-node kernel's bit for
// bit; wave 0 then routes the row from LDS.  (First version: four groups of 256, two rounds for Mixtral's eight experts: the launch
// then took as long as the two it replaced, gpu_ms_per_token 2.94 -> 2.93.)
__device__ __forceinline__ float dot_f32_share(const float * __restrict__ pa, const float * __restrict__ pb, const int K, const int t);
// NORM (round 3): x is the un-normed row; the workgroup forms rms_norm(x) * norm_w itself (rms_norm_vec_kernel<true, false, 1024>'s arithmetic and order of
// additions, so the bits of the separate launch), stores it to `normed` for the expert MUL_MAT_IDs and dots the logits against the copy in LDS:
// build_moe_ffn's ffn_norm launch (4.75 us of a Mixtral layer's ~84) disappears.  K <= 16384, K % 4 == 0, 16-byte aligned rows.
template <bool NORM>
__global__ void __launch_bounds__(1024)
moe_router_logits_kernel(const char * __restrict__ wgt, const char * __restrict__ x, char * __restrict__ logits, char * __restrict__ ids,
                         char * __restrict__ weights, const int64_t a_nb1, const int64_t b_nb1, const int64_t l_nb1, const int64_t i_nb1, const int64_t w_nb1,
                         const int K, const int n_expert, const int n_used, const int normalise,
                         const float * __restrict__ norm_w = nullptr, const float eps = 0.0f, char * __restrict__ normed = nullptr, const int64_t y_nb1 = 0) {
    constexpr int NG = 1024 / DOT_T, WPG = DOT_T / 64;     // groups per workgroup (experts side by side), waves per group
    extern __shared__ __attribute__((aligned(16))) float xs[];
    __shared__ float red[17];
    __shared__ float lg[64];
    const int n = blockIdx.x, tid = threadIdx.x, grp = tid / DOT_T, tg = tid % DOT_T, lane = tid & 63, wg = (tid >> 6) % WPG;
    const float * pb = (const float *) (x + (int64_t) n * b_nb1);
    if (NORM) {
        const float4 * px = (const float4 *) pb;
        float4 *       py = (float4 *) (normed + (int64_t) n * y_nb1);
        const uint32_t n4 = (uint32_t) K / 4;
        float4 v[4], wv[4];
        float sum = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = tid + j * 1024;
            v[j]  = i < n4 ? px[i] : make_float4(0, 0, 0, 0);
            wv[j] = i < n4 ? ((const float4 *) norm_w)[i] : make_float4(0, 0, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += v[j].x * v[j].x + v[j].y * v[j].y + v[j].z * v[j].z + v[j].w * v[j].w;
        const float scale = rms_scale_block<1024>(sum, red, (float) K, eps);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t i = tid + j * 1024;
            if (i < n4) {
                float4 r = make_float4(v[j].x * scale, v[j].y * scale, v[j].z * scale, v[j].w * scale);
                r.x *= wv[j].x; r.y *= wv[j].y; r.z *= wv[j].z; r.w *= wv[j].w;
                py[i] = r;
                ((float4 *) xs)[i] = r;
            }
        }
        __syncthreads();
        pb = xs;
    }
    for (int e0 = 0; e0 < n_expert; e0 += NG) {              // uniform trip count: every thread meets every barrier
        const int e = e0 + grp, ec = e < n_expert ? e : n_expert - 1;
        float s = dot_f32_share((const float *) (wgt + (int64_t) ec * a_nb1), pb, K, tg);
        s = wave_sum(s);
        __syncthreads();
        if (lane == 0) red[grp * WPG + wg] = s;
        __syncthreads();
        float r = red[grp * WPG];
        for (int i = 1; i < WPG; ++i) r += red[grp * WPG + i];
        if (e < n_expert && tg == 0) { lg[e] = r; ((float *) (logits + (int64_t) n * l_nb1))[e] = r; }
    }
    __syncthreads();
    if (tid < 64)
        router_of_logits(lane < n_expert ? lg[lane] : -INFINITY, lane, n_expert, n_used, normalise, (int32_t *) (ids + (int64_t) n * i_nb1),
                         (float *) (weights + (int64_t) n * w_nb1));
}

// The other end of a mixture-of-experts block (build_moe_ffn, src/llama-graph.cpp:896-911): experts * weights, then the sum over the
// used experts through 2-D views, as one launch: out[n][c] = ((x[n][0][c] w[n][0] + x[n][1][c] w[n][1]) + ...), in the graph's order.
// (four columns of one token: ((x0 w0) + x1 w1) + ..., shared by moe_combine_kernel and moe_combine_add_norm_kernel)
__device__ __forceinline__ float4 moe_combine4(const char * __restrict__ px, const char * __restrict__ pw, const int64_t x_nb1, const int64_t w_nb1, const int U) {
    float4 acc = *(const float4 *) px;
    {
        const float w0 = *(const float *) pw;
        acc.x *= w0; acc.y *= w0; acc.z *= w0; acc.w *= w0;
    }
    for (int u = 1; u < U; ++u) {
        const float4 v = *(const float4 *) (px + (int64_t) u * x_nb1);
        const float wu = *(const float *) (pw + (int64_t) u * w_nb1);
        acc.x += v.x * wu; acc.y += v.y * wu; acc.z += v.z * wu; acc.w += v.w * wu;
    }
    return acc;
}
__global__ void __launch_bounds__(256)
moe_combine_kernel(const char * __restrict__ x, const char * __restrict__ w, char * __restrict__ out, const int64_t x_nb1, const int64_t x_nb2,
                   const int64_t w_nb1, const int64_t w_nb2, const int64_t o_nb1, const int E, const int U) {
    const int n = blockIdx.y;
    const int c = (blockIdx.x * 256 + threadIdx.x) * 4;
    if (c >= E) return;
    *(float4 *) (out + (int64_t) n * o_nb1 + (int64_t) c * 4) = moe_combine4(x + (int64_t) n * x_nb2 + (int64_t) c * 4, w + (int64_t) n * w_nb2, x_nb1, w_nb1, U);
}

// The block's tail with what follows it in the layer (round 3): out = combine(x, w) as above, sum = out + b (the residual: l_out),
// y = rms_norm(sum) * nw (the next attn_norm, or result_norm): moe_combine_kernel's and rms_norm_vec_kernel<true, true, NT>'s arithmetic
// in that kernel's partition and order of additions, so both results are the two launches' bit for bit.
template <int NT>
__global__ void __launch_bounds__(NT)
moe_combine_add_norm_kernel(const char * __restrict__ x, const char * __restrict__ wts, const char * __restrict__ b, const float * __restrict__ nw,
                            char * __restrict__ y, char * __restrict__ s, const int64_t x_nb1, const int64_t x_nb2, const int64_t w_nb1, const int64_t w_nb2,
                            const int64_t b_nb1, const int64_t y_nb1, const int64_t s_nb1, const int E, const int U, const float eps) {
    __shared__ float red[17];
    const int n = blockIdx.x;
    const float4 * pb = (const float4 *) (b + (int64_t) n * b_nb1);
    float4 *       py = (float4 *) (y + (int64_t) n * y_nb1);
    float4 *       ps = (float4 *) (s + (int64_t) n * s_nb1);
    const uint32_t n4 = (uint32_t) E / 4;
    float4 v[4], wv[4];
    float sum = 0.0f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x + j * NT;
        v[j] = i < n4 ? moe_combine4(x + (int64_t) n * x_nb2 + (int64_t) i * 16, wts + (int64_t) n * w_nb2, x_nb1, w_nb1, U) : make_float4(0, 0, 0, 0);
        wv[j] = i < n4 ? ((const float4 *) nw)[i] : make_float4(0, 0, 0, 0);
        if (i < n4) {
            const float4 t = pb[i];
            v[j].x += t.x; v[j].y += t.y; v[j].z += t.z; v[j].w += t.w;
        }
    }
    // every input of this token is in registers before the first output is stored: with ONE token (one workgroup: token generation) the
    // two results may therefore lie on ANY of the inputs, which is where ggml-alloc puts them in llama.cpp's graphs (l_out on the
    // dead router weights, the normed row on the residual); with more tokens the caller keeps them clear of what other workgroups read
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x + j * NT;
        if (i < n4) ps[i] = v[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) sum += v[j].x * v[j].x + v[j].y * v[j].y + v[j].z * v[j].z + v[j].w * v[j].w;
    const float scale = rms_scale_block<NT>(sum, red, (float) E, eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const uint32_t i = threadIdx.x + j * NT;
        if (i < n4) {
            float4 r = make_float4(v[j].x * scale, v[j].y * scale, v[j].z * scale, v[j].w * scale);
            r.x *= wv[j].x; r.y *= wv[j].y; r.z *= wv[j].z; r.w *= wv[j].w;
            py[i] = r;
        }
    }
}

// Few outputs with a long K (the MoE router at batch 1: 8 x 4096): one WORKGROUP per dst element, so K is spread over DOT_T = 128
// threads (256 until round 3: eight experts then did not fit one workgroup of moe_router_logits_kernel side by side) instead of 64 (the wave-per-element kernel walks K = 4096 in 64 dependent trips: 27 us per call, 0.87 ms per Mixtral token).
// (thread t of DOT_T's share of the dot product; shared with moe_router_logits_kernel so that both give the same bits)
__device__ __forceinline__ float dot_f32_share(const float * __restrict__ pa, const float * __restrict__ pb, const int K, const int t) {
    float s = 0.0f;
    if ((((uintptr_t) pa | (uintptr_t) pb) & 15) == 0) {
        const int k4 = K / 4;
        for (int k = t; k < k4; k += DOT_T) {
            const float4 x = ((const float4 *) pa)[k], y = ((const float4 *) pb)[k];
            s += x.x * y.x + x.y * y.y + x.z * y.z + x.w * y.w;
        }
        for (int k = k4 * 4 + t; k < K; k += DOT_T) s += pa[k] * pb[k];
    } else {
        for (int k = t; k < K; k += DOT_T) s += pa[k] * pb[k];
    }
    return s;
}
__global__ void __launch_bounds__(DOT_T)
mul_mat_dot_block_kernel(const MmArgs g) {
    __shared__ float red[4];
    const int i12 = blockIdx.z % g.ne12, i13 = blockIdx.z / g.ne12;
    const int m = blockIdx.x % g.M, n = blockIdx.x / g.M;
    const float * pa = (const float *) (g.a + (int64_t) (i12 / g.r2) * g.a_nb2 + (int64_t) (i13 / g.r3) * g.a_nb3 + (int64_t) m * g.a_nb1);
    const float * pb = (const float *) (g.b + (int64_t) i12 * g.b_nb2 + (int64_t) i13 * g.b_nb3 + (int64_t) n * g.b_nb1);
    float s = dot_f32_share(pa, pb, g.K, threadIdx.x);
    s = block_reduce<false>(s, red);
    if (threadIdx.x == 0) *(float *) (g.d + (int64_t) i12 * g.d_nb2 + (int64_t) i13 * g.d_nb3 + (int64_t) n * g.d_nb1 + (int64_t) m * 4) = s;
}

// F32 src0 (small matrices such as the MoE router ffn_gate_inp): one wave per dst element, f32 FMA, lanes stride K.
template <typename TA>
__global__ void __launch_bounds__(256)
mul_mat_dot_kernel(const MmArgs g) {
    const int i12 = blockIdx.z % g.ne12, i13 = blockIdx.z / g.ne12;
    const int64_t e = (int64_t) blockIdx.x * 4 + (threadIdx.x >> 6);
    if (e >= (int64_t) g.M * g.N) return;
    const int m = (int) (e % g.M), n = (int) (e / g.M), lane = threadIdx.x & 63;
    const char *  pa = g.a + (int64_t) (i12 / g.r2) * g.a_nb2 + (int64_t) (i13 / g.r3) * g.a_nb3 + (int64_t) m * g.a_nb1;
    const float * pb = (const float *) (g.b + (int64_t) i12 * g.b_nb2 + (int64_t) i13 * g.b_nb3 + (int64_t) n * g.b_nb1);
    float s = 0.0f;
    for (int k = lane; k < g.K; k += 64) s += ld_as_f32<TA>(pa + (int64_t) k * sizeof(TA)) * pb[k];
    s = wave_sum(s);
    if (lane == 0) *(float *) (g.d + (int64_t) i12 * g.d_nb2 + (int64_t) i13 * g.d_nb3 + (int64_t) n * g.d_nb1 + (int64_t) m * 4) = s;
}

// ------------------------------------------------------------------------------------------------ host side

// ggml_rope_yarn_corr_dims (ggml.c:3738-3754)
void rope_corr_dims(int n_dims, int n_ctx_orig, float freq_base, float beta_fast, float beta_slow, float dims[2]) {
    auto corr_dim = [&](float n_rot) { return n_dims * logf(n_ctx_orig / (n_rot * 2 * (float) M_PI)) / (2 * logf(freq_base)); };
    const float start = floorf(corr_dim(beta_fast)), end = ceilf(corr_dim(beta_slow));
    dims[0] = start > 0 ? start : 0;
    dims[1] = end < n_dims - 1 ? end : n_dims - 1;
}

// op_params of ggml_rope_ext (ggml.c ggml_rope_impl) -> kernel parameters
RopeParams rope_params(const qmm_tensor * d) {
    RopeParams rp;
    rp.n_dims = d->op_params[1];
    rp.neox = (d->op_params[2] & 2) != 0;
    const int n_ctx_orig = d->op_params[4];
    const float freq_base = f32_param(d, 5), beta_fast = f32_param(d, 9), beta_slow = f32_param(d, 10);
    rp.freq_scale = f32_param(d, 6);
    rp.ext_factor = f32_param(d, 7);
    rp.attn_factor = f32_param(d, 8);
    rp.theta_scale = powf(freq_base, -2.0f / rp.n_dims);
    float cd[2];
    rope_corr_dims(rp.n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow, cd);
    rp.corr0 = cd[0];
    rp.corr1 = cd[1];
    return rp;
}

// ------------------------------------------------------------------------------------------------ the executor

// the operands of an entry point under their own names, and its scalar arguments
struct GlueArgs {
    const qmm_tensor * a = nullptr, * b = nullptr, * c = nullptr, * d = nullptr;      // qmm_op_compute: sources and destination; d: every add + norm's normed result too
    const qmm_tensor * w = nullptr, * sum = nullptr;                                     // the weight row of a norm; the sum an add + norm also stores
    const qmm_tensor * q = nullptr, * pos = nullptr, * ff = nullptr, * qd = nullptr, * k = nullptr, * kd = nullptr, * v = nullptr, * vd = nullptr;       // qmm_rope_kv_store
    const qmm_tensor * gate_inp = nullptr, * logits = nullptr, * ids = nullptr, * weights = nullptr, * normed = nullptr;     // the routers; weights: the combines' too
    const qmm_tensor * x = nullptr;                                                      // the routers' activations; the combines' expert outputs
    float eps = 0.0f;
    int   n_used = 0, normalise = 0;
};

template <typename T> T * data_of(const qmm_tensor * t) { return t ? (T *) t->data : nullptr; }

// launches a plan of qmm_glue_plan.h: the refusal, the trace label, then the one launch of the plan's kernel family with the
// instantiation its template arguments name.  Every instantiation the library holds is named in one of the tables here
int run_glue(qmm_ctx * ctx, hipStream_t st, const GluePlan & p, const GlueArgs & g) {
    if (p.err) return fail(p.err, "%s", p.msg);
    if (p.label) QMM_TRACE(ctx, p.label, p.targ[0]);
    if (!p.launch) return QMM_OK;
    const dim3 grid(p.grid[0], p.grid[1], p.grid[2]), block(p.block);
    const int * const t = p.targ;
    switch (p.kernel) {
        case GK_BINARY: {
            static const decltype(&binary_kernel<QMM_OP_ADD, false>) K[4][2] = {
                { binary_kernel<QMM_OP_ADD, false>, binary_kernel<QMM_OP_ADD, true> }, { binary_kernel<QMM_OP_SUB, false>, binary_kernel<QMM_OP_SUB, true> },
                { binary_kernel<QMM_OP_MUL, false>, binary_kernel<QMM_OP_MUL, true> }, { binary_kernel<QMM_OP_DIV, false>, binary_kernel<QMM_OP_DIV, true> } };
            hipLaunchKernelGGL((K[t[0] - QMM_OP_ADD][t[1]]), grid, block, p.lds, st, data_of<const char>(g.a), data_of<const char>(g.b), data_of<char>(g.d),
                               shape_of(g.a), shape_of(g.b), shape_of(g.d), (uint32_t) nrows(g.d));
            break;
        }
        case GK_UNARY: {
            static const decltype(&unary_kernel<QMM_OP_SCALE, false>) K[9] = {
                unary_kernel<QMM_OP_SCALE, false>, unary_kernel<QMM_OP_SILU, false>, unary_kernel<QMM_OP_GELU, false>, unary_kernel<QMM_OP_GELU_QUICK, false>,
                unary_kernel<QMM_OP_RELU, false>, unary_kernel<QMM_OP_TANH, false>, unary_kernel<QMM_OP_SIGMOID, false>, unary_kernel<QMM_OP_NEG, false>,
                unary_kernel<QMM_OP_EXP, false> };
            hipLaunchKernelGGL((t[1] ? unary_kernel<QMM_OP_SILU, true> : K[t[0] - QMM_OP_SCALE]), grid, block, p.lds, st, data_of<const float>(g.a),
                               t[1] ? data_of<const float>(g.b) : nullptr, data_of<float>(g.d), (uint32_t) nelements(g.d), t[0] == QMM_OP_SCALE ? f32_param(g.d, 0) : 0.0f);
            break;
        }
        case GK_RMS_NORM:
            hipLaunchKernelGGL((t[0] ? rms_norm_kernel<true> : rms_norm_kernel<false>), grid, block, p.lds, st, data_of<const char>(g.a), data_of<const float>(g.w),
                               data_of<char>(g.d), shape_of(g.a), shape_of(g.d), g.eps);
            break;
        case GK_RMS_NORM_VEC: {
            static const decltype(&rms_norm_vec_kernel<false, false, 256>) K[2][2][2] = {
                { { rms_norm_vec_kernel<false, false, 256>, rms_norm_vec_kernel<false, false, 1024> }, { rms_norm_vec_kernel<false, true, 256>, rms_norm_vec_kernel<false, true, 1024> } },
                { { rms_norm_vec_kernel<true, false, 256>, rms_norm_vec_kernel<true, false, 1024> }, { rms_norm_vec_kernel<true, true, 256>, rms_norm_vec_kernel<true, true, 1024> } } };
            hipLaunchKernelGGL((K[t[0]][t[1]][t[2] == 1024]), grid, block, p.lds, st, data_of<const char>(g.a), data_of<const char>(g.b), data_of<const float>(g.w),
                               data_of<char>(g.d), data_of<char>(g.sum), shape_of(g.a), shape_of(g.b ? g.b : g.a), shape_of(g.d), shape_of(g.sum ? g.sum : g.d), g.eps);
            break;
        }
        case GK_NORM:
            hipLaunchKernelGGL((norm_kernel), grid, block, p.lds, st, data_of<const char>(g.a), data_of<char>(g.d), shape_of(g.a), shape_of(g.d), g.eps);
            break;
        case GK_SOFT_MAX_WAVE:
            hipLaunchKernelGGL((t[0] == 1 ? soft_max_wave_kernel<1> : t[0] == 2 ? soft_max_wave_kernel<2> : soft_max_wave_kernel<4>), grid, block, p.lds, st,
                               data_of<const float>(g.a), data_of<const float>(g.b), data_of<float>(g.d), (uint32_t) g.a->ne[0], (uint32_t) g.a->ne[1],
                               (uint32_t) nrows(g.d), f32_param(g.d, 0));
            break;
        case GK_SOFT_MAX: {
            const float max_bias = f32_param(g.d, 1);
            const uint32_t n_head_log2 = 1u << (uint32_t) floor(log2((double) (uint32_t) g.a->ne[2]));
            const float m0 = powf(2.0f, -(max_bias) / n_head_log2), m1 = powf(2.0f, -(max_bias / 2.0f) / n_head_log2);
            hipLaunchKernelGGL((t[0] ? soft_max_kernel<true> : soft_max_kernel<false>), grid, block, p.lds, st, data_of<const float>(g.a), data_of<const void>(g.b),
                               data_of<float>(g.d), (uint32_t) g.a->ne[0], (uint32_t) g.a->ne[1], (uint32_t) g.a->ne[2], f32_param(g.d, 0), max_bias, m0, m1, n_head_log2);
            break;
        }
        case GK_ROPE:
            hipLaunchKernelGGL((rope_kernel), grid, block, p.lds, st, data_of<const char>(g.a), data_of<const int32_t>(g.b), data_of<const float>(g.c), data_of<char>(g.d),
                               shape_of(g.a), shape_of(g.d), rope_params(g.d), (uint32_t) (nelements(g.d) / 2));
            break;
        case GK_MEMCPY:
            HIP_TRY(hipMemcpyAsync(g.d->data, g.a->data, (size_t) nelements(g.a) * esize(g.a->type), hipMemcpyDeviceToDevice, st));
            return QMM_OK;
        case GK_CPY: {
            static const decltype(&cpy_kernel<float, float>) K[2][2] = { { cpy_kernel<float, float>, cpy_kernel<float, __half> }, { cpy_kernel<__half, float>, cpy_kernel<__half, __half> } };
            hipLaunchKernelGGL((K[t[0] == G_F16][t[1] == G_F16]), grid, block, p.lds, st, data_of<const char>(g.a), data_of<char>(g.d), shape_of(g.a), shape_of(g.d),
                               (uint32_t) nelements(g.a));
            break;
        }
        case GK_CPY_TRANSPOSE: {
            static const decltype(&cpy_transpose_kernel<float, float>) K[2][2] = { { cpy_transpose_kernel<float, float>, cpy_transpose_kernel<float, __half> },
                                                                                  { cpy_transpose_kernel<__half, float>, cpy_transpose_kernel<__half, __half> } };
            hipLaunchKernelGGL((K[t[0] == G_F16][t[1] == G_F16]), grid, block, p.lds, st, data_of<const char>(g.a), data_of<char>(g.d), (uint32_t) g.a->ne[0],
                               (uint32_t) g.a->ne[1], g.a->nb[0], g.d->nb[1]);
            break;
        }
        case GK_GET_ROWS:
            hipLaunchKernelGGL((t[0] == G_F16 ? get_rows_kernel<__half> : get_rows_kernel<float>), grid, block, p.lds, st, data_of<const char>(g.a), data_of<const char>(g.b),
                               data_of<char>(g.d), shape_of(g.a), shape_of(g.b), shape_of(g.d));
            break;
        case GK_GET_ROWS_Q: {
            decltype(&get_rows_q_kernel<T_Q4_0>) kern;
#define QMM_X(TT) kern = get_rows_q_kernel<TT>; break
            QMM_FOR_TYPE(t[0], QMM_X)
#undef QMM_X
            hipLaunchKernelGGL((kern), grid, block, p.lds, st, data_of<const uint8_t>(g.a), data_of<const char>(g.b), data_of<char>(g.d), shape_of(g.a), shape_of(g.b),
                               shape_of(g.d));
            break;
        }
        case GK_MUL_MAT_F16:
        case GK_MUL_MAT_DOT_BLOCK:
        case GK_MUL_MAT_DOT: {
            const qmm_tensor * a = g.a, * b = g.b, * d = g.d;
            MmArgs m;
            m.a = (const char *) a->data;  m.b = (const char *) b->data;  m.d = (char *) d->data;
            m.a_nb1 = a->nb[1]; m.a_nb2 = a->nb[2]; m.a_nb3 = a->nb[3];
            m.b_nb1 = b->nb[1]; m.b_nb2 = b->nb[2]; m.b_nb3 = b->nb[3];
            m.d_nb1 = d->nb[1]; m.d_nb2 = d->nb[2]; m.d_nb3 = d->nb[3];
            m.M = (int32_t) a->ne[1]; m.N = (int32_t) b->ne[1]; m.K = (int32_t) a->ne[0];
            m.ne12 = (int32_t) b->ne[2]; m.r2 = (int32_t) (b->ne[2] / a->ne[2]); m.r3 = (int32_t) (b->ne[3] / a->ne[3]);
            hipLaunchKernelGGL((p.kernel == GK_MUL_MAT_DOT_BLOCK ? mul_mat_dot_block_kernel : p.kernel == GK_MUL_MAT_DOT ? mul_mat_dot_kernel<float> :
                               t[0] ? mul_mat_f16_kernel<true> : mul_mat_f16_kernel<false>), grid, block, p.lds, st, m);
            break;
        }
        case GK_ARGSORT:
            hipLaunchKernelGGL((argsort_kernel), grid, block, p.lds, st, data_of<const char>(g.a), data_of<char>(g.d), shape_of(g.a), shape_of(g.d), g.d->op_params[0]);
            break;
        case GK_SUM_ROWS:
            hipLaunchKernelGGL((sum_rows_kernel), grid, block, p.lds, st, data_of<const char>(g.a), data_of<char>(g.d), shape_of(g.a), shape_of(g.d), (uint32_t) nrows(g.a));
            break;
        case GK_ROPE_STORE: {
            RopeStoreArgs r;
            r.q = data_of<const char>(g.q); r.qd = data_of<char>(g.qd); r.sq = shape_of(g.q); r.sqd = shape_of(g.qd);
            r.k = data_of<const char>(g.k); r.kd = data_of<char>(g.k ? g.kd : nullptr); r.sk = shape_of(g.k ? g.k : g.q); r.skd = shape_of(g.k ? g.kd : g.qd);
            r.v = data_of<const char>(g.v); r.vd = data_of<char>(g.v ? g.vd : nullptr); r.sv = shape_of(g.v ? g.v : g.q); r.svd = shape_of(g.v ? g.vd : g.qd);
            r.pos = data_of<const int32_t>(g.pos); r.ff = data_of<const float>(g.ff);
            r.rp = rope_params(g.qd);
            r.nq = rope_heads_threads(g.q); r.nk = g.k ? rope_heads_threads(g.k) : 0; r.nv = g.v ? (uint32_t) nelements(g.v) : 0;
            hipLaunchKernelGGL((t[0] ? rope_store_kernel<true> : rope_store_kernel<false>), grid, block, p.lds, st, r, p.karg[0], p.karg[1]);
            break;
        }
        case GK_MOE_ROUTER:
            hipLaunchKernelGGL((moe_router_kernel), grid, block, p.lds, st, data_of<const char>(g.logits), data_of<char>(g.ids), data_of<char>(g.weights), g.logits->nb[1], g.ids->nb[1],
                               (int64_t) g.n_used * 4, (int) g.logits->ne[0], g.n_used, (int) g.logits->ne[1], g.normalise);
            break;
        case GK_MOE_ROUTER_LOGITS:
            hipLaunchKernelGGL((t[0] ? moe_router_logits_kernel<true> : moe_router_logits_kernel<false>), grid, block, p.lds, st, data_of<const char>(g.gate_inp), data_of<const char>(g.x),
                               data_of<char>(g.logits), data_of<char>(g.ids), data_of<char>(g.weights), g.gate_inp->nb[1], g.x->nb[1], g.logits->nb[1], g.ids->nb[1], (int64_t) g.n_used * 4,
                               (int) g.gate_inp->ne[0], (int) g.logits->ne[0], g.n_used, g.normalise, data_of<const float>(g.w), g.eps, data_of<char>(g.normed), g.normed ? g.normed->nb[1] : (int64_t) 0);
            break;
        case GK_MOE_COMBINE:
            hipLaunchKernelGGL((moe_combine_kernel), grid, block, p.lds, st, data_of<const char>(g.x), data_of<const char>(g.weights), data_of<char>(g.d), g.x->nb[1], g.x->nb[2],
                               g.weights->nb[1], g.weights->nb[2], g.d->nb[1], (int) g.x->ne[0], (int) g.x->ne[1]);
            break;
        case GK_MOE_COMBINE_ADD_NORM:
            hipLaunchKernelGGL((t[0] == 1024 ? moe_combine_add_norm_kernel<1024> : moe_combine_add_norm_kernel<256>), grid, block, p.lds, st, data_of<const char>(g.x),
                               data_of<const char>(g.weights), data_of<const char>(g.b), data_of<const float>(g.w), data_of<char>(g.d), data_of<char>(g.sum), g.x->nb[1], g.x->nb[2],
                               g.weights->nb[1], g.weights->nb[2], g.b->nb[1], g.d->nb[1], g.sum->nb[1], (int) g.x->ne[0], (int) g.x->ne[1], g.eps);
            break;
        default: return fail(QMM_EUNSUPPORTED, "glue ops: no kernel for plan %d", p.kernel);
    }
    HIP_TRY(hipGetLastError());
    return QMM_OK;
}

} // namespace

// qmm_set_codebook (qmm_api.hip) writes every code object's tables (IQ3, IQ2 and the IQ1 grid alike): this one's serves get_rows_q_kernel
int qmm_internal_ops_codebook(int type, const uint32_t * entries, int n) {
    HIP_TRY(codebook_upload(type, entries, n));
    return QMM_OK;
}

#include "qmm_attn.hiph"         // the attention kernels, their launch executor and entry points
#include "qmm_kcache.hiph"       // a Q8_0 K cache: CPY into and out of block_q8_0 rows, attention on them (what runs: qmm_kcache_plan.h)
#include "qmm_kblk.hiph"         // a K cache in Q4_0 / Q4_1 / Q5_0 / Q5_1: the same surface on those blocks (what runs: qmm_kblk_plan.h)
#include "qmm_ropekq.hiph"       // rope(q), rope(k) into a K cache of any of those five block types and the V store as one launch (what runs: qmm_ropekq_plan.h)

extern "C" {

int qmm_op_supported(int op, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * c, const qmm_tensor * d) {
    if (op == QMM_OP_CPY && kq8_cpy_case(a, d)) return kq8_takes_cpy(a, d);
    if (op == QMM_OP_CPY && kblk_cpy_case(a, d)) return kblk_takes_cpy(a, d);
    return sup_op(op, a, b, c, d);
}

int qmm_op_compute(qmm_ctx * ctx, int op, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * c, const qmm_tensor * d, void * stream) {
    if (!ctx || !d) return fail(QMM_EINVAL, "qmm_op_compute: NULL context or dst");
    if (op == QMM_OP_CPY && kq8_cpy_case(a, d)) return kq8_cpy(ctx, a, d, stream);
    if (op == QMM_OP_CPY && kblk_cpy_case(a, d)) return kblk_cpy(ctx, a, d, stream);
    if (!sup_op(op, a, b, c, d)) return fail(QMM_EUNSUPPORTED, "qmm_op_compute: op %d with these types / shapes / strides is not implemented", op);
    if (op == QMM_OP_GET_ROWS) { const int rc = need_codebook(ctx, a->type, "qmm_op_compute(GET_ROWS)"); if (rc) return rc; }
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.a = a; g.b = b; g.c = c; g.d = d;
    if (op == QMM_OP_NORM || op == QMM_OP_RMS_NORM || op == QMM_OP_RMS_NORM_MUL) {
        g.eps = f32_param(d, 0);
        if (g.eps < 0.0f) return fail(QMM_EINVAL, op == QMM_OP_NORM ? "NORM: eps < 0" : "RMS_NORM: eps < 0");
        g.w = op == QMM_OP_RMS_NORM_MUL ? b : nullptr;
        g.b = nullptr;
    }
    return run_glue(ctx, ctx->s(stream), glue_op_plan(op, a, b, c, d), g);
}

int qmm_op_add_rms_norm_supported(const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * sum, const qmm_tensor * dst) {
    return sup_add_rms_norm(a, b, w, sum, dst);
}

int qmm_op_add_rms_norm(qmm_ctx * ctx, const qmm_tensor * a, const qmm_tensor * b, const qmm_tensor * w, const qmm_tensor * sum,
                        const qmm_tensor * dst, float eps, void * stream) {
    if (!ctx || !sup_add_rms_norm(a, b, w, sum, dst)) return fail(QMM_EUNSUPPORTED, "qmm_op_add_rms_norm: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    if (eps < 0.0f) return fail(QMM_EINVAL, "RMS_NORM: eps < 0");
    GlueArgs g;
    g.a = a; g.b = b; g.w = w; g.sum = sum; g.d = dst; g.eps = eps;
    return run_glue(ctx, ctx->s(stream), glue_add_rms_norm_plan(a, b, w, sum, dst), g);
}

int qmm_rope_kv_store_supported(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                                const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst) {
    return sup_rope_kv_store(q, pos, ff, q_dst, k, k_dst, v, v_dst);
}

int qmm_rope_kv_store(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                      const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst, void * stream) {
    if (!ctx || !sup_rope_kv_store(q, pos, ff, q_dst, k, k_dst, v, v_dst)) return fail(QMM_EUNSUPPORTED, "qmm_rope_kv_store: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.q = q; g.pos = pos; g.ff = ff; g.qd = q_dst; g.k = k; g.kd = k_dst; g.v = v; g.vd = v_dst;
    return run_glue(ctx, ctx->s(stream), glue_rope_kv_store_plan(q, k, v, v_dst), g);
}

int qmm_rope_kq_store_supported(const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                                const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst) {
    return ropekq_takes_store(q, pos, ff, q_dst, k, k_dst, v, v_dst);
}

int qmm_rope_kq_store(qmm_ctx * ctx, const qmm_tensor * q, const qmm_tensor * pos, const qmm_tensor * ff, const qmm_tensor * q_dst,
                      const qmm_tensor * k, const qmm_tensor * k_dst, const qmm_tensor * v, const qmm_tensor * v_dst, void * stream) {
    if (!ctx || !ropekq_takes_store(q, pos, ff, q_dst, k, k_dst, v, v_dst)) return fail(QMM_EUNSUPPORTED, "qmm_rope_kq_store: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    return ropekq_store(ctx, ctx->s(stream), q, pos, ff, q_dst, k, k_dst, v, v_dst);
}

int qmm_moe_router_supported(const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used) {
    return sup_moe_router(logits, ids, weights, n_used);
}

int qmm_moe_router(qmm_ctx * ctx, const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used, int normalise,
                   void * stream) {
    if (!ctx || !sup_moe_router(logits, ids, weights, n_used)) return fail(QMM_EUNSUPPORTED, "qmm_moe_router: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.logits = logits; g.ids = ids; g.weights = weights; g.n_used = (int) n_used; g.normalise = normalise;
    return run_glue(ctx, ctx->s(stream), glue_moe_router_plan(logits), g);
}

int qmm_moe_router_logits_supported(const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * logits, const qmm_tensor * ids,
                                    const qmm_tensor * weights, int64_t n_used) {
    return sup_moe_router_logits(gate_inp, x, logits, ids, weights, n_used);
}

int qmm_moe_router_logits(qmm_ctx * ctx, const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * logits, const qmm_tensor * ids,
                          const qmm_tensor * weights, int64_t n_used, int normalise, void * stream) {
    if (!ctx || !sup_moe_router_logits(gate_inp, x, logits, ids, weights, n_used))
        return fail(QMM_EUNSUPPORTED, "qmm_moe_router_logits: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.gate_inp = gate_inp; g.x = x; g.logits = logits; g.ids = ids; g.weights = weights; g.n_used = (int) n_used; g.normalise = normalise;
    return run_glue(ctx, ctx->s(stream), glue_moe_router_logits_plan(x, false), g);
}

int qmm_moe_router_logits_norm_supported(const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * norm_w, const qmm_tensor * normed,
                                         const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used) {
    return sup_moe_router_logits_norm(gate_inp, x, norm_w, normed, logits, ids, weights, n_used);
}

int qmm_moe_router_logits_norm(qmm_ctx * ctx, const qmm_tensor * gate_inp, const qmm_tensor * x, const qmm_tensor * norm_w, float eps, const qmm_tensor * normed,
                               const qmm_tensor * logits, const qmm_tensor * ids, const qmm_tensor * weights, int64_t n_used, int normalise, void * stream) {
    if (!ctx || eps < 0.0f || !sup_moe_router_logits_norm(gate_inp, x, norm_w, normed, logits, ids, weights, n_used))
        return fail(QMM_EUNSUPPORTED, "qmm_moe_router_logits_norm: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.gate_inp = gate_inp; g.x = x; g.logits = logits; g.normed = normed; g.w = norm_w; g.eps = eps; g.ids = ids; g.weights = weights; g.n_used = (int) n_used; g.normalise = normalise;
    return run_glue(ctx, ctx->s(stream), glue_moe_router_logits_plan(x, true), g);
}

int qmm_moe_combine_supported(const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * out) { return sup_moe_combine(x, w, out); }

int qmm_moe_combine(qmm_ctx * ctx, const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * out, void * stream) {
    if (!ctx || !sup_moe_combine(x, w, out)) return fail(QMM_EUNSUPPORTED, "qmm_moe_combine: operands not supported");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.x = x; g.weights = w; g.d = out;
    return run_glue(ctx, ctx->s(stream), glue_moe_combine_plan(x, out), g);
}

int qmm_moe_combine_add_rms_norm_supported(const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * b, const qmm_tensor * nw, const qmm_tensor * sum,
                                           const qmm_tensor * dst) {
    return sup_moe_combine_add_rms_norm(x, w, b, nw, sum, dst);
}

int qmm_moe_combine_add_rms_norm(qmm_ctx * ctx, const qmm_tensor * x, const qmm_tensor * w, const qmm_tensor * b, const qmm_tensor * nw, const qmm_tensor * sum,
                                 const qmm_tensor * dst, float eps, void * stream) {
    if (!ctx || !sup_moe_combine_add_rms_norm(x, w, b, nw, sum, dst)) return fail(QMM_EUNSUPPORTED, "qmm_moe_combine_add_rms_norm: operands not supported");
    if (eps < 0.0f) return fail(QMM_EINVAL, "qmm_moe_combine_add_rms_norm: eps < 0");
    HIP_TRY(hipSetDevice(ctx->device));
    QMM_CHAIN_FLUSH(ctx);
    GlueArgs g;
    g.x = x; g.weights = w; g.b = b; g.w = nw; g.sum = sum; g.d = dst; g.eps = eps;
    return run_glue(ctx, ctx->s(stream), glue_moe_combine_add_rms_norm_plan(x), g);
}

} // extern "C"
