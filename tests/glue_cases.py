"""The cases of tests/test_gpu_glue_ops.py: for every branch of the launch plan csrc/qmm_glue_plan.h the smallest operands that reach it.
Each case is built on the CPU (operands as glue_refs.Buf, the float64 reference, the float32 restatement, the trace label it must
take); tests/test_glue_refs.py checks the restatements on the CPU, tests/test_gpu_glue_ops.py runs the kernels.  A plain module."""
import zlib

import numpy as np

import glue_refs as R
from glue_refs import F16, F32, I32, Buf, f32, f64

# enum qmm_op (include/ggml_mi355x_ops.h)
(OP_ADD, OP_SUB, OP_MUL, OP_DIV, OP_SCALE, OP_SILU, OP_GELU, OP_GELU_QUICK, OP_RELU, OP_TANH, OP_SIGMOID, OP_NEG, OP_EXP, OP_RMS_NORM,
 OP_ROPE, OP_SOFT_MAX, OP_CPY, OP_GET_ROWS, OP_MUL_MAT_F, OP_RMS_NORM_MUL, OP_SILU_MUL, OP_ARGSORT, OP_SUM_ROWS, OP_NORM) = range(1, 25)
OP_ADD_RMS_NORM = 100            # qmm_op_add_rms_norm, its own entry point

FLOOR = 2e-6                     # the per-element bar never drops below this (test_add_rms_norm_two_results' bar)


def f2i(x):
    return int(f32(x).view(np.int32))


def nbytes_of(ne, es=4, pad1=0, pad2=0):
    """byte strides of a tensor whose rows are pad1 bytes and whose planes are pad2 bytes further apart than dense"""
    ne = list(ne) + [1] * (4 - len(ne))
    nb1 = ne[0] * es + pad1
    nb2 = nb1 * ne[1] + pad2
    return [es, nb1, nb2, nb2 * ne[2]]


class Case:
    """op, operands and what the launch must give.  want: float64 reference (or the exact array when exact); rest: the float32
    restatement; extra: a derived addition to the per-element bound (with its derivation where it is set)"""

    def __init__(self, op, label, dst, src0=None, src1=None, src2=None, params=(), want=None, rest=None, exact=False, extra=0.0,
                 sum_=None, want_sum=None, eps=0.0, untouched=None, shape=""):
        self.op, self.label, self.dst, self.src = op, label, dst, (src0, src1, src2)
        self.params, self.want, self.rest, self.exact, self.extra = tuple(params), want, rest, exact, extra
        self.sum, self.want_sum, self.eps = sum_, want_sum, eps
        self.untouched = untouched            # boolean array over dst's values: elements the launch must leave as they were
        self.shape = shape

    def bound(self):
        """per-element bar: 4 x the restatement's own rel_rms against the float64 reference, at least FLOOR, plus the derived extra"""
        return max(4.0 * R.rel_rms(self.rest, self.want), FLOOR) + self.extra


CASES = []                       # (id, builder)


def rng_of(id_):
    return np.random.default_rng(zlib.crc32(id_.encode()))


def reg(id_, fn, *args, **kw):
    CASES.append((id_, lambda: fn(rng_of(id_), *args, **kw)))


# ------------------------------------------------------------------------------------------------ binary
BIN = {"add": OP_ADD, "sub": OP_SUB, "mul": OP_MUL, "div": OP_DIV}


def binary_case(rng, op, ne, bne=None, a_pad=0, b_pad=0, d_pad=0, off=0, in_place=False, label="vec"):
    ne = list(ne) + [1] * (4 - len(ne))
    bne = list(bne or ne) + [1] * (4 - len(bne or ne))
    a = Buf(F32, ne, nbytes_of(ne, 4, a_pad), off=off, seed=1).put(rng.normal(0, 2, ne[::-1]))
    bv = rng.normal(0, 2, bne[::-1])
    if op == "div":
        bv = np.where(np.abs(bv) < 0.1, 0.5, bv)
    b = Buf(F32, bne, nbytes_of(bne, 4, b_pad), off=off, seed=2).put(bv)
    d = Buf(F32, ne, a.nb, off=off, share=a) if in_place else Buf(F32, ne, nbytes_of(ne, 4, d_pad), off=off, seed=3)
    want = R.binary(op, a.values(), b.values(), f32)
    return Case(BIN[op], f"binary_kernel<{label}>", d, a, b, want=want, exact=True, shape=f"{ne} b{bne} pad{a_pad}/{b_pad}/{d_pad} off{off}")


for _op in BIN:
    reg(f"{_op}-1028-vec", binary_case, _op, [1028, 3])
    reg(f"{_op}-1027-scalar", binary_case, _op, [1027, 3], label="scalar")
reg("add-400x5-vec", binary_case, "add", [400, 5])
reg("mul-100x5-scalar-idle", binary_case, "mul", [100, 5], a_pad=4, d_pad=4, label="scalar")        # rows 4-byte aligned only
reg("sub-516x3-scalar", binary_case, "sub", [516, 3], bne=[1, 3], label="scalar")
reg("div-400x5x3-b-ne0-1-ne2-1", binary_case, "div", [400, 5, 3, 2], bne=[400, 1, 3, 1])
reg("mul-bcast-1-ne1", binary_case, "mul", [400, 5, 3], bne=[1, 5, 1, 1], label="scalar")
reg("add-bcast-scalar", binary_case, "add", [1028, 3, 2], bne=[1, 1, 1, 1], label="scalar")
reg("add-rowview-16", binary_case, "add", [400, 5], a_pad=16, b_pad=32, d_pad=48)
reg("add-rowview-4", binary_case, "add", [400, 5], a_pad=4, label="scalar")
reg("mul-ptr-off-4", binary_case, "mul", [1028, 3], off=4, label="scalar")
reg("add-4d-ragged-rows", binary_case, "add", [100, 3, 5, 3], label="vec")              # 45 rows, 10 rows per block
reg("sub-4d-ragged-rows-scalar", binary_case, "sub", [99, 3, 5, 3], label="scalar")     # 45 rows, 2 rows per block
reg("add-in-place", binary_case, "add", [400, 5], in_place=True)
reg("div-in-place-scalar", binary_case, "div", [100, 5], in_place=True, a_pad=4, label="scalar")

# ------------------------------------------------------------------------------------------------ unaries, SCALE, SILU_MUL
UNA = {"scale": OP_SCALE, "silu": OP_SILU, "gelu": OP_GELU, "gelu_quick": OP_GELU_QUICK, "relu": OP_RELU, "tanh": OP_TANH, "sigmoid": OP_SIGMOID,
       "neg": OP_NEG, "exp": OP_EXP}
SPECIAL = np.array([0.0, -0.0, 20.0, -20.0, 1e-3, -1e-3], np.float32)


def unary_values(rng, name, n):
    x = rng.uniform(-20, 20, n).astype(f32)
    k = min(n, len(SPECIAL))
    x[:k] = SPECIAL[:k]
    # saturation: exp(88) is finite in f32, exp(-88) is below the normal range.  For EXP in one size only: exp(88) is the whole rms of its
    # case, and the per-element bar, which is relative to the rms, says little about the other elements there
    if name in ("sigmoid", "silu") and n > 8 or name == "exp" and n == 1023:
        x[6], x[7] = 88.0, -88.0
    return x


def unary_case(rng, name, n, off=0, in_place=False):
    a = Buf(F32, [n], off=off, seed=1).put(unary_values(rng, name, n))
    d = Buf(F32, [n], off=off, share=a) if in_place else Buf(F32, [n], off=off, seed=3)
    p = 0.37 if name == "scale" else None
    x = a.values()
    if name in ("neg", "relu", "scale"):
        return Case(UNA[name], "unary_kernel", d, a, params=(f2i(p),) if p else (), want=R.unary(name, x, p, f32), exact=True, shape=f"n={n} off{off}")
    want, extra = R.unary(name, x, p), 0.0
    if name == "exp":
        # exp over [-20, 20] (and 88) spans so many decades that the few largest outputs are the whole rms: the restatement's figure is
        # then the rounding luck of those few values (anything from 0 to half an ulp where numpy rounds correctly), while a device expf is
        # specified to 1 ulp.  One ulp of the largest output is added to the bar
        extra = float(2.0 ** -23 * np.abs(want).max() / np.sqrt(np.mean(want ** 2)))
    return Case(UNA[name], "unary_kernel", d, a, want=want, rest=R.unary(name, x, p, f32), extra=extra, shape=f"n={n} off{off}")


def silu_mul_case(rng, n, off=0):
    a = Buf(F32, [n], off=off, seed=1).put(unary_values(rng, "silu", n))
    b = Buf(F32, [n], off=off, seed=2).put(rng.normal(0, 1, n))
    d = Buf(F32, [n], off=off, seed=3)
    return Case(OP_SILU_MUL, "unary_kernel", d, a, b, want=R.silu_mul(a.values(), b.values()), rest=R.silu_mul(a.values(), b.values(), f32), shape=f"n={n} off{off}")


for _name in UNA:
    for _n in (1, 3, 4, 1023, 1024, 1029):
        reg(f"{_name}-{_n}", unary_case, _name, _n)
    reg(f"{_name}-1029-ptr-off-4", unary_case, _name, 1029, off=4)
reg("silu-1029-in-place", unary_case, "silu", 1029, in_place=True)
for _n in (1, 3, 4, 1023, 1024, 1029):
    reg(f"silu_mul-{_n}", silu_mul_case, _n)
reg("silu_mul-1029-ptr-off-4", silu_mul_case, 1029, off=4)

# ------------------------------------------------------------------------------------------------ RMS_NORM, NORM
def rms_case(rng, rows, ne0, weight=False, add=False, eps=1e-6, pad=0, label=None, in_place=False, ne=None, zero_row=False):
    ne = ne or [ne0, rows]
    shape = (list(ne) + [1] * (4 - len(ne)))[::-1]
    xv = rng.normal(0, 1.5, shape).astype(f32)
    if zero_row:
        xv.reshape(-1, ne0)[0] = 0
    nb = nbytes_of(ne, 4, pad)
    a = Buf(F32, ne, nb, seed=1).put(xv)
    w = Buf(F32, [ne0], seed=2).put(rng.normal(1, 0.2, ne0)) if weight else None
    wv = w.values().reshape(-1) if weight else None
    if add:
        b = Buf(F32, ne, nb, seed=4).put(rng.normal(0, 1, shape))
        s = Buf(F32, ne, nb, share=a) if in_place else Buf(F32, ne, nb, seed=5)
        d = Buf(F32, ne, nb, seed=3)
        want, ws = R.rms_norm(a.values(), eps, wv, b.values())
        return Case(OP_ADD_RMS_NORM, label, d, a, b, w, want=want, rest=R.rms_norm_f32(a.values(), eps, wv, b.values()), sum_=s, want_sum=ws, eps=eps,
                    shape=f"{rows}x{ne0} w{int(weight)} eps{eps} pad{pad}")
    d = Buf(F32, ne, nb, share=a) if in_place else Buf(F32, ne, nb, seed=3)
    return Case(OP_RMS_NORM_MUL if weight else OP_RMS_NORM, label, d, a, w, params=(f2i(eps),), want=R.rms_norm(a.values(), eps, wv),
                rest=R.rms_norm_f32(a.values(), eps, wv), shape=f"{rows}x{ne0} w{int(weight)} eps{eps} pad{pad}")


V1024, V256, SCAL = "rms_norm_vec_kernel<1024>", "rms_norm_vec_kernel<256>", "rms_norm_kernel"
for _rows, _ne0, _label in ((3, 4, V1024), (3, 4096, V1024), (256, 4096, V256), (256, 1028, V256), (256, 4100, V1024), (2, 16384, V1024),
                            (2, 16388, SCAL), (3, 2047, SCAL), (3, 2049, SCAL), (5, 1, SCAL)):
    for _w in (False, True):
        reg(f"rms_norm-{_rows}x{_ne0}-w{int(_w)}", rms_case, _rows, _ne0, weight=_w, label=_label)
    if _label != SCAL:
        reg(f"add_rms_norm-{_rows}x{_ne0}", rms_case, _rows, _ne0, weight=True, add=True, label=_label)
reg("rms_norm-3x2048-vec", rms_case, 3, 2048, weight=True, label=V1024)
reg("rms_norm-3x2048-scalar-rowview-4", rms_case, 3, 2048, weight=True, pad=4, label=SCAL)          # ne0 == 256 * 8: the last row length kept in registers
reg("rms_norm-3x2048-scalar-rowview-4-w0", rms_case, 3, 2048, pad=4, label=SCAL)
reg("rms_norm-4d", rms_case, 30, 260, weight=True, ne=[260, 2, 5, 3], label=V1024)
reg("rms_norm-4d-scalar", rms_case, 30, 259, weight=True, ne=[259, 2, 5, 3], label=SCAL)
reg("rms_norm-strided-rows", rms_case, 7, 1028, weight=True, pad=48, label=V1024)
reg("rms_norm-eps0", rms_case, 3, 4096, eps=0.0, label=V1024)
reg("rms_norm-eps0-scalar", rms_case, 3, 2047, eps=0.0, weight=True, label=SCAL)
reg("rms_norm-zero-row", rms_case, 3, 1028, zero_row=True, label=V1024)
reg("rms_norm-zero-row-scalar", rms_case, 3, 1027, zero_row=True, label=SCAL)
reg("rms_norm-in-place", rms_case, 3, 4096, weight=True, in_place=True, label=V1024)
reg("rms_norm-in-place-scalar", rms_case, 2, 16388, in_place=True, label=SCAL)
reg("add_rms_norm-sum-in-place", rms_case, 3, 4096, weight=True, add=True, in_place=True, label=V1024)
reg("add_rms_norm-no-weight-strided", rms_case, 5, 1028, add=True, pad=16, label=V1024)
reg("add_rms_norm-256x1028-in-place", rms_case, 256, 1028, weight=True, add=True, in_place=True, label=V256)


def norm_case(rng, rows, ne0, kind="normal", pad=0, in_place=False):
    xv = rng.normal(0, 1.5, (rows, ne0)).astype(f32)
    if kind == "constant":
        xv[0] = 3.25                                         # centred values are exactly zero: y = 0 / sqrt(eps)
    if kind == "offset":
        xv = rng.normal(1000, 1, (rows, ne0)).astype(f32)
    a = Buf(F32, [ne0, rows], nbytes_of([ne0, rows], 4, pad), seed=1).put(xv)
    d = Buf(F32, [ne0, rows], a.nb, share=a) if in_place else Buf(F32, [ne0, rows], a.nb, seed=3)
    eps = 1e-5
    return Case(OP_NORM, "norm_kernel", d, a, params=(f2i(eps),), want=R.norm(a.values(), eps), rest=R.norm_f32(a.values(), eps), shape=f"{rows}x{ne0} {kind} pad{pad}")


for _ne0 in (64, 255, 256, 257, 5000):
    reg(f"norm-{_ne0}", norm_case, 3, _ne0)
reg("norm-1", norm_case, 5, 1)
reg("norm-constant-row", norm_case, 3, 257, kind="constant")
reg("norm-mean-1000", norm_case, 3, 5000, kind="offset")
reg("norm-strided-in-place", norm_case, 5, 257, pad=12, in_place=True)

# ------------------------------------------------------------------------------------------------ SOFT_MAX
def soft_max_case(rng, ne, label, mask=None, mask_rows=None, scale=1.0, max_bias=0.0, causal=False, in_place=False):
    ne = list(ne) + [1] * (4 - len(ne))
    nc, ne1 = ne[0], ne[1]
    a = Buf(F32, ne, seed=1).put(rng.normal(0, 2, ne[::-1]))
    m = None
    if mask is not None:
        mr = mask_rows or ne1
        mv = np.zeros((mr, nc), f32)
        if max_bias > 0:
            mv = -rng.integers(0, 8, (mr, nc)).astype(f32)                  # small integers: exact in f16, products with the slopes exact
        if causal:
            for i in range(mr):
                mv[i, 1 + (i * 7) % nc:] = -np.inf                          # a different prefix per row, column 0 always finite
        elif max_bias == 0:
            mv = rng.normal(0, 1, (mr, nc)).astype(np.float16).astype(f32)
        m = Buf(mask, [nc, mr], seed=2).put(mv)
    d = Buf(F32, ne, share=a) if in_place else Buf(F32, ne, seed=3)
    mvv = m.values()[0, 0] if m is not None else None
    want = R.soft_max(a.values(), mvv, scale, max_bias)
    rest = R.soft_max(a.values(), mvv, scale, max_bias, f32)
    return Case(OP_SOFT_MAX, label, d, a, m, params=(f2i(scale), f2i(max_bias)), want=want, rest=rest,
                shape=f"{ne} mask{mask} rows{mask_rows} scale{scale} bias{max_bias} causal{int(causal)}")


LDS, DST = "soft_max_kernel<lds>", "soft_max_kernel<dst>"
reg("soft_max-nc1", soft_max_case, [1, 5], LDS)
reg("soft_max-nc77-nomask", soft_max_case, [77, 5, 3], LDS, scale=0.1)
reg("soft_max-nc77-f32mask-causal", soft_max_case, [77, 5, 3], LDS, mask=F32, causal=True, scale=0.1)
reg("soft_max-nc77-f16mask-causal-more-rows", soft_max_case, [77, 5, 3], LDS, mask=F16, mask_rows=32, causal=True)
reg("soft_max-nc77-f16mask", soft_max_case, [77, 5, 3, 2], LDS, mask=F16, scale=0.1)
reg("soft_max-nc8192-lds", soft_max_case, [8192, 3], LDS, mask=F32)
reg("soft_max-nc8196-dst", soft_max_case, [8196, 3], DST, mask=F32, scale=0.1)
reg("soft_max-nc8196-dst-in-place-f16mask", soft_max_case, [8196, 2, 2], DST, mask=F16, in_place=True)
reg("soft_max-alibi-6-heads", soft_max_case, [77, 5, 6], LDS, mask=F32, max_bias=8.0, scale=0.1)
reg("soft_max-alibi-8-heads-f16", soft_max_case, [77, 5, 8, 2], LDS, mask=F16, max_bias=8.0, mask_rows=8)
reg("soft_max-rows1023-nc256-block", soft_max_case, [256, 341, 3], LDS, mask=F32, mask_rows=352)
reg("soft_max-rows1026-nc1028-block", soft_max_case, [1028, 171, 6], LDS, mask=F32, mask_rows=192, causal=True)
reg("soft_max-rows1026-nc256-f16mask-block", soft_max_case, [256, 171, 6], LDS, mask=F16, mask_rows=192)        # an f16 mask keeps the block kernel
reg("soft_max-in-place", soft_max_case, [77, 5, 3], LDS, mask=F32, in_place=True)
for _nc, _v in ((4, 1), (252, 1), (256, 1), (260, 2), (512, 2), (516, 4), (1020, 4), (1024, 4)):
    reg(f"soft_max-wave-nc{_nc}-mask", soft_max_case, [_nc, 171, 6], f"soft_max_wave_kernel<{_v}>", mask=F32, mask_rows=192, causal=True, scale=0.1)
    reg(f"soft_max-wave-nc{_nc}-nomask", soft_max_case, [_nc, 171, 6], f"soft_max_wave_kernel<{_v}>")
reg("soft_max-wave-in-place", soft_max_case, [260, 171, 6], "soft_max_wave_kernel<2>", mask=F32, mask_rows=192, in_place=True)

# ------------------------------------------------------------------------------------------------ ROPE
def rope_case(rng, ne0, n_dims, heads, pos, neox=False, ff=False, yarn=False, permuted=False, in_place=False):
    n_tok = len(pos)
    ne = [ne0, heads, n_tok, 1]
    kw = dict(freq_base=10000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0, n_ctx_orig=8192)
    if yarn:
        kw.update(freq_scale=0.25, ext_factor=1.0, attn_factor=1.25)
    xv = rng.normal(0, 1, ne[::-1]).astype(f32)
    if permuted:                                             # storage [heads][tokens][ne0], viewed as [ne0, heads, tokens]
        a = Buf(F32, ne, [4, n_tok * ne0 * 4, ne0 * 4, heads * n_tok * ne0 * 4], seed=1).put(xv)
    else:
        a = Buf(F32, ne, seed=1).put(xv)
    p = Buf(I32, [n_tok], seed=2).put(np.asarray(pos, np.int32))
    fv = rng.uniform(0.8, 4.0, n_dims // 2).astype(f32) if ff else None
    f = Buf(F32, [n_dims // 2], seed=4).put(fv) if ff else None
    d = Buf(F32, ne, a.nb, share=a) if in_place else Buf(F32, ne, seed=3)
    want = R.rope(a.values(), pos, n_dims, neox, ff=fv, **kw)
    rest = R.rope(a.values(), pos, n_dims, neox, dtype=f32, ff=fv, **kw)
    extra = 0.0
    if yarn:
        # th = interp * (1 - mix) + extrap * mix: a compiler may contract either product into the addition (ggml's CPU build and hipcc both do
        # by default), which moves the float32 angle by up to one ulp wherever 0 < mix < 1, and an output element by |x pair| * mscale * that.
        # Outside the ramp one product is exactly zero and nothing can move.
        th, mscale = R.rope_angles(pos, n_dims, ff=fv, **kw)
        c0, c1 = R.rope_corr_dims(n_dims, kw["n_ctx_orig"], kw["freq_base"], kw["beta_fast"], kw["beta_slow"])
        ramp = [q for q in range(n_dims // 2) if c0 < q < c1]
        ulp = float(np.max(np.spacing(np.abs(th[:, ramp])))) if ramp else 0.0
        extra = ulp * float(mscale) * float(np.sqrt(2.0) * np.abs(xv).max()) / float(np.sqrt(np.mean(want ** 2)))
    params = [0, n_dims, 2 if neox else 0, 0, kw["n_ctx_orig"], f2i(kw["freq_base"]), f2i(kw["freq_scale"]), f2i(kw["ext_factor"]), f2i(kw["attn_factor"]),
              f2i(kw["beta_fast"]), f2i(kw["beta_slow"])]
    return Case(OP_ROPE, "rope_kernel", d, a, p, f, params=params, want=want, rest=rest, extra=extra,
                shape=f"ne0={ne0} n_dims={n_dims} heads={heads} neox{int(neox)} ff{int(ff)} yarn{int(yarn)} perm{int(permuted)}")


POS = [0, 1, 4095, 100000]
reg("rope-normal-128", rope_case, 128, 128, 3, POS)                     # 768 pairs: three blocks
reg("rope-neox-128", rope_case, 128, 128, 3, POS, neox=True)
reg("rope-neox-80-ndims20", rope_case, 80, 20, 3, POS, neox=True)       # 480 pairs: not a multiple of 256
reg("rope-neox-80-ndims32", rope_case, 80, 32, 3, POS, neox=True)
reg("rope-normal-80-ndims32", rope_case, 80, 32, 3, POS)
reg("rope-normal-256-loop", rope_case, 256, 256, 2, POS)
reg("rope-neox-256-loop-ff", rope_case, 256, 256, 2, POS, neox=True, ff=True)
reg("rope-normal-ff", rope_case, 128, 128, 3, POS, ff=True)
reg("rope-normal-yarn", rope_case, 128, 128, 3, POS, yarn=True)
reg("rope-neox-yarn-ff", rope_case, 128, 64, 3, POS, neox=True, yarn=True, ff=True)
reg("rope-normal-permuted", rope_case, 128, 128, 3, POS, permuted=True)
reg("rope-normal-in-place", rope_case, 128, 128, 3, POS, in_place=True)
reg("rope-neox-in-place", rope_case, 80, 32, 3, POS, neox=True, in_place=True)

# ------------------------------------------------------------------------------------------------ CPY
def permuted_nb(ne, es, perm, pad=0):
    """strides of a view whose dimension perm[0] is stored fastest, then perm[1], ...; rows of storage pad bytes apart from dense"""
    nb, acc = [0] * 4, es
    for j, ax in enumerate(perm):
        nb[ax] = acc
        acc = acc * ne[ax] + (pad if j == 0 else 0)
    return nb


def cpy_case(rng, st, dt, s_ne, d_ne=None, s_perm=None, d_perm=None, s_pad=0, d_pad=0, label="cpy_kernel", same=False):
    s_ne = list(s_ne) + [1] * (4 - len(s_ne))
    d_ne = list(d_ne or s_ne) + [1] * (4 - len(d_ne or s_ne))
    es_s, es_d = (4 if st == F32 else 2), (4 if dt == F32 else 2)
    s_nb = permuted_nb(s_ne, es_s, s_perm, s_pad) if s_perm else nbytes_of(s_ne, es_s, s_pad)
    d_nb = permuted_nb(d_ne, es_d, d_perm, d_pad) if d_perm else nbytes_of(d_ne, es_d, d_pad)
    a = Buf(st, s_ne, s_nb, seed=1).put(rng.normal(0, 3, s_ne[::-1]))
    d = Buf(dt, d_ne, d_nb, share=a) if same else Buf(dt, d_ne, d_nb, off=16 if d_pad else 0, seed=3)
    want_bytes = R.cpy(a.root.host, st, s_ne, s_nb, a.off, d.root.host, dt, d_ne, d_nb, d.off)
    c = Case(OP_CPY, label, d, a, want=d.read(want_bytes), exact=True, shape=f"{st}->{dt} {s_ne}->{d_ne} perm{s_perm}/{d_perm} pad{s_pad}/{d_pad}")
    c.want_bytes = want_bytes
    return c


reg("cpy-f32-contiguous-memcpy", cpy_case, F32, F32, [300, 7], label="memcpy")
reg("cpy-f16-contiguous-memcpy-reshape", cpy_case, F16, F16, [300, 7], d_ne=[100, 21], label="memcpy")
reg("cpy-same-buffer-memcpy", cpy_case, F32, F32, [300, 7], same=True, label="memcpy")
for _st, _dt in ((F32, F32), (F32, F16), (F16, F16), (F16, F32)):
    reg(f"cpy-{_st}to{_dt}-permuted-src", cpy_case, _st, _dt, [17, 5, 3, 2], s_perm=[0, 2, 1, 3], s_pad=8)
    reg(f"cpy-{_st}to{_dt}-permuted-dst", cpy_case, _st, _dt, [17, 5, 3, 2], d_perm=[1, 0, 3, 2], d_pad=8)
    reg(f"cpy-{_st}to{_dt}-reshape", cpy_case, _st, _dt, [30, 7, 2], d_ne=[21, 20], s_perm=[1, 0, 2, 3], d_pad=4)
for _dt in (F16, F32):
    for _ne0, _ne1, _label in ((33, 9, "cpy_transpose_kernel"), (70, 45, "cpy_transpose_kernel"), (32, 8, "cpy_transpose_kernel"), (31, 9, "cpy_kernel"),
                               (33, 7, "cpy_kernel")):
        reg(f"cpy-transpose-{_ne0}x{_ne1}-f32to{_dt}", cpy_case, F32, _dt, [_ne0, _ne1], s_perm=[1, 0, 2, 3], d_pad=12 if _dt == F32 else 6, label=_label)
reg("cpy-transpose-70x45-f16tof16", cpy_case, F16, F16, [70, 45], s_perm=[1, 0, 2, 3], s_pad=4, d_pad=6, label="cpy_transpose_kernel")
reg("cpy-transpose-70x45-f16tof32", cpy_case, F16, F32, [70, 45], s_perm=[1, 0, 2, 3], d_pad=4, label="cpy_transpose_kernel")

# ------------------------------------------------------------------------------------------------ GET_ROWS (f32 / f16; quantized: in the GPU test, against the oracle)
def get_rows_case(rng, type_, ne0, n_rows=9, ne11=1, ne12=1, pad=0, strided_ids=False, bad_ids=False):
    es = 4 if type_ == F32 else 2
    # one spare row either side of the view: an id of -1 or n_rows read through a broken guard still lands inside the allocation
    nb = nbytes_of([ne0, n_rows + 2, ne11, ne12], es, pad)
    a = Buf(type_, [ne0, n_rows, ne11, ne12], nb, off=nb[1], tail=nb[1] + 64, seed=1).put(rng.normal(0, 3, (ne12, ne11, n_rows, ne0)))
    ne10 = 3
    idv = rng.integers(0, n_rows, (ne12, ne11, ne10)).astype(np.int32)
    untouched = None
    if bad_ids:
        idv[0, 0, 0], idv[-1, -1, -1] = -1, n_rows
        untouched = np.zeros((ne12, ne11, ne10, ne0), bool)
        untouched[0, 0, 0] = untouched[-1, -1, -1] = True
    i_ne = [ne10, ne11, ne12]
    ids = Buf(I32, i_ne, [8, 8 * ne10 + 4, (8 * ne10 + 4) * ne11 + 12, 0] if strided_ids else None, seed=2).put(idv)
    if strided_ids:
        ids.nb[3] = ids.nb[2] * ne12
    d = Buf(F32, [ne0, ne10, ne11, ne12], nbytes_of([ne0, ne10, ne11, ne12], 4, 16 if pad else 0), seed=3)
    want = R.get_rows(a.values().astype(f32), np.clip(idv, 0, n_rows - 1))
    return Case(OP_GET_ROWS, "get_rows_kernel", d, a, ids, want=want, exact=True, untouched=untouched,
                shape=f"type{type_} ne0={ne0} rows={n_rows} ids=[{ne10},{ne11},{ne12}] pad{pad} strided_ids{int(strided_ids)} bad{int(bad_ids)}")


for _t in (F32, F16):
    for _ne0 in (1, 300, 1024):
        reg(f"get_rows-type{_t}-{_ne0}", get_rows_case, _t, _ne0)
    reg(f"get_rows-type{_t}-batched-strided", get_rows_case, _t, 300, ne11=3, ne12=2, pad=8, strided_ids=True)
    reg(f"get_rows-type{_t}-bad-ids", get_rows_case, _t, 300, ne11=3, ne12=2, pad=8, bad_ids=True)

# ------------------------------------------------------------------------------------------------ MUL_MAT_F
def mul_mat_case(rng, type_, M, N, K, label, a_ne23=(1, 1), b_ne23=(1, 1), a_pad=0, b_pad=0, d_pad=0, off=0, kcache=False):
    es = 4 if type_ == F32 else 2
    a_ne, b_ne, d_ne = [K, M, *a_ne23], [K, N, *b_ne23], [M, N, *b_ne23]
    a_nb = nbytes_of(a_ne, es, a_pad)
    if kcache:                                               # [d, n_kv, h_kv] view of a cache stored [n_kv][h_kv][d]
        hk = a_ne23[0]
        a_nb = [2, hk * K * 2, K * 2, M * hk * K * 2]
    a = Buf(type_, a_ne, a_nb, off=off, seed=1).put(rng.normal(0, 1, a_ne[::-1]))
    b = Buf(F32, b_ne, nbytes_of(b_ne, 4, b_pad), off=off, seed=2).put(rng.normal(0, 1, b_ne[::-1]))
    d = Buf(F32, d_ne, nbytes_of(d_ne, 4, d_pad), seed=3)
    f16 = type_ == F16
    return Case(OP_MUL_MAT_F, label, d, a, b, want=R.mul_mat(a.values(), b.values(), f16), rest=R.mul_mat_f32(a.values(), b.values(), f16),
                shape=f"type{type_} M={M} N={N} K={K} a{list(a_ne23)} b{list(b_ne23)} pad{a_pad}/{b_pad}/{d_pad} off{off} kcache{int(kcache)}")


FV, FS = "mul_mat_f16_kernel<vec>", "mul_mat_f16_kernel<scalar>"
for _M, _N in ((1, 1), (63, 65), (65, 63), (130, 70)):
    for _K in (8, 24, 32, 40, 96):
        reg(f"mul_mat_f16-{_M}x{_N}x{_K}-vec", mul_mat_case, F16, _M, _N, _K, FV)
    # K = 4: rows of 8 bytes are 16-byte aligned only when padded (one row: any stride is)
    reg(f"mul_mat_f16-{_M}x{_N}x4-vec", mul_mat_case, F16, _M, _N, 4, FV, a_pad=8)
    for _K in (37, 100):                                     # rows padded to a 16-byte stride: the V-cache view of the KQV product
        reg(f"mul_mat_f16-{_M}x{_N}x{_K}-padded-vec", mul_mat_case, F16, _M, _N, _K, FV, a_pad=(-_K * 2) % 16 + 16, b_pad=(-_K * 4) % 16)
reg("mul_mat_f16-63x65x37-dense-scalar", mul_mat_case, F16, 63, 65, 37, FS)
reg("mul_mat_f16-130x70x37-dense-scalar", mul_mat_case, F16, 130, 70, 37, FS)
reg("mul_mat_f16-1x1x3-scalar", mul_mat_case, F16, 1, 1, 3, FS, a_ne23=(2, 1), b_ne23=(2, 1))
reg("mul_mat_f16-gqa-r2-4-r3-2", mul_mat_case, F16, 65, 9, 40, FV, a_ne23=(2, 1), b_ne23=(8, 2))
reg("mul_mat_f16-kcache-view", mul_mat_case, F16, 70, 5, 64, FV, a_ne23=(2, 1), b_ne23=(8, 1), kcache=True)
reg("mul_mat_f16-dst-rows-strided", mul_mat_case, F16, 65, 63, 32, FV, d_pad=20, b_ne23=(2, 1))
DB, DK = "mul_mat_dot_block_kernel", "mul_mat_dot_kernel"
reg("mul_mat_f32-8x1x1024-block", mul_mat_case, F32, 8, 1, 1024, DB)
reg("mul_mat_f32-8x2x1030-block", mul_mat_case, F32, 8, 2, 1030, DB)            # rows of 4120 bytes: every other one off 16-byte alignment
reg("mul_mat_f32-64x32x1024-block", mul_mat_case, F32, 64, 32, 1024, DB)
reg("mul_mat_f32-8x2x1027-block-ptr-off-4", mul_mat_case, F32, 8, 2, 1027, DB, off=4, b_ne23=(2, 1))
reg("mul_mat_f32-64x33x1024-dot", mul_mat_case, F32, 64, 33, 1024, DK)
reg("mul_mat_f32-8x1x1023-dot", mul_mat_case, F32, 8, 1, 1023, DK)
reg("mul_mat_f32-5x3x7-dot-batch", mul_mat_case, F32, 5, 3, 7, DK, a_ne23=(2, 1), b_ne23=(4, 3), d_pad=8)

# ------------------------------------------------------------------------------------------------ ARGSORT, SUM_ROWS
def argsort_case(rng, ne0, rows, desc, pad=0):
    xv = rng.normal(0, 1, (rows, ne0)).astype(f32)
    if ne0 >= 8:
        xv[:, rng.integers(0, ne0, ne0 // 3)] = f32(0.5)                  # repeated values: ties go by index
        xv[0, 1], xv[0, ne0 - 2], xv[-1, 3], xv[-1, 4] = np.inf, -np.inf, np.inf, np.inf
    a = Buf(F32, [ne0, rows], nbytes_of([ne0, rows], 4, pad), seed=1).put(xv)
    d = Buf(I32, [ne0, rows], nbytes_of([ne0, rows], 4, 2 * pad), seed=3)
    return Case(OP_ARGSORT, "argsort_kernel", d, a, params=(int(desc),), want=R.argsort(a.values(), desc), exact=True, shape=f"{rows}x{ne0} desc{int(desc)} pad{pad}")


for _ne0 in (1, 8, 255, 256, 257, 300, 4096):
    for _desc in (False, True):
        reg(f"argsort-{_ne0}-{'desc' if _desc else 'asc'}", argsort_case, _ne0, 2 if _ne0 == 4096 else 3, _desc)
reg("argsort-300-strided", argsort_case, 300, 5, True, pad=12)


def sum_rows_case(rng, ne, pad=0):
    ne = list(ne) + [1] * (4 - len(ne))
    a = Buf(F32, ne, nbytes_of(ne, 4, pad, 2 * pad), seed=1).put(rng.normal(0.3, 1, ne[::-1]))
    d_ne = [1] + ne[1:]
    d = Buf(F32, d_ne, [4, 4 + pad, (4 + pad) * ne[1], (4 + pad) * ne[1] * ne[2]], seed=3)
    return Case(OP_SUM_ROWS, "sum_rows_kernel", d, a, want=R.sum_rows(a.values()), rest=R.sum_rows(a.values(), f32), shape=f"{ne} pad{pad}")


for _ne0 in (1, 63, 64, 65, 5000):
    reg(f"sum_rows-{_ne0}", sum_rows_case, [_ne0, 5])
reg("sum_rows-4d", sum_rows_case, [65, 3, 5, 2])
reg("sum_rows-4d-strided", sum_rows_case, [65, 3, 5, 2], pad=8)

IDS = [i for i, _ in CASES]
assert len(set(IDS)) == len(IDS)
BUILDERS = dict(CASES)
