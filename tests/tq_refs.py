"""TQ1_0 / TQ2_0 checkers: the live reference (oracle/_ref/libggml-{base,cpu}.so through ctypes) and a numpy restatement of its two
dequantizers and its two scalar dot products.

Neither format needs a table.  Layouts (ggml/src/ggml-common.h:233-246), d is the LAST field of both blocks:
  TQ2_0  66 B  qs[64] | f16 d      weight w: j = w / 128, l = (w % 128) / 32, m = w % 32: code = (qs[32 j + m] >> 2 l) & 3, value (code - 1) * d
  TQ1_0  54 B  qs[48] | qh[4] | f16 d     five trits per byte, trit n of byte b = ((uint8) (b * 3^n) * 3) >> 8, value (trit - 1) * d
         w in [0, 160): qs[w % 32], n = w / 32;  w in [160, 240): qs[32 + (w - 160) % 16], n = (w - 160) / 16;
         w in [240, 256): qh[(w - 240) % 4], n = (w - 240) / 4
Every byte value is valid content: TQ2_0's code 3 is +2, and a TQ1_0 byte above 242 goes through the same formula."""
import ctypes as C

import numpy as np

from iq2_refs import Iq2Ref
from iq3_refs import Q8K_BYTES, _ptr, split_q8_K  # noqa: F401

TQ1_0, TQ2_0, Q8_K = 34, 35, 15
NAMES = {TQ1_0: "tq1_0", TQ2_0: "tq2_0"}
BLOCK_BYTES = {TQ1_0: 54, TQ2_0: 66}
D_AT = {TQ1_0: 52, TQ2_0: 64}
F16_MAX, F16_TINY = 65504.0, 2.0 ** -24
f32 = np.float32


def row_size(t, k):
    assert k % 256 == 0
    return k // 256 * BLOCK_BYTES[t]


class TqRef(Iq2Ref):
    """ggml_quantize_chunk, dequantize_row_tq*_0, ggml_vec_dot_tq*_0_q8_K and quantize_row_q8_K of the live reference"""

    def dequantize(self, t, w, k):
        w = np.ascontiguousarray(w, np.uint8).reshape(-1, row_size(t, k))
        out = np.empty((w.shape[0], k), f32)
        fn = getattr(self.base, f"dequantize_row_{NAMES[t]}")
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        for r in range(w.shape[0]):
            fn(_ptr(w[r]), _ptr(out[r]), k)
        return out

    def vec_dot(self, t, k, w_row, a_row):
        fn = getattr(self.cpu, f"ggml_vec_dot_{NAMES[t]}_q8_K")
        fn.argtypes = [C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_int]
        out = C.c_float(0)
        fn(k, C.byref(out), 0, _ptr(np.ascontiguousarray(w_row)), 0, _ptr(np.ascontiguousarray(a_row)), 0, 1)
        return out.value

    def mul_mat(self, t, w, k, x):
        """dst f32 [N, M]: the reference's quantize_row_q8_K and vec_dot, row by row"""
        w = np.ascontiguousarray(w, np.uint8).reshape(-1, row_size(t, k))
        acts = self.quantize_act(x)
        return np.array([[self.vec_dot(t, k, w[j], acts[i]) for j in range(w.shape[0])] for i in range(acts.shape[0])], f32)


# ------------------------------------------------------------------------------------------------ numpy restatement

def _trit(b, n):
    """trit n (0 .. 4) of the bytes b: the multiply wraps at 8 bits"""
    q = (b.astype(np.uint32) * np.uint32(3 ** n)) & 0xff
    return ((q * 3) >> 8).astype(np.int64)


def fields(t, w, k):
    """d f32 [rows, nb, 1] and the stored values before the - 1 (trits 0 .. 2, codes 0 .. 3), int64 [rows, nb, 256] in k order"""
    w = np.ascontiguousarray(w, np.uint8).reshape(-1, k // 256, BLOCK_BYTES[t])
    rows, nb = w.shape[:2]
    d = w[:, :, D_AT[t]:D_AT[t] + 2].copy().view(np.float16).astype(f32)
    if t == TQ2_0:
        qs = w[:, :, 0:64].reshape(rows, nb, 2, 1, 32).astype(np.int64)
        v = (qs >> (2 * np.arange(4)).reshape(1, 1, 1, 4, 1)) & 3                                   # [rows, nb, j, l, m]
        return d, v.reshape(rows, nb, 256)
    a = np.stack([_trit(w[:, :, 0:32], n) for n in range(5)], 2).reshape(rows, nb, 160)
    b = np.stack([_trit(w[:, :, 32:48], n) for n in range(5)], 2).reshape(rows, nb, 80)
    c = np.stack([_trit(w[:, :, 48:52], n) for n in range(4)], 2).reshape(rows, nb, 16)
    return d, np.concatenate([a, b, c], -1)


def dequantize_np(t, w, k):
    """dequantize_row_tq1_0 / _tq2_0 (ggml-quants.c:2137-2193): (float) (v - 1) * d, one f32 product: f32 [rows, k]"""
    d, v = fields(t, w, k)
    return ((v - 1).astype(f32) * d).astype(f32).reshape(d.shape[0], k)


def mul_mat_np(t, w, k, acts):
    """the scalar branches of ggml_vec_dot_tq1_0_q8_K / _tq2_0_q8_K (ggml-cpu-quants.c:4299-4336 and the function behind it) on Q8_K
    rows: one exact integer sum per block, sumf += (float) sum * (d * y.d) block by block in f32: f32 [n, rows]"""
    d, v = fields(t, w, k)
    yd, yq = split_q8_K(acts, k)
    n, rows, nb = yq.shape[0], v.shape[0], v.shape[1]
    out = np.zeros((n, rows), f32)
    for b in range(nb):
        sumi = yq[:, b] @ (v[:, b] - 1).T                                                            # [n, rows], exact
        dd = (d[None, :, b, 0] * yd[:, b, None]).astype(f32)
        out = (out + (sumi.astype(f32) * dd).astype(f32)).astype(f32)
    return out


# ------------------------------------------------------------------------------------------------ crafted blocks

N_EDGE = 96                                        # divisible by the blocks per row of K = 256, 512, 768, 1024, 4096


def edge_rows(t, k, big=True, seed=0):
    """N_EDGE blocks as rows of K: every byte value 0 .. 255 in each position class (TQ1_0: qs[0 .. 31] in blocks 0 .. 7, qs[32 .. 47] in
    blocks 0 .. 15, qh in blocks 0 .. 63; TQ2_0: qs in blocks 0 .. 3, so every code, 3 included, at every shift), the other bytes
    random; d random with both signs but for d = 0, -0, the smallest subnormal of either sign, and (big) +-65504 on blocks whose bytes
    hold code 3 / every trit.  big=False keeps |d| <= 2^-4: rows a product can be compared on"""
    assert N_EDGE % (k // 256) == 0
    rng = np.random.default_rng(seed + t)
    blk = rng.integers(0, 256, (N_EDGE, BLOCK_BYTES[t]), dtype=np.uint8)
    b = np.arange(N_EDGE)[:, None]
    if t == TQ1_0:
        blk[:, 0:32] = (32 * b + np.arange(32)) & 0xff
        blk[:, 32:48] = (16 * b + np.arange(16)) & 0xff
        blk[:, 48:52] = (4 * b + np.arange(4)) & 0xff
    else:
        blk[:, 0:64] = (64 * b + np.arange(64) + 7 * (b // 4)) & 0xff
    d = np.exp2(rng.uniform(-10, -4, N_EDGE)).astype(f32) * rng.choice(np.array([-1, 1], f32), N_EDGE)
    d[8], d[9], d[10], d[11], d[12] = 0.0, -0.0, F16_TINY, -F16_TINY, -2.0 ** -7
    if big:
        d[3], d[7], d[63] = F16_MAX, -F16_MAX, F16_MAX
    blk[:, D_AT[t]:] = d.astype(np.float16).view(np.uint8).reshape(N_EDGE, 2)
    return blk.reshape(-1, k // 256 * BLOCK_BYTES[t])


def assert_edges(t, rows, k, big=True):
    """what edge_rows promises, read back from the bytes"""
    blk = np.ascontiguousarray(rows, np.uint8).reshape(-1, BLOCK_BYTES[t])
    classes = ((0, 32), (32, 48), (48, 52)) if t == TQ1_0 else ((0, 64),)
    for lo, hi in classes:
        assert len(np.unique(blk[:, lo:hi])) == 256
    d, v = fields(t, rows, k)
    assert set(np.unique(v).tolist()) == ({0, 1, 2} if t == TQ1_0 else {0, 1, 2, 3})
    ad = np.abs(d)
    assert (d == 0).any() and ad[ad > 0].min() == F16_TINY and d.min() < 0 < d.max() and np.isfinite(d).all()
    assert (ad.max() == F16_MAX) == big
