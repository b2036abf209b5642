"""IQ1_S / IQ1_M checkers: the live reference (oracle/_ref/libggml-{base,cpu}.so through ctypes) and a numpy restatement of its two
dequantizers and its two scalar dot products.

Both formats index one grid of 2048 entries of eight values -1 / 0 / +1.  Neither the repository nor this file holds it.
``Iq1Ref.codebook`` reads it out of the reference at run time the way the plugin does: IQ1_S's dequantizer on crafted blocks whose every
output float is 8 * (g + 0.125) = 8 g + 1.  The numpy functions take the table as an argument: uint32 [4096], entry e = words 2e
(weights 0 .. 3) and 2e + 1 (weights 4 .. 7), every byte an int8, the form qmm_set_codebook takes.  Layouts: ggml/src/ggml-common.h:382-402.
IQ1_S: f16 d | qs[32] | qh[8] u16 (four 3-bit high index parts, a 3-bit scale, the delta sign).  IQ1_M: qs[32] | qh[16] (per nibble three
high index bits and a delta sign) | four u16 of 3-bit scales whose top nibbles spell the f16 super-scale."""
import ctypes as C

import numpy as np

from iq2_refs import Iq2Ref
from iq3_refs import Q8K_BYTES, _ptr, split_q8_K  # noqa: F401

IQ1_S, IQ1_M, Q8_K = 19, 29, 15
NAMES = {IQ1_S: "iq1_s", IQ1_M: "iq1_m"}
BLOCK_BYTES = {IQ1_S: 50, IQ1_M: 56}
ENTRIES = 2048
f32 = np.float32


def row_size(t, k):
    assert k % 256 == 0
    return k // 256 * BLOCK_BYTES[t]


def set_d_iq1m(blk, d):
    """writes the f16 of d [n] into the top nibbles of the four scale words of IQ1_M blocks [n, 56] (nibble j of the f16 -> byte 49 + 2 j)"""
    h = np.asarray(d, f32).astype(np.float16).view(np.uint16).astype(np.uint32)
    for j in range(4):
        blk[:, 49 + 2 * j] = (blk[:, 49 + 2 * j] & 0x0f) | (((h >> (4 * j)) & 15) << 4).astype(np.uint8)


def crafted_blocks(t=IQ1_S):
    """the 64 blocks whose dequantized floats spell the grid: super-scale 8.0, sub-block scales 0 (2 * 0 + 1 = 1), every delta +; block
    b holds the entries 32 b .. 32 b + 31: the low byte in qs, h = 32 b >> 8 in every 3-bit high part.  IQ1_M's four scale words are
    then 0x0000, 0x0000, 0x8000, 0x4000: the top nibbles 0, 0, 8, 4 of f16 8.0 = 0x4800"""
    blk = np.zeros((64, BLOCK_BYTES[t]), np.uint8)
    for b in range(64):
        h = (32 * b) >> 8
        if t == IQ1_S:
            blk[b, 2:34] = (32 * b + np.arange(32)) & 0xff
            blk[b, 34:50] = np.full(8, h | h << 3 | h << 6 | h << 9, "<u2").view(np.uint8)
        else:
            blk[b, 0:32] = (32 * b + np.arange(32)) & 0xff
            blk[b, 32:48] = h | h << 4
    if t == IQ1_S:
        blk[:, 0:2] = np.array([8.0], np.float16).view(np.uint8)
    else:
        blk[:, 48:56] = np.array([0x0000, 0x0000, 0x8000, 0x4000], "<u2").view(np.uint8)
    return blk


def grid_from_floats(out):
    """f32 [2048 * 8] -> uint32 [4096], byte j of word w = the int8 (float 4 w + j - 1) / 8; None unless every float is -7, 1 or 9"""
    out = np.asarray(out, f32)
    if not np.all((out == -7) | (out == 1) | (out == 9)):
        return None
    b = ((out - 1) / 8).astype(np.int8).view(np.uint8).astype(np.uint32).reshape(-1, 4)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)


class Iq1Ref(Iq2Ref):
    """ggml_quantize_chunk (with an importance matrix of ones, which IQ1_S requires), dequantize_row_iq1_*, ggml_vec_dot_iq1_*_q8_K and
    quantize_row_q8_K of the live reference"""

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

    def codebook(self, t=IQ1_S):
        """uint32 [4096], derived through the dequantizer of t (both give the same table); never stored"""
        if t not in self._books:
            grid = grid_from_floats(self.dequantize(t, crafted_blocks(t), 256).reshape(-1))
            assert grid is not None and grid.size == 2 * ENTRIES
            grid.setflags(write=False)
            self._books[t] = grid
        return self._books[t]


# ------------------------------------------------------------------------------------------------ numpy restatement

def _fields(t, w, k):
    """per 32-weight sub-block of every row: d f32 [rows, nb, 1], grid index [rows, nb, 8, 4] (one per eight weights), delta sign
    [rows, nb, 8, 4] (+1 / -1), 3-bit scales [rows, nb, 8, 2] (weights 0 .. 15, 16 .. 31; IQ1_S: the same one twice)"""
    w = np.ascontiguousarray(w, np.uint8).reshape(-1, k // 256, BLOCK_BYTES[t])
    rows, nb = w.shape[:2]
    l = np.arange(4)
    if t == IQ1_S:
        d = w[:, :, 0:2].copy().view(np.float16).astype(f32)
        qs = w[:, :, 2:34].reshape(rows, nb, 8, 4).astype(np.uint32)
        qh = w[:, :, 34:50].copy().view("<u2").astype(np.uint32)                 # [rows, nb, 8]
        idx = qs | (((qh[..., None] >> (3 * l)) & 7) << 8)
        sign = np.broadcast_to(np.where(qh[..., None] & 0x8000, -1, 1), idx.shape)
        s = (qh >> 12) & 7
        scale = np.stack([s, s], -1)
    else:
        sc = w[:, :, 48:56].copy().view("<u2").astype(np.uint32)                 # [rows, nb, 4]
        h = (sc[..., 0] >> 12) | ((sc[..., 1] >> 8) & 0x00f0) | ((sc[..., 2] >> 4) & 0x0f00) | (sc[..., 3] & 0xf000)
        d = h.astype(np.uint16).view(np.float16).astype(f32)[..., None]
        qs = w[:, :, 0:32].reshape(rows, nb, 8, 4).astype(np.uint32)
        qh = w[:, :, 32:48].reshape(rows, nb, 8, 2).astype(np.uint32)
        nib = np.stack([qh[..., 0] & 15, qh[..., 0] >> 4, qh[..., 1] & 15, qh[..., 1] >> 4], -1)    # [rows, nb, 8, 4]
        idx = qs | ((nib & 7) << 8)
        sign = np.where(nib & 8, -1, 1)
        ib = np.arange(8)
        s6 = (sc[:, :, ib // 2] >> (6 * (ib % 2))) & 63                           # [rows, nb, 8]
        scale = np.stack([s6 & 7, s6 >> 3], -1)
    return d, idx, sign.astype(np.int64), scale.astype(np.int64)


def _grid_values(idx, grid):
    """int64 [..., 4, 8]: the eight int8 values of each entry"""
    g = np.asarray(grid, np.uint32).reshape(-1, 2)[idx]                          # [..., 4, 2]
    b = np.stack([(g >> (8 * j)) & 0xff for j in range(4)], -1).reshape(*idx.shape, 8)
    return b.astype(np.uint8).view(np.int8).astype(np.int64)


def dequantize_np(t, w, k, grid):
    """dequantize_row_iq1_s / _iq1_m (ggml-quants.c:2359-2432) in f32 steps, dl = d * (2 s + 1), then dl * (g + delta): f32 [rows, k]"""
    d, idx, sign, scale = _fields(t, w, k)
    g = _grid_values(idx, grid).astype(f32)                                      # [rows, nb, 8, 4, 8]
    dl = (d[..., None] * (2 * scale + 1).astype(f32)).astype(f32)                # [rows, nb, 8, 2]
    dl = np.repeat(dl, 2, -1)[..., None]                                         # per entry l: the half l / 2
    delta = (sign.astype(f32) * f32(0.125))[..., None]
    return (dl * (g + delta).astype(f32)).astype(f32).reshape(d.shape[0], k)


def mul_mat_np(t, w, k, acts, grid):
    """the scalar branches of ggml_vec_dot_iq1_s_q8_K / _iq1_m_q8_K (ggml-cpu-quants.c:12099-12130, 12401-12446) on Q8_K rows: exact
    integer sums, sumf += (d * y.d) * (sumi + 0.125 * sumi1) block by block in f32: f32 [n, rows]"""
    d, idx, sign, scale = _fields(t, w, k)
    g = _grid_values(idx, grid)                                                  # [rows, nb, 8, 4, 8]
    yd, yq = split_q8_K(acts, k)
    n, rows, nb = yq.shape[0], g.shape[0], g.shape[1]
    ls = np.repeat(2 * scale + 1, 2, -1)                                         # [rows, nb, 8, 4]
    out = np.zeros((n, rows), f32)
    for b in range(nb):
        y = yq[:, b].reshape(n, 8, 4, 8)
        lsum = np.einsum("rslj,nslj->nrsl", g[:, b], y)                          # exact
        ysum = y.sum(-1)                                                         # [n, 8, 4]
        sumi = (lsum * ls[None, :, b]).sum((-1, -2))
        sumi1 = (ysum[:, None] * (sign[:, b] * ls[:, b])[None]).sum((-1, -2))
        dd = (d[None, :, b, 0] * yd[:, b, None]).astype(f32)
        out = (out + (dd * (sumi.astype(f32) + f32(0.125) * sumi1.astype(f32)).astype(f32)).astype(f32)).astype(f32)
    return out


def covering_rows(t, k=512, seed=0):
    """random-byte rows in which all 2048 grid indices, both delta signs (IQ1_M: all 16 patterns of the four of a sub-block) and all 8
    values of every scale field occur; d finite with both signs, |d| in [2^-10, 2^-4] but for one block each of +-2^-24 (f16's smallest)"""
    rng = np.random.default_rng(seed)
    bpr = k // 256
    nb = -(-80 // bpr) * bpr
    blk = rng.integers(0, 256, (nb, BLOCK_BYTES[t]), dtype=np.uint8)
    d = np.exp2(rng.uniform(-10, -4, nb)).astype(f32) * rng.choice(np.array([-1, 1], f32), nb)
    d[74], d[75], d[76] = 2.0 ** -24, -2.0 ** -24, -2.0 ** -7
    v = np.arange(8)
    if t == IQ1_S:
        blk[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(nb, 2)
        qh = blk[:, 34:50].copy().view("<u2")                                    # [nb, 8]
        for b in range(64):                                                      # indices 0 .. 2047
            h = (32 * b) >> 8
            blk[b, 2:34] = (32 * b + np.arange(32)) & 0xff
            qh[b] = (qh[b] & 0xf000) | h | h << 3 | h << 6 | h << 9
        qh[64] = (qh[64] & 0x0fff) | (v << 12)                                   # scales 0 .. 7, delta +
        qh[65] = (qh[65] & 0x0fff) | (v << 12) | 0x8000                          # scales 0 .. 7, delta -
        blk[:, 34:50] = qh.view(np.uint8)
    else:
        for b in range(64):
            h = (32 * b) >> 8
            blk[b, 0:32] = (32 * b + np.arange(32)) & 0xff
            blk[b, 32:48] = (blk[b, 32:48] & 0x88) | h | h << 4
        c = np.arange(16)                                                        # the delta signs of sub-block c of blocks 64, 65 = the bits of c
        qh = blk[64:66, 32:48].reshape(16, 2)
        qh[:, 0] = (qh[:, 0] & 0x77) | ((c & 1) << 3) | (((c >> 1) & 1) << 7)
        qh[:, 1] = (qh[:, 1] & 0x77) | (((c >> 2) & 1) << 3) | (((c >> 3) & 1) << 7)
        blk[64:66, 32:48] = qh.reshape(2, 16)
        sc = blk[:, 48:56].copy().view("<u2")                                    # [nb, 4]
        for j in range(8):                                                       # block 66 + j: field f of every word holds (j + f) % 8
            sc[66 + j] = (sc[66 + j] & 0xf000) | ((j % 8) | ((j + 1) % 8) << 3 | ((j + 2) % 8) << 6 | ((j + 3) % 8) << 9)
        blk[:, 48:56] = sc.view(np.uint8)
        set_d_iq1m(blk, d)
    return blk.reshape(-1, bpr * BLOCK_BYTES[t])
