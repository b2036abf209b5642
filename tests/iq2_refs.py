"""IQ2_XS / IQ2_S checkers: the live reference (oracle/_ref/libggml-{base,cpu}.so through ctypes) and a numpy restatement of its two
dequantizers and its two scalar dot products.

Neither the repository nor this file holds the formats' grids.  ``Iq2Ref.codebook`` reads them out of the reference at run time the way
the plugin does: the type's dequantizer on crafted blocks whose every output float is one byte of one grid entry.  The numpy functions
take such a table as an argument: uint32 [2 * entries], entry e = words 2e (weights 0 .. 3) and 2e + 1 (weights 4 .. 7), the form
qmm_set_codebook takes.  Layouts: ggml/src/ggml-common.h:343-357.  Both formats carry two 4-bit scales per 32 weights, one per 16; the
signs of an IQ2_XS entry come from a 7-bit index whose eighth bit is its parity (``iq3_refs.sign_byte``), IQ2_S stores the byte."""
import ctypes as C

import numpy as np
import pytest

from iq3_refs import Q8K_BYTES, _ptr, sign_byte, split_q8_K  # noqa: F401

IQ2_XS, IQ2_S, Q8_K = 17, 22, 15
NAMES = {IQ2_XS: "iq2_xs", IQ2_S: "iq2_s"}
BLOCK_BYTES = {IQ2_XS: 74, IQ2_S: 82}
ENTRIES = {IQ2_XS: 512, IQ2_S: 1024}
N_SIGNS = {IQ2_XS: 128, IQ2_S: 256}               # IQ2_XS: eight signs of even parity out of a 7-bit index
f32 = np.float32


def row_size(t, k):
    assert k % 256 == 0
    return k // 256 * BLOCK_BYTES[t]


def crafted_blocks(t):
    """the blocks whose dequantized floats spell the grid: d = 8.0, scales 0 (8 * (0.5 + 0) * 0.25 = 1) and every sign +; block b holds
    the entries 32 b .. 32 b + 31 (IQ2_XS: the u16 itself, sign index 0; IQ2_S: the low byte, and qh = 0x55 * (32 b >> 8) gives all four
    entries of a sub-block the block's two high bits)"""
    n = ENTRIES[t] // 32
    blk = np.zeros((n, BLOCK_BYTES[t]), np.uint8)
    blk[:, 0:2] = np.array([8.0], np.float16).view(np.uint8)
    for b in range(n):
        e = 32 * b + np.arange(32)
        if t == IQ2_XS:
            blk[b, 2:66] = e.astype("<u2").view(np.uint8)
        else:
            blk[b, 2:34] = e & 0xff
            blk[b, 66:74] = 0x55 * ((32 * b) >> 8)
    return blk


def grid_from_floats(out):
    """f32 [entries * 8] -> uint32 [entries * 2], byte j of word w = float 4 w + j; None unless every float is an integer in 1 .. 255"""
    if not np.all((out >= 1) & (out <= 255) & (out == np.floor(out))):
        return None
    b = out.astype(np.uint32).reshape(-1, 4)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)


class Iq2Ref:
    """ggml_quantize_chunk, dequantize_row_iq2_*, ggml_vec_dot_iq2_*_q8_K and quantize_row_q8_K of the live reference"""

    def __init__(self):
        from oracle.pyoracle import RefGgml, ref_available
        if not ref_available():
            pytest.skip("oracle/_ref not built (needs the reference tree; run `make -C oracle ref`)")
        self.ref = RefGgml("avx2")
        self.base, self.cpu = self.ref.base, self.ref.cpu
        self.base.ggml_quantize_chunk.restype = C.c_size_t
        self.base.ggml_quantize_chunk.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int64, C.c_void_p]
        self._books = {}

    def quantize(self, t, x):
        """f32 [rows, k] -> uint8 [rows, row size] with the reference's own quantizer; any ggml type.  IQ2_XS is refused without an
        importance matrix (ggml_quantize_requires_imatrix, ggml.c:6496): k ones weigh every column alike"""
        x = np.ascontiguousarray(x, f32)
        rows, k = x.shape
        out = np.zeros((rows, self.ref.row_size(t, k)), np.uint8)
        ones = np.ones(k, f32)
        n = self.base.ggml_quantize_chunk(t, _ptr(x), _ptr(out), 0, rows, k, _ptr(ones))
        assert n == out.size
        return out

    def dequantize(self, t, w, k):
        w = np.ascontiguousarray(w, np.uint8).reshape(-1, row_size(t, k))
        out = np.empty((w.shape[0], k), f32)
        fn = getattr(self.base, f"dequantize_row_{NAMES[t]}")
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        for r in range(w.shape[0]):
            fn(_ptr(w[r]), _ptr(out[r]), k)
        return out

    def quantize_act(self, x):
        """f32 [n, k] -> uint8 [n, k / 256 * 292]: ggml-cpu's quantize_row_q8_K"""
        x = np.ascontiguousarray(x, f32)
        n, k = x.shape
        out = np.zeros((n, k // 256 * Q8K_BYTES), np.uint8)
        fn = self.cpu.quantize_row_q8_K
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        for r in range(n):
            fn(_ptr(x[r]), _ptr(out[r]), k)
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

    def codebook(self, t):
        """uint32 [1024 | 2048], derived from the reference's dequantizer; never stored"""
        if t not in self._books:
            grid = grid_from_floats(self.dequantize(t, crafted_blocks(t), 256).reshape(-1))
            assert grid is not None and grid.size == 2 * ENTRIES[t]
            grid.setflags(write=False)
            self._books[t] = grid
        return self._books[t]


# ------------------------------------------------------------------------------------------------ numpy restatement

def _fields(t, w, k):
    """per 32-weight sub-block of every row: d f32 [rows, nb, 1], grid index [rows, nb, 8, 4], sign bytes [rows, nb, 8, 4] (one per
    entry of eight weights), the two scale nibbles [rows, nb, 8, 2] (weights 0 .. 15, 16 .. 31)"""
    w = np.ascontiguousarray(w, np.uint8).reshape(-1, k // 256, BLOCK_BYTES[t])
    rows, nb = w.shape[:2]
    d = w[:, :, 0:2].copy().view(np.float16).astype(f32)                      # [rows, nb, 1]
    if t == IQ2_XS:
        qs = w[:, :, 2:66].copy().view("<u2").reshape(rows, nb, 8, 4).astype(np.uint32)
        idx = qs & 511
        signs = sign_byte(qs >> 9)
        sc = w[:, :, 66:74]
    else:
        qh = w[:, :, 66:74].astype(np.uint32)                                  # [rows, nb, 8]
        idx = w[:, :, 2:34].reshape(rows, nb, 8, 4).astype(np.uint32) | (((qh[..., None] << (8 - 2 * np.arange(4))) & 0x300))
        signs = w[:, :, 34:66].reshape(rows, nb, 8, 4)
        sc = w[:, :, 74:82]
    nib = np.stack([sc & 15, sc >> 4], -1).astype(np.int64)
    return d, idx, signs, nib


def _signed_magnitudes(t, w, k, grid):
    """int64 [rows, nb, 8, 32]: grid byte with its sign, in k order"""
    d, idx, signs, nib = _fields(t, w, k)
    g = np.asarray(grid, np.uint32).reshape(-1, 2)[idx]                        # [rows, nb, 8, 4, 2]
    mag = np.stack([(g >> (8 * j)) & 0xff for j in range(4)], -1).reshape(*g.shape[:3], 32).astype(np.int64)
    bits = ((signs[..., None].astype(np.uint32) >> np.arange(8)) & 1).reshape(*g.shape[:3], 32)
    return d, np.where(bits == 1, -mag, mag), nib


def dequantize_np(t, w, k, grid):
    """dequantize_row_iq2_xs / _iq2_s (ggml-quants.c:2225-2280) in f32 steps, d * (0.5 + scale) * 0.25 * magnitude: f32 [rows, k]"""
    d, sm, nib = _signed_magnitudes(t, w, k, grid)
    db = ((d[..., None] * (f32(0.5) + nib.astype(f32))).astype(f32) * f32(0.25)).astype(f32)       # [rows, nb, 8, 2]
    mag = np.abs(sm).astype(f32).reshape(*sm.shape[:3], 2, 16)
    v = (db[..., None] * mag).astype(f32).reshape(sm.shape)
    return np.where(sm < 0, -v, v).astype(f32).reshape(sm.shape[0], k)


def mul_mat_np(t, w, k, acts, grid):
    """the scalar branches of ggml_vec_dot_iq2_xs_q8_K / _iq2_s_q8_K (ggml-cpu-quants.c:10411-10447, 10885-10923) on Q8_K rows: exact
    integer sums per 16 weights times 2 scale + 1, sumf += (d * y.d) * bsum block by block in f32, the result * 0.125: f32 [n, rows]"""
    d, sm, nib = _signed_magnitudes(t, w, k, grid)
    yd, yq = split_q8_K(acts, k)
    n, rows, nb = yq.shape[0], sm.shape[0], sm.shape[1]
    ls = (2 * nib + 1).reshape(rows, nb, 16)
    out = np.zeros((n, rows), f32)
    for b in range(nb):
        sumi = np.einsum("rsk,nsk->nrs", sm[:, b].reshape(rows, 16, 16), yq[:, b].reshape(n, 16, 16))       # [n, rows, 16], exact
        bsum = (sumi * ls[None, :, b, :]).sum(-1)
        dd = (d[None, :, b, 0] * yd[:, b, None]).astype(f32)
        out = (out + (dd * bsum.astype(f32)).astype(f32)).astype(f32)
    return (f32(0.125) * out).astype(f32)


def covering_rows(t, k=512, seed=0):
    """random-byte rows in which every grid index, every sign pattern and all 16 values of both scale nibbles occur; d finite, |d| in
    [2^-10, 2^-4]"""
    rng = np.random.default_rng(seed)
    nb = 16 * (k // 256) * 4
    assert nb >= 48
    blk = rng.integers(0, 256, (nb, BLOCK_BYTES[t]), dtype=np.uint8)
    d = np.exp2(rng.uniform(-10, -4, nb)).astype(f32) * rng.choice(np.array([-1, 1], f32), nb)
    blk[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(nb, 2)
    sc_at = 66 if t == IQ2_XS else 74
    if t == IQ2_XS:
        qs = blk[:, 2:66].copy().view("<u2")                                   # [nb, 32]
        qs[0:16] = (qs[0:16] & 0xfe00) | np.arange(512, dtype=np.uint16).reshape(16, 32)          # indices 0 .. 511
        qs[16:20] = (qs[16:20] & 0x01ff) | (np.arange(128, dtype=np.uint16).reshape(4, 32) << 9)  # the 128 sign indices
        blk[:, 2:66] = qs.view(np.uint8)
    else:
        for b in range(32):                                                     # indices 0 .. 1023
            blk[b, 2:34] = (32 * b + np.arange(32)) & 0xff
            blk[b, 66:74] = 0x55 * ((32 * b) >> 8)
        blk[32:40, 34:66] = np.arange(256, dtype=np.uint8).reshape(8, 32)      # every sign byte
    blk[40, sc_at:sc_at + 8] = [0x10, 0x32, 0x54, 0x76, 0x98, 0xba, 0xdc, 0xfe]                   # both nibbles: 0 .. 15
    blk[41, sc_at:sc_at + 8] = [0x01, 0x23, 0x45, 0x67, 0x89, 0xab, 0xcd, 0xef]
    return blk.reshape(-1, k // 256 * BLOCK_BYTES[t])
