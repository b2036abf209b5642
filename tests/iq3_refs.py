"""IQ3_XXS / IQ3_S checkers: the live reference (oracle/_ref/libggml-{base,cpu}.so through ctypes) and a numpy restatement of its two
dequantizers and its two scalar dot products.

Neither the repository nor this file holds the formats' grids.  ``Iq3Ref.codebook`` reads them out of the reference at run time the way
the plugin does: the type's dequantizer on crafted blocks whose every output float is one byte of one grid entry.  The numpy functions
take such a table as an argument.  Layouts: ggml/src/ggml-common.h:365-380; the sign of a weight in IQ3_XXS comes from a 7-bit index
whose eighth bit is its parity (``sign_byte``)."""
import ctypes as C

import numpy as np
import pytest

IQ3_XXS, IQ3_S, Q8_K = 18, 21, 15
NAMES = {IQ3_XXS: "iq3_xxs", IQ3_S: "iq3_s"}
BLOCK_BYTES = {IQ3_XXS: 98, IQ3_S: 110}
ENTRIES = {IQ3_XXS: 256, IQ3_S: 512}
Q8K_BYTES = 292                                   # block_q8_K: f32 d, 256 int8, 16 int16 sums
f32 = np.float32


def row_size(t, k):
    assert k % 256 == 0
    return k // 256 * BLOCK_BYTES[t]


def sign_byte(s7):
    """the eight sign bits behind a 7-bit sign index: the index, with its parity as bit 7"""
    s7 = np.asarray(s7, np.uint32)
    par = np.zeros_like(s7)
    for b in range(7):
        par ^= (s7 >> b) & 1
    return (s7 | (par << 7)).astype(np.uint8)


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p)


def crafted_blocks(t):
    """the blocks whose dequantized floats spell the grid: IQ3_XXS d = 4.0 with all sign / scale words 0 (scale 4 * 0.5 * 0.5 = 1, signs +),
    IQ3_S d = 1.0 with scales 0 and signs 0; block b holds indices 64 b .. 64 b + 63 (IQ3_S: the ninth bit, qh, set from block 4 on)"""
    n = ENTRIES[t] // 64
    blk = np.zeros((n, BLOCK_BYTES[t]), np.uint8)
    blk[:, 0:2] = np.array([4.0 if t == IQ3_XXS else 1.0], np.float16).view(np.uint8)
    for b in range(n):
        blk[b, 2:66] = (64 * b + np.arange(64)) & 0xff
        if t == IQ3_S and b >= 4:
            blk[b, 66:74] = 0xff
    return blk


def grid_from_floats(out):
    """f32 [entries * 4] -> uint32 [entries], byte j of an entry = float 4 e + j; None unless every float is an integer in 1 .. 255"""
    if not np.all((out >= 1) & (out <= 255) & (out == np.floor(out))):
        return None
    b = out.astype(np.uint32).reshape(-1, 4)
    return b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16) | (b[:, 3] << 24)


class Iq3Ref:
    """ggml_quantize_chunk, dequantize_row_iq3_*, ggml_vec_dot_iq3_*_q8_K and quantize_row_q8_K of the live reference"""

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
        """f32 [rows, k] -> uint8 [rows, row size] with the reference's own quantizer (no importance matrix); any ggml type"""
        x = np.ascontiguousarray(x, f32)
        rows, k = x.shape
        out = np.zeros((rows, self.ref.row_size(t, k)), np.uint8)
        n = self.base.ggml_quantize_chunk(t, _ptr(x), _ptr(out), 0, rows, k, None)
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
        """dst f32 [N, M]: the reference's quantizer and vec_dot, row by row"""
        w = np.ascontiguousarray(w, np.uint8).reshape(-1, row_size(t, k))
        acts = self.quantize_act(x)
        return np.array([[self.vec_dot(t, k, w[j], acts[i]) for j in range(w.shape[0])] for i in range(acts.shape[0])], f32)

    def codebook(self, t):
        """uint32 [256 | 512], derived from the reference's dequantizer; never stored"""
        if t not in self._books:
            grid = grid_from_floats(self.dequantize(t, crafted_blocks(t), 256).reshape(-1))
            assert grid is not None and grid.size == ENTRIES[t]
            self._books[t] = grid
        return self._books[t]


# ------------------------------------------------------------------------------------------------ numpy restatement

def _fields(t, w, k):
    """per 32-weight sub-block of every row: d f32 [rows, nb, 1], grid index [rows, nb, 8, 8], sign bits [rows, nb, 8, 4] (one byte per
    eight weights), odd scale multiplier 2 s + 1 [rows, nb, 8]"""
    w = np.ascontiguousarray(w, np.uint8).reshape(-1, k // 256, BLOCK_BYTES[t])
    rows, nb = w.shape[:2]
    d = w[:, :, 0:2].copy().view(np.float16).astype(f32)                      # [rows, nb, 1]
    idx = w[:, :, 2:66].reshape(rows, nb, 8, 8).astype(np.uint32)
    if t == IQ3_XXS:
        aux = w[:, :, 66:98].copy().view("<u4").reshape(rows, nb, 8)
        signs = np.stack([sign_byte((aux >> (7 * l)) & 127) for l in range(4)], -1)
        ls = (2 * (aux >> 28) + 1).astype(np.int64)
    else:
        qh = w[:, :, 66:74].astype(np.uint32)                                  # [rows, nb, 8]
        idx = idx | (((qh[..., None] >> np.arange(8)) & 1) << 8)
        signs = w[:, :, 74:106].reshape(rows, nb, 8, 4)
        sc = w[:, :, 106:110].astype(np.int64)                                 # [rows, nb, 4]
        nib = np.stack([sc & 15, sc >> 4], -1).reshape(rows, nb, 8)
        ls = 2 * nib + 1
    return d, idx, signs, ls


def _signed_magnitudes(t, w, k, grid):
    """int64 [rows, nb, 8, 32]: grid byte with its sign, in k order"""
    d, idx, signs, ls = _fields(t, w, k)
    g = np.asarray(grid, np.uint32)[idx]                                       # [rows, nb, 8, 8]
    mag = np.stack([(g >> (8 * j)) & 0xff for j in range(4)], -1).reshape(*g.shape[:3], 32).astype(np.int64)
    bits = ((signs[..., None].astype(np.uint32) >> np.arange(8)) & 1).reshape(*g.shape[:3], 32)
    return d, np.where(bits == 1, -mag, mag), ls


def dequantize_np(t, w, k, grid):
    """dequantize_row_iq3_xxs / _iq3_s (ggml-quants.c:2284-2355) in f32 steps: f32 [rows, k]"""
    d, sm, ls = _signed_magnitudes(t, w, k, grid)
    if t == IQ3_XXS:
        db = (d * (f32(0.5) + ((ls - 1) // 2).astype(f32))).astype(f32) * f32(0.5)      # d * (0.5 + s) * 0.5
    else:
        db = (d * ls.astype(f32)).astype(f32)                                           # d * (1 + 2 s)
    mag = np.abs(sm).astype(f32)
    v = (db[..., None] * mag).astype(f32)
    return np.where(sm < 0, -v, v).astype(f32).reshape(sm.shape[0], k)


def split_q8_K(acts, k):
    """uint8 [n, k / 256 * 292] -> d f32 [n, nb], q int64 [n, nb, 256]"""
    a = np.ascontiguousarray(acts, np.uint8).reshape(acts.shape[0], k // 256, Q8K_BYTES)
    return a[:, :, 0:4].copy().view(f32)[..., 0], a[:, :, 4:260].copy().view(np.int8).astype(np.int64)


def mul_mat_np(t, w, k, acts, grid):
    """the scalar branches of ggml_vec_dot_iq3_xxs_q8_K / _iq3_s_q8_K (ggml-cpu-quants.c:11218-11249, 11733-11776) on Q8_K rows:
    exact integer block sums, sumf += (d * y.d) * bsum block by block in f32, IQ3_XXS * 0.25: f32 [n, rows]"""
    d, sm, ls = _signed_magnitudes(t, w, k, grid)
    yd, yq = split_q8_K(acts, k)
    n, rows, nb = yq.shape[0], sm.shape[0], sm.shape[1]
    out = np.zeros((n, rows), f32)
    for b in range(nb):
        sumi = np.einsum("rsk,nsk->nrs", sm[:, b], yq[:, b].reshape(n, 8, 32))            # [n, rows, 8], exact
        bsum = (sumi * ls[None, :, b, :]).sum(-1)
        dd = (d[None, :, b, 0] * yd[:, b, None]).astype(f32)
        out = (out + (dd * bsum.astype(f32)).astype(f32)).astype(f32)
    return (f32(0.25) * out).astype(f32) if t == IQ3_XXS else out


def covering_rows(t, k=512, seed=0):
    """random-byte rows in which every grid index, every sign pattern and every scale value occurs; d finite, |d| in [2^-10, 2^-4]"""
    rng = np.random.default_rng(seed)
    nb = 16 * (k // 256) * 4
    blk = rng.integers(0, 256, (nb, BLOCK_BYTES[t]), dtype=np.uint8)
    d = np.exp2(rng.uniform(-10, -4, nb)).astype(f32) * rng.choice(np.array([-1, 1], f32), nb)
    blk[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(nb, 2)
    if t == IQ3_XXS:
        blk[:4, 2:66] = (np.arange(256) & 0xff).reshape(4, 64)                 # indices 0 .. 255
        aux = blk[:, 66:98].copy().view("<u4")                                 # [nb, 8] sign / scale words
        a = aux[4:8].reshape(-1)                                                # 32 words x 4 positions: the 128 sign indices
        for l in range(4):
            a = (a & ~np.uint32(127 << (7 * l))) | ((4 * np.arange(32, dtype=np.uint32) + l) << (7 * l))
        aux[4:8] = a.reshape(4, 8)
        s = aux[8:10].reshape(-1)                                               # 16 words: the 16 scales
        aux[8:10] = ((s & np.uint32(0x0fffffff)) | (np.arange(16, dtype=np.uint32) << 28)).reshape(2, 8)
        blk[:, 66:98] = aux.view(np.uint8).reshape(nb, 32)
    else:
        for b in range(8):                                                      # indices 0 .. 511
            blk[b, 2:66] = (64 * b + np.arange(64)) & 0xff
            blk[b, 66:74] = 0xff if b >= 4 else 0
        blk[8:16, 74:106] = np.arange(256, dtype=np.uint8).reshape(8, 32)      # every sign byte
        blk[16, 106:110] = [0x10, 0x32, 0x54, 0x76]                            # scales 0 .. 15
        blk[17, 106:110] = [0x98, 0xba, 0xdc, 0xfe]
    return blk.reshape(-1, k // 256 * BLOCK_BYTES[t])
