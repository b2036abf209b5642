"""numpy references of the glue ops behind qmm_op_compute / qmm_op_add_rms_norm (csrc/qmm_ops.hip), in float64 unless stated, and
the descriptor helper the GPU tests build their operands with.  A plain module: no fixtures, no GPU, torch only inside Buf.dev().

Arrays are in numpy order, the reverse of ggml's: a tensor with ne = [ne0, ne1, ne2, ne3] is an array of shape (ne3, ne2, ne1, ne0).
Every reference has a `*_f32` restatement beside it: the same op in np.float32 throughout with sequential accumulation; the GPU
tests derive their per-element bound from the restatement's own distance to the float64 result (never from the kernel's output)."""
import ctypes
import ctypes.util

import numpy as np

F32, F16, I32 = 0, 1, 26
NP_TYPE = {F32: np.float32, F16: np.float16, I32: np.int32}
f32, f64 = np.float32, np.float64

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.powf.restype = _libm.logf.restype = ctypes.c_float
_libm.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.logf.argtypes = [ctypes.c_float]


def powf(a, b):
    """the C library's powf: what the launchers call for theta_scale and the ALiBi bases (numpy's float32 power may differ in the last bit,
    and a last bit of theta_scale is p ulps of the angle of pair p)"""
    return f32(_libm.powf(float(f32(a)), float(f32(b))))


def logf(a):
    return f32(_libm.logf(float(f32(a))))


# ------------------------------------------------------------------------------------------------ error measures
def nmse(got, want):
    """test-backend-ops.cpp:325-327: sum of squared differences over sum of squares of the reference"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    return float(((got - want) ** 2).sum() / max((want ** 2).sum(), 1e-300))


def rel_rms(got, want):
    """largest element difference over the rms of the reference (the suite's per-element figure)"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def seq_sum_f32(x, axis=-1):
    """sequential float32 sum (np.sum is pairwise; cumsum is not)"""
    return np.take(np.cumsum(np.asarray(x, f32), axis=axis, dtype=f32), -1, axis=axis)


# ------------------------------------------------------------------------------------------------ binary ops, ggml broadcast
def repeat_to(b, shape):
    """ggml_can_repeat broadcast: b tiled along every dimension it is smaller in (element i of dst reads b[i mod ne])"""
    b = np.asarray(b)
    b = b.reshape((1,) * (len(shape) - b.ndim) + b.shape)
    assert all(s % t == 0 for s, t in zip(shape, b.shape)), (shape, b.shape)
    return np.tile(b, [s // t for s, t in zip(shape, b.shape)])


def binary(op, a, b, dtype=f64):
    """op in 'add', 'sub', 'mul', 'div'; dtype=np.float32 gives the single IEEE operation the kernel performs"""
    a = np.asarray(a, dtype)
    b = repeat_to(np.asarray(b, dtype), a.shape)
    with np.errstate(all="ignore"):
        return {"add": np.add, "sub": np.subtract, "mul": np.multiply, "div": np.divide}[op](a, b)


# ------------------------------------------------------------------------------------------------ unaries
GELU_A, GELU_C, GELU_QUICK_C = 0.044715, 0.79788456080286535587989211986876, -1.702     # the kernel's (ggml-cpu vec.h) constants
UNARIES = ("silu", "gelu", "gelu_quick", "relu", "tanh", "sigmoid", "neg", "exp", "scale")


def unary(name, x, p=None, dtype=f64):
    """the nine unaries (SCALE takes its factor in p); GELU in tanh form.  dtype=np.float32: the restatement"""
    x = np.asarray(x, dtype)
    one = dtype(1)
    with np.errstate(over="ignore"):
        if name == "scale":
            return x * dtype(f32(p))
        if name == "silu":
            return x / (one + np.exp(-x))
        if name == "gelu":
            return dtype(0.5) * x * (one + np.tanh(dtype(f32(GELU_C)) * x * (one + dtype(f32(GELU_A)) * x * x)))
        if name == "gelu_quick":
            return x * (one / (one + np.exp(dtype(f32(GELU_QUICK_C)) * x)))
        if name == "relu":
            return np.where(x > 0, x, dtype(0))
        if name == "tanh":
            return np.tanh(x)
        if name == "sigmoid":
            return one / (one + np.exp(-x))
        if name == "neg":
            return -x
        if name == "exp":
            return np.exp(x)
    raise ValueError(name)


def silu_mul(a, b, dtype=f64):
    return unary("silu", a, dtype=dtype) * np.asarray(b, dtype)


# ------------------------------------------------------------------------------------------------ RMS_NORM, NORM
def rms_norm(x, eps, w=None, b=None):
    """y = x / sqrt(mean(x^2) + eps) [* w]; with b the input is the float32 sum x + b, returned as well: (y, s)"""
    s = None
    if b is not None:
        s = (np.asarray(x, f32) + np.asarray(b, f32)).astype(f32)
        x = s
    x = np.asarray(x, f64)
    y = x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + f64(f32(eps)))
    if w is not None:
        y = y * np.asarray(w, f64)
    return y if b is None else (y, s)


def rms_norm_f32(x, eps, w=None, b=None):
    x = np.asarray(x, f32)
    if b is not None:
        x = x + np.asarray(b, f32)
    mean = seq_sum_f32(x * x)[..., None] / f32(x.shape[-1])
    y = x * (f32(1) / np.sqrt(mean + f32(eps), dtype=f32))
    return y * np.asarray(w, f32) if w is not None else y


def norm(x, eps):
    """LayerNorm without affine part: (x - mean) / sqrt(var + eps), the variance of the centred values"""
    x = np.asarray(x, f64)
    c = x - x.mean(axis=-1, keepdims=True)
    return c / np.sqrt((c * c).mean(axis=-1, keepdims=True) + f64(f32(eps)))


def norm_f32(x, eps):
    """the restatement.  ggml's CPU code takes both sums in double; in float32 the mean is taken in two steps (the sum, then the sum of
    what is left over), because one float32 sum of n values near m is only good to about n * ulp(n * m) / 2: for a row of 5000 values
    around 1000 with standard deviation 1 that is a few 1e-3 of the standard deviation, which is the whole signal after centring"""
    x = np.asarray(x, f32)
    n = f32(x.shape[-1])
    mean = seq_sum_f32(x)[..., None] / n
    mean = mean + seq_sum_f32(x - mean)[..., None] / n
    c = x - mean
    return c * (f32(1) / np.sqrt(seq_sum_f32(c * c)[..., None] / n + f32(eps), dtype=f32))


# ------------------------------------------------------------------------------------------------ SOFT_MAX
def alibi_slopes(n_head, max_bias, dtype=f64):
    """ggml-cpu.c:8290-8310: m0 = 2^(-max_bias / n_head_log2), m1 = 2^(-max_bias / 2 / n_head_log2);
    slope(h) = m0^(h + 1) for h < n_head_log2, else m1^(2 (h - n_head_log2) + 1); 1 when max_bias == 0"""
    if max_bias <= 0:
        return np.ones(n_head, dtype)
    n2 = 1 << int(np.floor(np.log2(n_head)))
    m0, m1 = dtype(2) ** dtype(-max_bias / n2), dtype(2) ** dtype(-(max_bias / 2) / n2)
    return np.array([m0 ** dtype(h + 1) if h < n2 else m1 ** dtype(2 * (h - n2) + 1) for h in range(n_head)], dtype)


def soft_max(x, mask=None, scale=1.0, max_bias=0.0, dtype=f64):
    """x (ne3, ne2, ne1, ne0); mask (rows >= ne1, ne0) f32 or f16, row i1 of it for every head and batch (row % ne01);
    v = x * scale + slope(head) * mask, softmax over the last axis.  dtype=np.float32: the restatement (sequential sum)"""
    x = np.asarray(x)
    assert x.ndim == 4
    v = np.asarray(x, dtype) * dtype(f32(scale))
    if mask is not None:
        m = np.asarray(mask)[:x.shape[2]].astype(dtype)
        v = v + alibi_slopes(x.shape[1], max_bias, dtype)[None, :, None, None] * m[None, None]
    e = np.exp(v - v.max(axis=-1, keepdims=True))
    if dtype is f32:
        return e * (f32(1) / seq_sum_f32(e)[..., None])
    return e / e.sum(axis=-1, keepdims=True)


# ------------------------------------------------------------------------------------------------ ROPE
def rope_corr_dims(n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow):
    """ggml_rope_yarn_corr_dims (ggml.c:3738-3754) in float32"""
    def corr_dim(n_rot):
        return f32(f32(f32(n_dims) * logf(f32(n_ctx_orig) / f32(f32(n_rot) * f32(2) * f32(np.pi)))) / f32(f32(2) * logf(freq_base)))
    start, end = np.floor(corr_dim(beta_fast)), np.ceil(corr_dim(beta_slow))
    return f32(max(start, 0)), f32(min(end, n_dims - 1))


def rope_angles(pos, n_dims, freq_base=10000.0, freq_scale=1.0, ext_factor=0.0, attn_factor=1.0, beta_fast=32.0, beta_slow=1.0,
                n_ctx_orig=8192, ff=None):
    """(theta [n_pos, n_dims / 2] float32, mscale float32): ggml_rope_cache_init + rope_yarn (ggml-cpu.c:8610-8648) with the CPU's
    float32 steps: theta by repeated multiply with theta_scale = powf(freq_base, -2 / n_dims), the YaRN ramp mix in float32"""
    half = n_dims // 2
    theta_scale = powf(freq_base, f32(-2.0) / f32(n_dims))
    corr0, corr1 = rope_corr_dims(n_dims, n_ctx_orig, freq_base, beta_fast, beta_slow)
    fs, ef = f32(freq_scale), f32(ext_factor)
    mscale = f32(attn_factor)
    if ef != 0:
        mscale = f32(mscale * f32(f32(1) + f32(f32(0.1) * logf(f32(1) / fs))))
    out = np.empty((len(pos), half), f32)
    with np.errstate(over="ignore"):
        for t, p0 in enumerate(pos):
            theta = f32(p0)
            for p in range(half):
                extrap = f32(theta / (f32(ff[p]) if ff is not None else f32(1)))
                interp = f32(fs * extrap)
                th = interp
                if ef != 0:
                    y = f32(f32(f32(p) - corr0) / max(f32(0.001), f32(corr1 - corr0)))
                    mix = f32(f32(f32(1) - min(f32(1), max(f32(0), y))) * ef)
                    th = f32(f32(interp * f32(f32(1) - mix)) + f32(extrap * mix))
                out[t, p] = th
                theta = f32(theta * theta_scale)
    return out, mscale


def rope(x, pos, n_dims, neox=False, dtype=f64, **kw):
    """x (ne3, ne2 = positions, ne1 = heads, ne0); pairs (2p, 2p + 1) in normal mode, (p, p + n_dims / 2) in NEOX; channels from
    n_dims on pass through.  cos / sin in float64 of the float32 angle.  dtype=np.float32: the restatement"""
    x = np.asarray(x)
    assert x.ndim == 4 and x.shape[1] == len(pos)
    th, mscale = rope_angles(pos, n_dims, **kw)
    c = (np.cos(th.astype(dtype)) * dtype(mscale))[None, :, None, :]
    s = (np.sin(th.astype(dtype)) * dtype(mscale))[None, :, None, :]
    out = np.asarray(x, dtype).copy()
    half = n_dims // 2
    ia = np.arange(half) if neox else 2 * np.arange(half)
    ib = ia + half if neox else ia + 1
    x0, x1 = np.asarray(x[..., ia], dtype), np.asarray(x[..., ib], dtype)
    out[..., ia] = x0 * c - x1 * s
    out[..., ib] = x0 * s + x1 * c
    return out


# ------------------------------------------------------------------------------------------------ CPY, GET_ROWS
def strided_offsets(ne, nb):
    """byte offset of every element, in the tensor's index order (i0 fastest)"""
    ne, nb = list(ne) + [1] * (4 - len(ne)), list(nb)
    o = np.zeros(1, np.int64)
    for n, b in zip(ne, nb):
        o = (o[None, :] + (np.arange(n, dtype=np.int64) * b)[:, None]).reshape(-1)
    return o


def cpy(src_bytes, s_type, s_ne, s_nb, s_off, dst_bytes, d_type, d_ne, d_nb, d_off):
    """ggml_compute_forward_dup: element i of src (in src's index order) to element i of dst (in dst's), converted; returns the new dst
    bytes.  Written with explicit offsets so that it shares nothing with numpy's own strided views"""
    so, do = strided_offsets(s_ne, s_nb) + s_off, strided_offsets(d_ne, d_nb) + d_off
    assert len(so) == len(do)
    st, dt = np.dtype(NP_TYPE[s_type]), np.dtype(NP_TYPE[d_type])
    src = np.asarray(src_bytes, np.uint8)
    vals = src[so[:, None] + np.arange(st.itemsize)].copy().view(st).reshape(-1).astype(dt)
    out = np.array(dst_bytes, np.uint8, copy=True)
    out[do[:, None] + np.arange(dt.itemsize)] = vals.view(np.uint8).reshape(-1, dt.itemsize)
    return out


def get_rows(a, ids):
    """a (ne3, ne2, ne1, ne0) already as float32 values; ids (ne12, ne11, ne10) int32: dst (ne12, ne11, ne10, ne0) with
    dst[i12, i11, i10] = a[i12, i11, ids[i12, i11, i10]]"""
    a, ids = np.asarray(a), np.asarray(ids)
    out = np.empty(ids.shape + (a.shape[-1],), f32)
    for i12 in range(ids.shape[0]):
        for i11 in range(ids.shape[1]):
            out[i12, i11] = a[i12, i11][ids[i12, i11]]
    return out


# ------------------------------------------------------------------------------------------------ MUL_MAT_F
def mul_mat(a, b, a_f16=False):
    """a (ne03, ne02, M, K), b (ne13, ne12, N, K) -> (ne13, ne12, N, M) in float64; a broadcast over dims 2 / 3 as i12 / r2, i13 / r3.
    a_f16: src1 is rounded to f16 first (vec_dot_type of an F16 src0)"""
    a, b = np.asarray(a), np.asarray(b, f32)
    if a_f16:
        b = b.astype(np.float16)
    r3, r2 = b.shape[0] // a.shape[0], b.shape[1] // a.shape[1]
    out = np.empty(b.shape[:3] + (a.shape[2],), f64)
    for i13 in range(b.shape[0]):
        for i12 in range(b.shape[1]):
            out[i13, i12] = b[i13, i12].astype(f64) @ a[i13 // r3, i12 // r2].astype(f64).T
    return out


def mul_mat_f32(a, b, a_f16=False):
    """the restatement: float32 products added one after the other along K"""
    a, b = np.asarray(a), np.asarray(b, f32)
    if a_f16:
        b = b.astype(np.float16)
    r3, r2 = b.shape[0] // a.shape[0], b.shape[1] // a.shape[1]
    out = np.empty(b.shape[:3] + (a.shape[2],), f32)
    for i13 in range(b.shape[0]):
        for i12 in range(b.shape[1]):
            out[i13, i12] = seq_sum_f32(b[i13, i12].astype(f32)[:, None, :] * a[i13 // r3, i12 // r2].astype(f32)[None, :, :])
    return out


# ------------------------------------------------------------------------------------------------ ARGSORT, SUM_ROWS
def argsort(x, desc=False):
    """stable, ties by index in both orders: element i goes to the position 'number of elements that sort before it'"""
    x = np.asarray(x, f32)
    return np.argsort(-x if desc else x, axis=-1, kind="stable").astype(np.int32)


def sum_rows(x, dtype=f64):
    x = np.asarray(x)
    return (seq_sum_f32(x) if dtype is f32 else x.astype(f64).sum(axis=-1))[..., None]


# ------------------------------------------------------------------------------------------------ operands
class Buf:
    """One operand: a view (type, ne, nb, byte offset) of a backing buffer that is allocated just large enough for it plus `tail`
    bytes and filled with sentinel bytes, so that strided, permuted and misaligned views are one line each and a test can compare
    every byte outside the view with what it held before the launch.

        b = Buf(F32, [100, 5], nb=[4, 416, 2080, 2080], off=4).put(values)      # rows 16 bytes apart from dense, pointer offset by 4
        t = b.tensor()                      # QmmTensor over b.dev() (the device copy, made on first use)
        got = b.read()                      # the view's values after the launch, shape (ne3, ne2, ne1, ne0)
        assert b.outside_untouched()
    """

    def __init__(self, type_, ne, nb=None, off=0, tail=64, seed=0, share=None):
        self.type, self.dt = type_, np.dtype(NP_TYPE[type_])
        self.ne = list(ne) + [1] * (4 - len(ne))
        es = self.dt.itemsize
        if nb is None:
            nb, acc = [], es
            for n in self.ne:
                nb.append(acc)
                acc *= n
        self.nb, self.off = list(nb), off
        self.span = off + sum((n - 1) * b for n, b in zip(self.ne, self.nb)) + es
        if share is not None:                 # a second view of another operand's buffer (in-place ops, views of a cache)
            self.root = share.root
            assert self.span <= len(self.root.host)
        else:
            self.root = self
            self.host = np.random.default_rng(1000 + seed).integers(0, 256, self.span + tail, dtype=np.uint8)
            self._dev = None
            self.before = None

    @property
    def shape(self):
        return tuple(self.ne[::-1])

    def view(self, raw):
        return np.ndarray(shape=self.shape, dtype=self.dt, buffer=raw, offset=self.off, strides=tuple(self.nb[::-1]))

    def put(self, values):
        self.view(self.root.host)[...] = np.asarray(values).astype(self.dt).reshape(self.shape)
        return self

    def values(self):
        return np.array(self.view(self.root.host))

    def dev(self):
        import torch
        r = self.root
        if r._dev is None:
            r.before = r.host.copy()
            r._dev = torch.from_numpy(r.host.copy()).cuda()
        return r._dev

    def tensor(self, op_params=()):
        from ggml_hexagon_amd.capi import QmmTensor
        return QmmTensor.make(self.type, self.ne, nb=self.nb, data=self.dev().data_ptr() + self.off, op_params=op_params)

    def download(self):
        return self.dev().cpu().numpy()

    def read(self, raw=None):
        return np.array(self.view(self.download() if raw is None else raw))

    def inside(self):
        m = np.zeros(len(self.root.host), bool)
        o = strided_offsets(self.ne, self.nb) + self.off
        m[(o[:, None] + np.arange(self.dt.itemsize)).reshape(-1)] = True
        return m

    def outside_untouched(self, raw=None):
        """every byte of the backing buffer that is not an element of this view still holds what was uploaded"""
        raw = self.download() if raw is None else raw
        keep = ~self.inside()
        return bool(np.array_equal(raw[keep], self.root.before[keep]))
