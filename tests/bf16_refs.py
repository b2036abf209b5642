"""numpy side of the BF16-weight tests: ggml's f32 -> bf16 rounding (ggml_compute_fp32_to_bf16 for non-NaN values: nearest even on
the upper 16 bits, subnormals kept), the exact widening, and the float64 reference of a MUL_MAT on BF16 weights with its error bound.
No test code in here; test_bf16_host.py checks the rounding against hand-written cases."""
import numpy as np


def f32_to_bf16(x):
    """uint16 bits: (u + 0x7fff + ((u >> 16) & 1)) >> 16 on the f32 bits u"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(h):
    """the exact widening: the 16 bits become the upper half of an f32"""
    return (np.ascontiguousarray(h, np.uint16).astype(np.uint32) << 16).view(np.float32)


def mul_mat_ref(w_bits, x):
    """w_bits uint16 [M, K], x f32 [N, K] -> (want, absum), float64 [N, M]:
    want = sum_k widen(bf16(x_k)) * widen(w_k), absum = sum_k |the same products|"""
    w = bf16_to_f32(w_bits).astype(np.float64)
    xr = bf16_to_f32(f32_to_bf16(x)).astype(np.float64)
    return xr @ w.T, np.abs(xr) @ np.abs(w).T


def bound(k, absum):
    """bf16 x bf16 products are exact in f32, so only the K - 1 additions round (2^-24 relative each, of a partial sum that is at most
    absum); the factor 2 covers truncating adds inside the MFMA.  Derived, not measured."""
    return 2.0 * k * 2.0 ** -24 * absum
