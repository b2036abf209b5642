"""Numpy restatements of quantize_row_q4_0_ref / q4_1_ref / q5_0_ref / q5_1_ref and dequantize_row_q4_0 / q4_1 / q5_0 / q5_1
(ggml/src/ggml-quants.c:31-191, 255-347), every step rounded to float32 on its own, nothing fused; the rows with the value edges of these
quantizers that tests/golden/kblk_quantize.npz pins to the reference's own bytes; and the descriptor helpers the K-cache tests of these
four types share.  Helper of tests/test_kblk_host.py, tests/test_gpu_kblk.py and profiles/tools/kblk_times.py.

    python tests/kblk_refs.py            rewrites tests/golden/kblk_quantize.npz from oracle/_ref (the reference's quantize_row_*_ref)
"""
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
GOLDEN = ROOT / "tests" / "golden" / "kblk_quantize.npz"

Q4_0, Q4_1, Q5_0, Q5_1 = 2, 3, 6, 7
TYPES = (Q4_0, Q4_1, Q5_0, Q5_1)
NAMES = {Q4_0: "q4_0", Q4_1: "q4_1", Q5_0: "q5_0", Q5_1: "q5_1"}
BLOCK = {Q4_0: 18, Q4_1: 20, Q5_0: 22, Q5_1: 24}          # bytes per 32 values: f16 d, [f16 m], [4 bytes qh], 16 bytes of nibbles
HAS_M = {Q4_0: False, Q4_1: True, Q5_0: False, Q5_1: True}
HAS_QH = {Q4_0: False, Q4_1: False, Q5_0: True, Q5_1: True}
f32 = np.float32


def qh_off(t):
    return 4 if HAS_M[t] else 2


def qs_off(t):
    return qh_off(t) + (4 if HAS_QH[t] else 0)


def quantize(t, x):
    """x f32 [rows, k] -> uint8 [rows, k / 32 * BLOCK[t]], as quantize_row_<t>_ref"""
    x = np.ascontiguousarray(x, f32)
    rows, k = x.shape
    xb = x.reshape(-1, 32)
    nb = xb.shape[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        if HAS_M[t]:
            mn, mx = xb.min(axis=1), xb.max(axis=1)
            d = ((mx - mn).astype(f32) / f32(15 if t == Q4_1 else 31)).astype(f32)
            idv = np.where(d != 0, (f32(1) / d).astype(f32), f32(0)).astype(f32)
            x0 = ((xb - mn[:, None]).astype(f32) * idv[:, None]).astype(f32)          # a rounded subtract, then a rounded multiply
            y = (x0 + f32(0.5)).astype(f32)
        else:
            first = np.argmax(np.abs(xb), axis=1)                                      # the first element of greatest magnitude (strict <)
            mx = xb[np.arange(nb), first]
            d = (mx / f32(-8 if t == Q4_0 else -16)).astype(f32)
            idv = np.where(d != 0, (f32(1) / d).astype(f32), f32(0)).astype(f32)
            x0 = (xb * idv[:, None]).astype(f32)
            y = (x0 + f32(8.5 if t == Q4_0 else 16.5)).astype(f32)
    q = y.astype(np.int32)                                                             # toward zero
    if t == Q5_1:
        q = q & 0xFF                                                                   # (uint8_t): no clamp
    else:
        q = np.minimum(31 if t == Q5_0 else 15, q)
    out = np.zeros((nb, BLOCK[t]), np.uint8)
    out[:, 0:2] = d.astype(np.float16).view(np.uint8).reshape(nb, 2)
    if HAS_M[t]:
        out[:, 2:4] = mn.astype(np.float16).view(np.uint8).reshape(nb, 2)
    if HAS_QH[t]:
        qh = np.zeros(nb, np.uint32)
        for e in range(32):
            qh |= (((q[:, e] >> 4) & 1).astype(np.uint32) << np.uint32(e))
        out[:, qh_off(t):qh_off(t) + 4] = qh.view(np.uint8).reshape(nb, 4)
    out[:, qs_off(t):] = ((q[:, :16] & 15) | ((q[:, 16:] & 15) << 4)).astype(np.uint8)
    return out.reshape(rows, -1)


def codes(t, blocks):
    """uint8 [..., BLOCK[t]] -> int32 [..., 32]: the 4- or 5-bit codes in element order"""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, BLOCK[t])
    qs = b[:, qs_off(t):].astype(np.int32)
    q = np.concatenate([qs & 15, qs >> 4], axis=1)
    if HAS_QH[t]:
        qh = np.ascontiguousarray(b[:, qh_off(t):qh_off(t) + 4]).view(np.uint32).reshape(-1)
        q |= (((qh[:, None] >> np.arange(32, dtype=np.uint32)[None, :]) & 1) << 4).astype(np.int32)
    return q.reshape(blocks.shape[:-1] + (32,))


def scales(t, blocks):
    """uint8 [..., BLOCK[t]] -> (d, m) as uint16 bit patterns of their f16 values (m None without one)"""
    b = np.ascontiguousarray(blocks, np.uint8).reshape(-1, BLOCK[t])
    d = np.ascontiguousarray(b[:, 0:2]).view(np.uint16).reshape(blocks.shape[:-1])
    m = np.ascontiguousarray(b[:, 2:4]).view(np.uint16).reshape(blocks.shape[:-1]) if HAS_M[t] else None
    return d, m


def dequantize(t, w, k):
    """w uint8 [rows, k / 32 * BLOCK[t]] -> f32 [rows, k], as dequantize_row_<t>: (q - 8) * d, q * d + m, (q - 16) * d, q * d + m"""
    b = np.ascontiguousarray(w, np.uint8).reshape(-1, BLOCK[t])
    q = codes(t, b).astype(f32)
    du, mu = scales(t, b)
    d = du.view(np.float16).astype(f32)[:, None]
    if HAS_M[t]:
        out = ((q * d).astype(f32) + mu.view(np.float16).astype(f32)[:, None]).astype(f32)
    else:
        out = ((q - f32(8 if t == Q4_0 else 16)).astype(f32) * d).astype(f32)
    return out.reshape(-1, k)


# ---- the rows the golden file pins

def _below(v):
    return np.nextafter(f32(v), f32(-np.inf))


def _halves(first, ties):
    """a block that starts with `first` and goes on with each tie value and the float just below it"""
    b = list(first)
    for v in ties:
        b += [f32(v), _below(v)]
    assert len(b) <= 32
    return np.array(b + [f32(0.25)] * (32 - len(b)), f32)


def edge_blocks():
    """the value edges of the four quantizers, one block of 32 each"""
    rng = np.random.default_rng(77)
    n = lambda: rng.normal(0, 1, 32).astype(f32)
    pos, neg = n(), n()
    pos[11], neg[19] = 4.75, -5.125                                    # the greatest magnitude positive / negative
    plus_first, minus_first = n(), n()
    plus_first[7], plus_first[20] = 3.5, -3.5                          # +a in front of -a at the greatest magnitude, and the other way round
    minus_first[7], minus_first[20] = -3.5, 3.5
    # max = -8: Q4_0 has d = id = 1 (x + 8.5: 8.0 hits the clamp, k + 0.5 sits exactly on an integer), Q5_0 d = 0.5, id = 2 (2 x + 16.5: k / 2 + 0.25)
    clamp = _halves([-8.0, 8.0], [-7.5, -3.5, -0.5, 0.5, 2.5, 6.5, 7.5, -3.25, -0.25, 0.25, 2.75, 7.75, 7.25])
    # min = 0, max = 15: Q4_1 has d = id = 1 (x + 0.5 on integers at k + 0.5); min = 0, max = 31: the same for Q5_1, and 15.5 / 16 cross its fifth bit
    q41 = _halves([0.0, 15.0], [0.5, 1.5, 6.5, 7.5, 8.5, 13.5, 14.5, 14.75, 1.0, 15.0])
    q51 = _halves([0.0, 31.0], [0.5, 1.5, 14.5, 15.5, 16.0, 16.5, 29.5, 30.5, 30.75, 31.0])
    const = np.full(32, 3.3, f32)                                      # d = 0 for Q4_1 / Q5_1
    odd_min = n()
    odd_min[5] = -4.2345678                                            # a min that is no f16 value
    return [np.zeros(32, f32), pos, neg, plus_first, minus_first, clamp, q41, q51, const, odd_min]


def golden_inputs():
    """the two sources of the CPY tests: `a` [64, 3] contiguous, `b` memory [128, 2, 5] (read as [128, 5, 2] through a permute); the edge
    blocks lead both, N(0, 1) otherwise"""
    e = edge_blocks()
    rng = np.random.default_rng(78)
    a = rng.normal(0, 1, (3, 64)).astype(f32)
    a.reshape(-1, 32)[:6] = e[:6]
    b = rng.normal(0, 1, (10, 128)).astype(f32)
    b.reshape(-1, 32)[:10] = e[::-1]
    return a, b


def load_golden():
    return dict(np.load(GOLDEN))


def write_golden():
    import sys
    sys.path.insert(0, str(ROOT))
    from oracle.pyoracle import RefGgml
    ref = RefGgml()
    a, b = golden_inputs()
    out = {"a": a, "b": b}
    for t in TYPES:
        out[f"a_{NAMES[t]}"] = ref.quantize_weights(t, a)
        out[f"b_{NAMES[t]}"] = ref.quantize_weights(t, b)
    GOLDEN.parent.mkdir(exist_ok=True)
    np.savez_compressed(GOLDEN, **out)
    print(f"wrote {GOLDEN} ({GOLDEN.stat().st_size} bytes)")


# ---- descriptors

def kblk_tensor(t, ne, nb=None, data=1 << 20):
    """a descriptor of block type t: contiguous rows of blocks unless byte strides are given"""
    from ggml_hexagon_amd.capi import QmmTensor
    ne = list(ne) + [1] * (4 - len(ne))
    if nb is None:
        nb, acc = [BLOCK[t]], ne[0] // 32 * BLOCK[t]
        for n in ne[1:]:
            nb.append(acc)
            acc *= n
    nb = list(nb)
    while len(nb) < 4:
        nb.append(nb[-1] * ne[len(nb) - 1])
    return QmmTensor.make(t, ne, nb=nb, data=data)


if __name__ == "__main__":
    write_golden()
