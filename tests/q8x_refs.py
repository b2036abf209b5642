"""QMM_PREC_Q8_EXACT on Q2_K / Q3_K / IQ4_XS: the inputs of tests/test_gpu_q8_exact_more.py, and a numpy restatement of what
mfma_q8x_kernel<10 | 11 | 23> computes (csrc/qmm_mfma_q8x.hiph): the weight times its integer sub-block scale as int8 planes, integer sums
over a whole 256-weight superblock, one f32 step per superblock in the kernel's expression order, f32 throughout.
tests/test_q8_exact_more_host.py holds it against the CPU oracle on the same inputs, which shows without a GPU that the bar can be met."""
import numpy as np

import ggml_hexagon_amd.synth as synth
from oracle.pyoracle import IQ4_XS, Q2_K, Q3_K, TYPE_NAMES

MORE = (Q2_K, Q3_K, IQ4_XS)
IDS = [TYPE_NAMES[t] for t in MORE]
BAR = 2e-5                       # max |err| / rms(want): "only the f32 summation order differs from the CPU backend" (test_gpu_parity.py)
KVALUES_IQ4NL = np.array([-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113], np.int32)      # ggml-common.h


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def uniform(seed, n, k):
    return np.random.default_rng(seed).uniform(-1, 1, (n, k)).astype(np.float32)


# ----------------------------------------------------------------------------- the inputs of the GPU tests

GRID_N = (9, 33, 64, 129)
RAGGED = ((16, 256, 9), (77, 1024, 130), (130, 512, 257), (48, 14336, 96))


def grid_case(t, n):
    k, m = 2048, 200
    return synth.synth_weights(t, m, k, seed=20 + t, sigma=0.3), k, uniform(n, n, k)


def ragged_case(t, m, k, n):
    return synth.synth_weights(t, m, k, seed=m, sigma=0.2), k, uniform(n, n, k)


def strided_case(t):
    m, k, n = 77, 1024, 130
    return synth.synth_weights(t, m, k, seed=7, sigma=0.2), k, uniform(5, n, k)


def edge_x(k, n=40):
    rng = np.random.default_rng(11)
    x = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    x[:8] = 1.0
    x[8:16] = -1.0
    x[16:24] = np.abs(x[16:24])
    return x                                                     # whole rows of q8 at +127 / -127


def f16_bytes(v):
    return np.array([v], np.float16).view(np.uint8)


def _q2k_all_ff():
    blk = np.full(84, 0xFF, np.uint8)
    blk[80:82] = f16_bytes(2.0 ** -6)
    blk[82:84] = f16_bytes(2.0 ** -8)
    return blk


def _q3k(qs, hmask, scale_field):
    """a block whose 16 six-bit scale fields all hold `scale_field`"""
    blk = np.zeros(110, np.uint8)
    blk[0:32] = hmask
    blk[32:96] = qs
    blk[96:104] = (scale_field & 15) * 0x11
    blk[104:108] = (scale_field >> 4) * 0x55
    blk[108:110] = f16_bytes(2.0 ** -8)
    return blk


def _iq4xs(index, scale_field):
    blk = np.zeros(136, np.uint8)
    blk[0:2] = f16_bytes(2.0 ** -12)
    blk[2:4] = np.array([(scale_field >> 4) * 0x5555], np.uint16).view(np.uint8)
    blk[4:8] = (scale_field & 15) * 0x11
    blk[8:136] = index * 0x11
    return blk


# name -> (type, block, the v = sc * q it holds in every weight)
EDGES = {
    "q2_K-sc15-m15-q3":      (Q2_K, _q2k_all_ff(), 45),           # every byte 0xFF: the top of the one plane and of the mins plane
    "q3_K-sc-32-q-4":        (Q3_K, _q3k(0x00, 0x00, 0), 128),    # all-zero block but d: +128 does not fit int8, the hi plane carries it
    "q3_K-sc31-q-4":         (Q3_K, _q3k(0x00, 0x00, 63), -124),
    "q3_K-sc-32-q3":         (Q3_K, _q3k(0xFF, 0xFF, 0), -96),
    "iq4_xs-ls-32-val-127":  (IQ4_XS, _iq4xs(0, 0), 4064),        # all-zero block but d: the top of the hi plane
    "iq4_xs-ls31-val-127":   (IQ4_XS, _iq4xs(0, 63), -3937),      # its bottom
    "iq4_xs-ls-32-val113":   (IQ4_XS, _iq4xs(15, 0), -3616),
}


def edge_case(name):
    t, blk, _ = EDGES[name]
    m, k = 40, 2048
    return t, np.tile(blk, (m, k // 256)), k, edge_x(k)


def f16_top_case(t):
    """one block of the matrix with d = 0x7BFF (65504, and dmin too for Q2_K): beyond what the default mode's f16 operands can hold"""
    k, m, n = 512, 64, 40
    w = synth.synth_weights(t, m, k, seed=3, sigma=0.05).reshape(m, -1, synth.TYPE_SIZE[t])
    top = np.array([0x7BFF], np.uint16).view(np.uint8)
    if t == Q2_K:
        w[5, 1, 80:82] = top
        w[5, 1, 82:84] = top
    elif t == Q3_K:
        w[5, 1, 108:110] = top
    else:
        w[5, 1, 0:2] = top
    return w.reshape(m, -1), k, uniform(9, n, k)


# ----------------------------------------------------------------------------- the kernel's arithmetic

def _f16(b):
    """uint8 [..., 2] -> f32 [...]"""
    return np.ascontiguousarray(b).view(np.float16)[..., 0].astype(np.float32)


def _low2(qs):
    """Q2_K / Q3_K qs[..., 64] -> the two low bits of the block's 256 weights as [..., 16 sub-blocks, 16]"""
    out = np.empty(qs.shape[:-1] + (16, 16), np.int32)
    for g in range(16):
        q = qs[..., 32 * (g >> 3) + 16 * (g & 1): 32 * (g >> 3) + 16 * (g & 1) + 16].astype(np.int32)
        out[..., g, :] = (q >> (2 * ((g & 7) >> 1))) & 3
    return out


def unpack(t, w, k):
    """w uint8 [M, row bytes] -> v = sc * q int32 [M, nb, 256], the mins plane int32 [M, nb, 256] or None, d f32 [M, nb], dmin f32 [M, nb] or None"""
    m, nb = w.shape[0], k // 256
    blk = np.ascontiguousarray(w, np.uint8).reshape(m, nb, synth.TYPE_SIZE[t])
    if t == Q2_K:
        sc = blk[..., 0:16].astype(np.int32)
        v = (sc & 15)[..., None] * _low2(blk[..., 16:80])
        mn = np.broadcast_to((sc >> 4)[..., None], v.shape)
        return v.reshape(m, nb, 256), mn.reshape(m, nb, 256), _f16(blk[..., 80:82]), _f16(blk[..., 82:84])
    if t == Q3_K:
        hm, s12 = blk[..., 0:32].astype(np.int32), blk[..., 96:108].astype(np.int32)
        q = _low2(blk[..., 32:96])
        sc = np.empty(blk.shape[:2] + (16,), np.int32)
        for g in range(16):
            q[..., g, :] -= np.where((hm[..., 16 * (g & 1): 16 * (g & 1) + 16] >> (g >> 1)) & 1, 0, 4)
            lo = (s12[..., g] & 15) if g < 8 else (s12[..., g - 8] >> 4)
            sc[..., g] = (lo | (((s12[..., 8 + (g & 3)] >> (2 * (g >> 2))) & 3) << 4)) - 32
        return (sc[..., None] * q).reshape(m, nb, 256), None, _f16(blk[..., 108:110]), None
    assert t == IQ4_XS
    sh = blk[..., 2].astype(np.int32) | (blk[..., 3].astype(np.int32) << 8)
    sl, qs = blk[..., 4:8].astype(np.int32), blk[..., 8:136].astype(np.int32)
    v = np.empty(blk.shape[:2] + (8, 32), np.int32)
    for ib in range(8):
        ls = ((sl[..., ib // 2] >> (4 * (ib & 1))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
        b16 = qs[..., 16 * ib: 16 * ib + 16]
        v[..., ib, :16] = (ls - 32)[..., None] * KVALUES_IQ4NL[b16 & 15]
        v[..., ib, 16:] = (ls - 32)[..., None] * KVALUES_IQ4NL[b16 >> 4]
    return v.reshape(m, nb, 256), None, _f16(blk[..., 0:2]), None


def _int_dot(plane, q8):
    """plane int [M, nb, 256] (inside int8), q8 int8 [N, nb, 256] -> the MFMA's exact sums int64 [nb, N, M] (below 2^53 in f64)"""
    assert plane.min() >= -128 and plane.max() <= 127
    s = np.matmul(q8.transpose(1, 0, 2).astype(np.float64), plane.transpose(1, 2, 0).astype(np.float64))
    return s.astype(np.int64)


def kernel_ref(oracle, t, w, k, x):
    """dst f32 [N, M] as mfma_q8x_kernel<t> forms it from the Q8_K rows of x"""
    v, mn, dw, dmw = unpack(t, w, k)
    n, nb = x.shape[0], k // 256
    a = oracle.quantize_act(t, x).reshape(n, nb, 292)           # block_q8_K: d f32, qs[256] int8, bsums[16] int16 (not read: the mins plane runs on qs)
    da = np.ascontiguousarray(a[..., 0:4]).view(np.float32)[..., 0]
    q8 = np.ascontiguousarray(a[..., 4:260]).view(np.int8)
    if t == Q2_K:                                                # one plane as it is
        sumi = _int_dot(v, q8)
    else:                                                        # v = 128 * hi + lo, lo in 0..127
        sumi = (_int_dot(v >> 7, q8) << 7) + _int_dot(v & 127, q8)
    assert np.abs(sumi).max() < 2 ** 27
    summs = _int_dot(mn, q8) if mn is not None else None
    acc = np.zeros((n, w.shape[0]), np.float32)
    for b in range(nb):
        dall = da[:, b, None] * dw[None, :, b]                   # f32 products, each rounded (contraction off in the kernel)
        if t == Q2_K:
            acc += dall * sumi[b].astype(np.float32) - (da[:, b, None] * dmw[None, :, b]) * summs[b].astype(np.float32)
        else:
            acc += dall * sumi[b].astype(np.float32)
    return acc
