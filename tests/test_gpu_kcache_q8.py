"""GPU parity of the Q8_0 K cache in the kernel library (csrc/qmm_kcache.hiph, planned by csrc/qmm_kcache_plan.h): CPY f32 -> Q8_0 byte for
byte against the CPU oracle's quantize_row_q8_0 in both act modes, CPY Q8_0 -> f32 / f16 against its dequantizer, and the two attention
entry points with k in Q8_0 against f64 numpy on the CPU's own arithmetic (few tokens: the oracle's Q8_0 x Q8_0 scores; prompt: K as
f16(d * q)), at the bounds of the F16-cache tests (tests/test_gpu_layer_ops.py): nothing new is rounded."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle.pyoracle import ACT_REF, ACT_X86, Q8_0  # noqa: E402

F32, F16 = 0, 1
QUANTIZE, UNPACK_F32, UNPACK_F16 = "cpy_q8_0_quantize_kernel", "cpy_q8_0_unpack_kernel<f32>", "cpy_q8_0_unpack_kernel<f16>"


@pytest.fixture(scope="module")
def qmm():
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


@pytest.fixture(scope="module")
def oracle():
    from oracle.pyoracle import Oracle
    return Oracle()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def q8_tensor(t, ne, nb=None):
    """a Q8_0 descriptor over the bytes of torch tensor t: contiguous rows of blocks unless byte strides are given"""
    from ggml_hexagon_amd.capi import QmmTensor
    ne = list(ne) + [1] * (4 - len(ne))
    if nb is None:
        nb, acc = [34], ne[0] // 32 * 34
        for n in ne[1:]:
            nb.append(acc)
            acc *= n
    return QmmTensor.make(Q8_0, ne, nb=list(nb), data=t.data_ptr())


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def edge_rows(n_rows, k, seed):
    """N(0, 1) rows with, in row 0: an all-zero block; a block whose largest value is negative; a block with amax = 127 (d = id = 1 in both
    act modes) that holds 2.5, -3.5 and 0.5: x * id exactly on .5, where roundf (ref) and rint (x86) part"""
    x = np.random.default_rng(seed).normal(0, 1, (n_rows, k)).astype(np.float32)
    x[0, 0:32] = 0.0
    x[0, 32:64] = -np.abs(x[0, 32:64])
    x[0, 40] = -7.25
    if k >= 96:
        x[0, 64:96] = np.round(x[0, 64:96] * 8)
        x[0, 64:68] = [127.0, 2.5, -3.5, 0.5]
    else:
        x[1, 0:32] = np.round(x[1, 0:32] * 8)
        x[1, 0:4] = [127.0, 2.5, -3.5, 0.5]
    return x


@pytest.mark.parametrize("act_mode", [ACT_REF, ACT_X86], ids=["ref", "x86"])
@pytest.mark.parametrize("shape", ["64x3", "128x2x5-permuted"])
def test_cpy_f32_to_q8_0_is_the_cpu_quantizer(qmm, oracle, shape, act_mode):
    from ggml_hexagon_amd import capi
    if shape == "64x3":
        rows = edge_rows(3, 64, 1)
        src = dev(rows)
        ts = capi.QmmTensor.make(F32, [64, 3], data=src.data_ptr())
        ne_d = [64, 3]
    else:
        base = edge_rows(10, 128, 2).reshape(5, 2, 128)                  # memory [128, 2, 5]; read as [128, 5, 2] through permute(0, 2, 1, 3)
        src = dev(base)
        ts = capi.QmmTensor.make(F32, [128, 5, 2], nb=[4, 1024, 512, 5120], data=src.data_ptr())
        rows = base.transpose(1, 0, 2).reshape(10, 128)                  # src's index order: i1 (the 5) inside i2 (the 2)
        ne_d = [1280]                                                    # element i of src is element i of dst: any contiguous shape
    want = oracle.quantize_act(Q8_0, rows, act_mode).reshape(-1)
    assert not np.array_equal(want, oracle.quantize_act(Q8_0, rows, ACT_X86 if act_mode == ACT_REF else ACT_REF).reshape(-1))   # the tie block tells the modes apart
    out = torch.full((want.size + 34,), 0xA5, dtype=torch.uint8, device="cuda")
    qmm.set_act_mode(act_mode)
    try:
        labels = qmm.trace(lambda: qmm.op(capi.OP_CPY, q8_tensor(out, ne_d), ts))
        got = out.cpu().numpy()
    finally:
        qmm.set_act_mode(ACT_REF)
    assert labels == (QUANTIZE,), labels
    assert np.array_equal(got[:want.size], want), np.flatnonzero(got[:want.size] != want)[:8]
    assert (got[want.size:] == 0xA5).all()                               # nothing behind the last block


@pytest.mark.parametrize("dst_type", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", ["128x6", "64x4x3-permuted"])
def test_cpy_q8_0_to_float_is_the_cpu_dequantizer(qmm, oracle, shape, dst_type):
    from ggml_hexagon_amd import capi
    k, n_rows = (128, 6) if shape == "128x6" else (64, 12)
    blocks = oracle.quantize_act(Q8_0, edge_rows(n_rows, k, 3), ACT_REF).reshape(n_rows, k // 32, 34).copy()
    blocks[1, 0, 2:34] = np.tile(np.array([0x80, 0x7F], np.uint8), 16)    # int8 -128 and 127
    blocks[2, 1, 0:2] = 0                                                # d = 0
    src = dev(blocks.reshape(-1))
    if shape == "128x6":
        ts, rows = q8_tensor(src, [128, 6]), blocks
    else:                                                                # memory [64, 4, 3] (rows of 68 bytes), read as [64, 3, 4]
        ts = q8_tensor(src, [64, 3, 4], nb=[34, 272, 68, 816])
        rows = blocks.reshape(3, 4, 2, 34).transpose(1, 0, 2, 3).reshape(12, 2, 34)
    want = oracle.dequantize(Q8_0, rows.reshape(n_rows, -1), k).reshape(-1)
    assert (rows[:, :, 2:] == 0x80).any() and (want == 0).any()
    out = torch.zeros(want.size + 8, dtype=torch.float32 if dst_type == F32 else torch.float16, device="cuda")
    td = capi.QmmTensor.make(dst_type, [k, n_rows], data=out.data_ptr())
    labels = qmm.trace(lambda: qmm.op(capi.OP_CPY, td, ts))
    assert labels == ((UNPACK_F32,) if dst_type == F32 else (UNPACK_F16,)), labels
    got = out.cpu().numpy()
    assert np.array_equal(got[:want.size], want if dst_type == F32 else want.astype(np.float16))      # d * q is exact in f32: one rounding
    assert (got[want.size:] == 0).all()
    # ... and with a destination off 16 bytes (the scalar stores)
    es = 4 if dst_type == F32 else 2
    td2 = capi.QmmTensor.make(dst_type, [k, n_rows], data=out.data_ptr() + es)
    out.zero_()
    qmm.op(capi.OP_CPY, td2, ts)
    got = out.cpu().numpy()
    assert got[0] == 0 and np.array_equal(got[1:want.size + 1], want if dst_type == F32 else want.astype(np.float16)) and (got[want.size + 1:] == 0).all()


# ---- attention

H, HK = 8, 2


def k_cache(oracle, n_ctx, d, seed):
    """a Q8_0 K cache [n_ctx rows][H_kv heads][d / 32 blocks] from the oracle's quantizer, with one row of -128 / 127 and one block of d = 0"""
    kf = np.random.default_rng(seed).normal(0, 1, (n_ctx * HK, d)).astype(np.float32)
    kb = oracle.quantize_act(Q8_0, kf, ACT_REF).reshape(n_ctx, HK, d // 32, 34).copy()
    kb[3, 0, :, 2:34] = np.tile(np.array([0x80, 0x7F], np.uint8), 16)
    kb[5, 1, 0, 0:2] = 0
    return kb


def attn_inputs(oracle, n_tok, n_kv, d, n_ctx, prompt):
    rng = np.random.default_rng(n_kv * 7 + n_tok)
    q = rng.normal(0, 1, (H, n_tok, d)).astype(np.float32)
    kb = k_cache(oracle, n_ctx, d, n_kv + n_tok)
    vc = rng.normal(0, 1, (HK, d, n_ctx)).astype(np.float16)
    n_pad = (n_tok + 63) // 64 * 64
    mask = np.zeros((n_pad, n_kv), np.float32)
    for t in range(n_tok):
        if prompt:
            mask[t, min(n_kv, n_kv - n_tok + t + 1):] = -np.inf          # token t sees the prefix that ends at its own position
        else:
            mask[t, n_kv - (n_tok - 1 - t) * 3:] = -np.inf              # each token sees a different prefix
    if not prompt:
        mask[:, 5] = -np.inf
    return q, kb, vc, mask, n_pad


def attn_descriptors(q, kb, vc, mask, n_tok, n_kv, d, n_ctx, n_pad):
    from ggml_hexagon_amd import capi
    hb = d // 32 * 34
    dq, dk, dv, dm = dev(q.transpose(1, 0, 2)), dev(kb.reshape(-1)), dev(vc), dev(mask)        # q_cur layout [n_tok, h, d], permuted view below
    out = torch.empty((n_tok, H * d), device="cuda")
    tq = capi.QmmTensor.make(F32, [d, n_tok, H], nb=[4, H * d * 4, d * 4, n_tok * H * d * 4], data=dq.data_ptr())
    tk = q8_tensor(dk, [d, n_kv, HK], nb=[34, HK * hb, hb, n_ctx * HK * hb])                   # llama.cpp's view: heads inside a cache row
    tv = capi.QmmTensor.make(F16, [n_kv, d, HK], nb=[2, n_ctx * 2, n_ctx * d * 2, n_ctx * d * HK * 2], data=dv.data_ptr())
    tm = capi.QmmTensor.make(F32, [n_kv, n_pad], data=dm.data_ptr())
    td = capi.QmmTensor.make(F32, [H * d, n_tok], data=out.data_ptr())
    return (tq, tk, tv, tm, td), out, (dq, dk, dv, dm)


def soft_max_v(s, vg, n_kv):
    """f64 soft-max of the score rows and the product with V, p rounded to f16 as the CPU's F16 vec_dot does"""
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float16).astype(np.float64)
    return p @ vg[:, :n_kv].astype(np.float64).T


KQ8_DECODE_CASES = [(1, 32, 64), (3, 96, 128), (2, 992, 128), (8, 1024, 128), (1, 1056, 64), (2, 4160, 128)]


@pytest.mark.parametrize("act_mode", [ACT_REF, ACT_X86], ids=["ref", "x86"])
@pytest.mark.parametrize("n_tok,n_kv,d", KQ8_DECODE_CASES, ids=["-".join(map(str, c)) for c in KQ8_DECODE_CASES])
def test_attn_decode_on_a_q8_0_k_cache(qmm, oracle, n_tok, n_kv, d, act_mode):
    """KQ -> soft_max(scale, mask) -> KQV -> merged heads, grouped-query, with the scores the CPU path forms for a Q8_0 src0 (q quantized
    to Q8_0 in the act mode, integer dots times d_k * d_q, f32 sums: the oracle's mul_mat), then f64 soft-max and V with p rounded to f16"""
    from ggml_hexagon_amd import capi
    n_ctx = n_kv + 64
    q, kb, vc, mask, n_pad = attn_inputs(oracle, n_tok, n_kv, d, n_ctx, prompt=False)
    ts, out, keep = attn_descriptors(q, kb, vc, mask, n_tok, n_kv, d, n_ctx, n_pad)
    scale = 1.0 / np.sqrt(d)
    r = lambda t: capi.C.byref(t)
    qmm.set_act_mode(act_mode)
    try:
        labels = qmm.trace(lambda: qmm._chk(qmm.lib.qmm_attn_decode(qmm.ctx, *[r(t) for t in ts], scale, qmm._stream())))
        got = out.cpu().numpy().reshape(n_tok, H, d)
    finally:
        qmm.set_act_mode(ACT_REF)
    assert labels == ((f"attn_kq8_decode_kernel<{d}>",) + (("attn_combine_kernel",) if n_kv >= 1024 else ())), labels
    for hh in range(H):
        g = hh // (H // HK)
        s = oracle.mul_mat(Q8_0, kb[:n_kv, g].reshape(n_kv, -1), d, q[hh], act_mode).astype(np.float64) * np.float32(scale) + mask[:n_tok]
        want = soft_max_v(s, vc[g], n_kv)
        err = rel_rms(got[:, hh], want)
        print(f"kq8 decode {n_tok}-{n_kv}-{d} act {act_mode} head {hh}: rel_rms {err:.3g}")
        # the bound of test_attn_decode_one_launch: one flipped f16 rounding of p below 1024 rows; from there on the cache is cut and p stays f32
        assert err < (5e-4 if n_kv < 1024 else 1.5e-3), (hh, n_tok, n_kv)


@pytest.mark.parametrize("n_tok,n_kv,d", [(33, 64, 64), (70, 96, 128), (130, 1056, 128)], ids=["33-64-64", "70-96-128", "130-1056-128"])
def test_attn_prefill_on_a_q8_0_k_cache(qmm, oracle, n_tok, n_kv, d):
    """the prompt form: K unpacked to f16 (k = f16(f32(d) * q)) by one launch, then attn_prefill_kernel; f64 reference with q rounded to f16"""
    from ggml_hexagon_amd import capi
    n_ctx = n_kv + 32
    q, kb, vc, mask, n_pad = attn_inputs(oracle, n_tok, n_kv, d, n_ctx, prompt=True)
    ts, out, keep = attn_descriptors(q, kb, vc, mask, n_tok, n_kv, d, n_ctx, n_pad)
    scale = 1.0 / np.sqrt(d)
    r = lambda t: capi.C.byref(t)
    labels = qmm.trace(lambda: qmm._chk(qmm.lib.qmm_attn_prefill(qmm.ctx, *[r(t) for t in ts], scale, qmm._stream())))
    assert labels == (UNPACK_F16, f"attn_prefill_kernel<{d}>"), labels
    got = out.cpu().numpy().reshape(n_tok, H, d)
    k16 = oracle.dequantize(Q8_0, kb.reshape(n_ctx * HK, -1), d).astype(np.float16).reshape(n_ctx, HK, d)
    qh = q.astype(np.float16).astype(np.float64)
    for hh in range(H):
        g = hh // (H // HK)
        s = qh[hh] @ k16[:n_kv, g].astype(np.float64).T * np.float32(scale) + mask[:n_tok]
        want = soft_max_v(s, vc[g], n_kv)
        err, nrm = rel_rms(got[:, hh], want), np.sqrt(np.mean((got[:, hh] - want) ** 2) / np.mean(want ** 2))
        print(f"kq8 prefill {n_tok}-{n_kv}-{d} head {hh}: rel_rms {err:.3g} nrmse {nrm:.3g}")
        # the two bounds of test_attn_prefill_one_launch
        assert err < (2e-3 if n_kv <= 512 else 6e-3), (hh, n_tok, n_kv)
        assert nrm < (1e-4 if n_kv <= 512 else 4e-4)
