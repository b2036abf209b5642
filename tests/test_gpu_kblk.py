"""GPU parity of a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 in the kernel library (csrc/qmm_kblk.hiph, planned by csrc/qmm_kblk_plan.h): CPY f32 ->
type byte for byte against the reference's quantize_row_*_ref bytes pinned in tests/golden/kblk_quantize.npz, CPY type -> f32 / f16 against
the oracle's dequantizer, and the two attention entry points with k in the type against f64 numpy on the CPU's own arithmetic (few tokens:
the oracle's scores for such a src0 against Q8_0 / Q8_1 activations; prompt: K as f16(dequantize)), at the bounds of the Q8_0 K cache's
tests (tests/test_gpu_kcache_q8.py): nothing new is rounded."""
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

sys.path.insert(0, str(Path(__file__).resolve().parent))

import kblk_refs as R  # noqa: E402
from oracle.pyoracle import ACT_REF, ACT_X86  # noqa: E402

F32, F16 = 0, 1
TYPE_IDS = [R.NAMES[t] for t in R.TYPES]


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


@pytest.fixture(scope="module")
def golden():
    return R.load_golden()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def kb_tensor(t, buf, ne, nb=None):
    return R.kblk_tensor(t, ne, nb, data=buf.data_ptr())


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


# ---- CPY

@pytest.mark.parametrize("shape", ["64x3", "128x5x2-permuted"])
@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_cpy_f32_to_the_type_is_the_reference_quantizer(qmm, golden, t, shape):
    from ggml_hexagon_amd import capi
    name = R.NAMES[t]
    if shape == "64x3":
        src = dev(golden["a"])
        ts = capi.QmmTensor.make(F32, [64, 3], data=src.data_ptr())
        want, ne_d = golden[f"a_{name}"].reshape(-1), [64, 3]
    else:
        src = dev(golden["b"])                                            # memory [128, 2, 5]; read as [128, 5, 2] through permute(0, 2, 1, 3)
        ts = capi.QmmTensor.make(F32, [128, 5, 2], nb=[4, 1024, 512, 5120], data=src.data_ptr())
        want = golden[f"b_{name}"].reshape(5, 2, -1).transpose(1, 0, 2).reshape(-1)          # src's index order: i1 (the 5) inside i2 (the 2)
        ne_d = [1280]                                                     # element i of src is element i of dst: any contiguous shape
    for act_mode in (ACT_REF, ACT_X86):                                   # from_float of these types knows no act mode
        out = torch.full((want.size + 34,), 0xA5, dtype=torch.uint8, device="cuda")
        qmm.set_act_mode(act_mode)
        try:
            labels = qmm.trace(lambda: qmm.op(capi.OP_CPY, kb_tensor(t, out, ne_d), ts))
            got = out.cpu().numpy()
        finally:
            qmm.set_act_mode(ACT_REF)
        assert labels == (f"cpy_{name}_quantize_kernel",), labels
        bad = np.flatnonzero(got[:want.size] != want)
        assert bad.size == 0, (bad[:8], bad[:8] // R.BLOCK[t], bad[:8] % R.BLOCK[t])
        assert (got[want.size:] == 0xA5).all()                            # nothing behind the last block


def source_blocks(t, golden, n_rows, k):
    """rows of blocks from the golden file with, written over them, one block of extreme codes (nibbles 0 and 15 alternating, qh all ones) and
    one block with d = 0"""
    blocks = golden[f"b_{R.NAMES[t]}"].reshape(-1, R.BLOCK[t])[:n_rows * k // 32].reshape(n_rows, k // 32, R.BLOCK[t]).copy()
    blocks[1, 0, R.qs_off(t):] = np.tile(np.array([0xF0, 0x0F], np.uint8), 8)
    if R.HAS_QH[t]:
        blocks[1, 0, R.qh_off(t):R.qh_off(t) + 4] = 0xFF
    blocks[2, 1, 0:2] = 0
    return blocks


@pytest.mark.parametrize("dst_type", [F32, F16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", ["128x6", "64x4x3-permuted"])
@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_cpy_the_type_to_float_is_the_cpu_dequantizer(qmm, oracle, golden, t, shape, dst_type):
    from ggml_hexagon_amd import capi
    B, name = R.BLOCK[t], R.NAMES[t]
    k, n_rows = (128, 6) if shape == "128x6" else (64, 12)
    blocks = source_blocks(t, golden, n_rows, k)
    src = dev(blocks.reshape(-1))
    if shape == "128x6":
        ts, rows = kb_tensor(t, src, [128, 6]), blocks
    else:                                                                # memory [64, 4, 3] (rows of 2 blocks), read as [64, 3, 4]
        ts = kb_tensor(t, src, [64, 3, 4], nb=[B, 8 * B, 2 * B, 24 * B])
        rows = blocks.reshape(3, 4, 2, B).transpose(1, 0, 2, 3).reshape(12, 2, B)
    want = oracle.dequantize(t, rows.reshape(n_rows, -1), k).reshape(-1)
    assert np.array_equal(want, R.dequantize(t, rows.reshape(n_rows, -1), k).reshape(-1))
    hi = 31 if R.HAS_QH[t] else 15
    assert (R.codes(t, rows) == hi).any() and (R.codes(t, rows) == 0).any()
    want = want if dst_type == F32 else want.astype(np.float16)           # the f16 form: one more rounding
    out = torch.zeros(want.size + 8, dtype=torch.float32 if dst_type == F32 else torch.float16, device="cuda")
    td = capi.QmmTensor.make(dst_type, [k, n_rows], data=out.data_ptr())
    labels = qmm.trace(lambda: qmm.op(capi.OP_CPY, td, ts))
    assert labels == (f"cpy_{name}_unpack_kernel<{'f32' if dst_type == F32 else 'f16'}>",), labels
    got = out.cpu().numpy()
    assert np.array_equal(got[:want.size], want), np.flatnonzero(got[:want.size] != want)[:8]
    assert (got[want.size:] == 0).all()
    # ... and with a destination off 16 bytes by one element (the scalar stores)
    es = 4 if dst_type == F32 else 2
    td2 = capi.QmmTensor.make(dst_type, [k, n_rows], data=out.data_ptr() + es)
    out.zero_()
    qmm.op(capi.OP_CPY, td2, ts)
    got = out.cpu().numpy()
    assert got[0] == 0 and np.array_equal(got[1:want.size + 1], want) and (got[want.size + 1:] == 0).all()


# ---- attention

H, HK = 8, 2


def k_cache(t, n_ctx, d, seed):
    """a K cache [n_ctx rows][H_kv heads][d / 32 blocks] of block type t from the restated quantizer (pinned to the reference by the golden
    file), with one row of extreme codes (nibbles 0 and 15, qh all ones) and one block of d = 0; the rows beyond n_kv are finite garbage.
    The extreme row's scales are set so that its values stay within [-1, 1] like its neighbours' (d = 1 / 8 for the 4-bit codes, 1 / 16
    with qh, m = -1): at the scale of a quantized N(0, 1) row every value would sit at full range, the row would hold most of the soft-max
    weight of the tokens that see it, and max |err| / rms per head would then measure the f16 rounding of one large p in the reference
    (which the cut-cache kernels, keeping p in f32, do not make) against the small rows of the other tokens, not the scores"""
    kf = np.random.default_rng(seed).normal(0, 1, (n_ctx * HK, d)).astype(np.float32)
    kb = R.quantize(t, kf).reshape(n_ctx, HK, d // 32, R.BLOCK[t]).copy()
    kb[3, 0, :, R.qs_off(t):] = np.tile(np.array([0xF0, 0x0F], np.uint8), 8)
    kb[3, 0, :, 0:2] = np.array([0.0625 if R.HAS_QH[t] else 0.125], np.float16).view(np.uint8)
    if R.HAS_M[t]:
        kb[3, 0, :, 2:4] = np.array([-1.0], np.float16).view(np.uint8)
    if R.HAS_QH[t]:
        kb[3, 0, :, R.qh_off(t):R.qh_off(t) + 4] = 0xFF
    kb[5, 1, 0, 0:2] = 0
    return kb


def attn_inputs(t, n_tok, n_kv, d, n_ctx, prompt):
    rng = np.random.default_rng(n_kv * 7 + n_tok + 1000 * t)
    q = rng.normal(0, 1, (H, n_tok, d)).astype(np.float32)
    kb = k_cache(t, n_ctx, d, n_kv + n_tok + t)
    vc = rng.normal(0, 1, (HK, d, n_ctx)).astype(np.float16)
    n_pad = (n_tok + 63) // 64 * 64
    mask = np.zeros((n_pad, n_kv), np.float32)
    for i in range(n_tok):
        if prompt:
            mask[i, min(n_kv, n_kv - n_tok + i + 1):] = -np.inf          # token i sees the prefix that ends at its own position
        else:
            mask[i, n_kv - (n_tok - 1 - i) * 3:] = -np.inf              # each token sees a different prefix
    if not prompt:
        mask[:, 7] = -np.inf
    return q, kb, vc, mask, n_pad


def attn_descriptors(t, q, kb, vc, mask, n_tok, n_kv, d, n_ctx, n_pad):
    from ggml_hexagon_amd import capi
    hb = d // 32 * R.BLOCK[t]
    dq, dk, dv, dm = dev(q.transpose(1, 0, 2)), dev(kb.reshape(-1)), dev(vc), dev(mask)        # q_cur layout [n_tok, h, d], permuted view below
    out = torch.empty((n_tok, H * d), device="cuda")
    tq = capi.QmmTensor.make(F32, [d, n_tok, H], nb=[4, H * d * 4, d * 4, n_tok * H * d * 4], data=dq.data_ptr())
    tk = kb_tensor(t, dk, [d, n_kv, HK], nb=[R.BLOCK[t], HK * hb, hb, n_ctx * HK * hb])        # llama.cpp's view: heads inside a cache row
    tv = capi.QmmTensor.make(F16, [n_kv, d, HK], nb=[2, n_ctx * 2, n_ctx * d * 2, n_ctx * d * HK * 2], data=dv.data_ptr())
    tm = capi.QmmTensor.make(F32, [n_kv, n_pad], data=dm.data_ptr())
    td = capi.QmmTensor.make(F32, [H * d, n_tok], data=out.data_ptr())
    return (tq, tk, tv, tm, td), out, (dq, dk, dv, dm)


def soft_max_v(s, vg, n_kv):
    """f64 soft-max of the score rows and the product with V, p rounded to f16 as the CPU's F16 vec_dot does"""
    p = np.exp(s - s.max(axis=1, keepdims=True))
    p = (p / p.sum(axis=1, keepdims=True)).astype(np.float32).astype(np.float16).astype(np.float64)
    return p @ vg[:, :n_kv].astype(np.float64).T


DECODE_CASES = [(1, 32, 64), (3, 96, 128), (2, 992, 128), (8, 1024, 128), (1, 1056, 64)]


@pytest.mark.parametrize("act_mode", [ACT_REF, ACT_X86], ids=["ref", "x86"])
@pytest.mark.parametrize("n_tok,n_kv,d", DECODE_CASES, ids=["-".join(map(str, c)) for c in DECODE_CASES])
@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_attn_decode_on_a_k_cache_of_the_type(qmm, oracle, t, n_tok, n_kv, d, act_mode):
    """KQ -> soft_max(scale, mask) -> KQV -> merged heads, grouped-query, with the scores the CPU path forms for such a src0 (q quantized to
    Q8_0 or Q8_1 in the act mode, integer dots, the float part of ggml_vec_dot_<t>_q8_x, f32 sums: the oracle's mul_mat), then f64 soft-max
    and V with p rounded to f16.  Measured on the MI355X (max |err| / rms per head, worst of the four types and both act modes): see
    profiles/kblk_attn_times.txt"""
    from ggml_hexagon_amd import capi
    n_ctx = n_kv + 64
    q, kb, vc, mask, n_pad = attn_inputs(t, n_tok, n_kv, d, n_ctx, prompt=False)
    ts, out, keep = attn_descriptors(t, q, kb, vc, mask, n_tok, n_kv, d, n_ctx, n_pad)
    scale = 1.0 / np.sqrt(d)
    r = lambda x: capi.C.byref(x)
    qmm.set_act_mode(act_mode)
    try:
        labels = qmm.trace(lambda: qmm._chk(qmm.lib.qmm_attn_decode(qmm.ctx, *[r(x) for x in ts], scale, qmm._stream())))
        got = out.cpu().numpy().reshape(n_tok, H, d)
    finally:
        qmm.set_act_mode(ACT_REF)
    assert labels == ((f"attn_kblk_decode_kernel<{R.NAMES[t]},{d}>",) + (("attn_combine_kernel",) if n_kv >= 1024 else ())), labels
    for hh in range(H):
        g = hh // (H // HK)
        s = oracle.mul_mat(t, kb[:n_kv, g].reshape(n_kv, -1), d, q[hh], act_mode).astype(np.float64) * np.float32(scale) + mask[:n_tok]
        want = soft_max_v(s, vc[g], n_kv)
        err = rel_rms(got[:, hh], want)
        print(f"{R.NAMES[t]} decode {n_tok}-{n_kv}-{d} act {act_mode} head {hh}: rel_rms {err:.3g}")
        # the bound of test_attn_decode_on_a_q8_0_k_cache: one flipped f16 rounding of p below 1024 rows; from there on the cache is cut and p stays f32
        assert err < (5e-4 if n_kv < 1024 else 1.5e-3), (hh, n_tok, n_kv)


@pytest.mark.parametrize("n_tok,n_kv,d", [(33, 64, 64), (70, 96, 128), (130, 1056, 128)], ids=["33-64-64", "70-96-128", "130-1056-128"])
@pytest.mark.parametrize("t", R.TYPES, ids=TYPE_IDS)
def test_attn_prefill_on_a_k_cache_of_the_type(qmm, oracle, t, n_tok, n_kv, d):
    """the prompt form: K unpacked to f16 (k = f16(dequantize)) by one launch, then attn_prefill_kernel; f64 reference with q rounded to f16"""
    from ggml_hexagon_amd import capi
    n_ctx = n_kv + 32
    q, kb, vc, mask, n_pad = attn_inputs(t, n_tok, n_kv, d, n_ctx, prompt=True)
    ts, out, keep = attn_descriptors(t, q, kb, vc, mask, n_tok, n_kv, d, n_ctx, n_pad)
    scale = 1.0 / np.sqrt(d)
    r = lambda x: capi.C.byref(x)
    labels = qmm.trace(lambda: qmm._chk(qmm.lib.qmm_attn_prefill(qmm.ctx, *[r(x) for x in ts], scale, qmm._stream())))
    assert labels == (f"cpy_{R.NAMES[t]}_unpack_kernel<f16>", f"attn_prefill_kernel<{d}>"), labels
    got = out.cpu().numpy().reshape(n_tok, H, d)
    k16 = oracle.dequantize(t, kb.reshape(n_ctx * HK, -1), d).astype(np.float16).reshape(n_ctx, HK, d)
    qh = q.astype(np.float16).astype(np.float64)
    for hh in range(H):
        g = hh // (H // HK)
        s = qh[hh] @ k16[:n_kv, g].astype(np.float64).T * np.float32(scale) + mask[:n_tok]
        want = soft_max_v(s, vc[g], n_kv)
        err, nrm = rel_rms(got[:, hh], want), np.sqrt(np.mean((got[:, hh] - want) ** 2) / np.mean(want ** 2))
        print(f"{R.NAMES[t]} prefill {n_tok}-{n_kv}-{d} head {hh}: rel_rms {err:.3g} nrmse {nrm:.3g}")
        # the two bounds of test_attn_prefill_on_a_q8_0_k_cache
        assert err < (2e-3 if n_kv <= 512 else 6e-3), (hh, n_tok, n_kv)
        assert nrm < (1e-4 if n_kv <= 512 else 4e-4)
