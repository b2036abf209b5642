"""MUL_MAT on BF16 weights (type 30) through qmm_mul_mat / qmm_mul_mat_group / qmm_dequantize: the streaming mat-vec at N <= 8 tokens and
the bf16 MFMA kernel above (csrc/qmm_bf16.hiph, planned by csrc/qmm_bf16_plan.h).

Reference (bf16_refs.py): want = sum_k widen(bf16(x_k)) * widen(w_k) in float64, x rounded to nearest even as ggml_compute_fp32_to_bf16
does.  Bound, for every element: |got - want| <= 2 K 2^-24 absum with absum = sum_k |the products|: bf16 x bf16 products are exact in
f32, so only the K - 1 additions round, and the factor 2 covers truncating adds inside the MFMA.  Derived, not measured; each case
prints its max |err| / rms(want) and its worst |err| / bound beside it.  Values: N(0, 1) x and N(0, 0.02) weights, so that no product or
partial sum is subnormal or overflows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import bf16_refs as B  # noqa: E402
import ggml_hexagon_amd.synth as synth  # noqa: E402
from ggml_hexagon_amd.capi import BF16, PREC_BF16, PREC_F16_Q8, PREC_Q8_EXACT, Q8_0, QmmError  # noqa: E402

N_FEW = (1, 2, 3, 8)
N_PROMPT = (9, 16, 33, 64, 65, 130)
MV_STAGE_BYTES = 128 * 1024        # the plan's budget for staged tokens (test_bf16_host.py pins it through the header)


@pytest.fixture(scope="module")
def qmm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def wdev(bits):
    """uint16 [M, K] -> the uint8 [M, 2 K] device tensor the binding takes"""
    return dev(np.ascontiguousarray(bits).view(np.uint8))


def normal_x(seed, n, k):
    return np.random.default_rng(seed).standard_normal((n, k)).astype(np.float32)


def labels_for(m, k, n):
    """the launches the plan gives this shape, by the design's rules"""
    if n > 8:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        large = m > 64 and n > 64 and ((m + 127) // 128) * ((n + 127) // 128) >= cus
        return ("bf16_mfma_kernel<128>" if large else "bf16_mfma_kernel<64>",)
    at_once = min(n, MV_STAGE_BYTES // (2 * k))
    out, n0 = [], 0
    while n0 < n:
        nt = min(at_once, n - n0)
        out.append(f"bf16_matvec_kernel<{nt},true>")
        n0 += nt
    return tuple(out)


def check(got, want, absum, k, what):
    err = np.abs(got.astype(np.float64) - want)
    lim = B.bound(k, absum)
    rms = max(float(np.sqrt(np.mean(want ** 2))), 1e-300)
    print(f"{what}: max|err|/rms {err.max() / rms:.3e}   worst |err|/bound {float(np.max(err / np.maximum(lim, 1e-300))):.3f}")
    assert np.all(np.isfinite(got)), what
    assert np.all(err <= lim), (what, float(err.max()), float(np.max(err / np.maximum(lim, 1e-300))))


# ----------------------------------------------------------------------------- 1. the shape grid, both kernels, labels per case

SHAPES = [(m, k) for m in (1, 17, 64, 83, 1057) for k in (32, 64, 256, 4128)] + [(64, 14336), (65, 256)]


@pytest.mark.parametrize("m,k", SHAPES, ids=[f"{m}x{k}" for m, k in SHAPES])
def test_shape_grid(qmm, m, k):
    w = synth.synth_weights_bf16(m, k, seed=m + k)
    x = normal_x(k, max(N_PROMPT), k)
    want, absum = B.mul_mat_ref(w, x)                           # once for the longest batch; a shorter batch is its first rows
    wd, xd = wdev(w), dev(x)
    for n in N_FEW + N_PROMPT:
        out = []
        labels = qmm.trace(lambda: out.append(qmm.mul_mat(BF16, wd, k, xd[:n])))
        assert labels == labels_for(m, k, n), (n, labels)
        check(out[0].cpu().numpy(), want[:n], absum[:n], k, f"M={m} K={k} N={n}")


@pytest.mark.parametrize("n,tile", [(1920, 64), (2048, 128)])
def test_large_tiles_where_they_fill_the_chip(qmm, n, tile):
    """the 128 x 128 instance runs only where there are at least as many such tiles as CUs: 2048 rows x 2048 tokens are 256 of them, and
    ragged edges (M = 2011, N - 5) are inside that grid; K = 32 keeps the case small"""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert 240 < cus <= 256, f"shapes chosen for the 256 CUs of an MI355X, this device has {cus}"
    m, k, n = 2011, 32, n - 5
    w, x = synth.synth_weights_bf16(m, k, seed=21), normal_x(21, n, k)
    out = []
    labels = qmm.trace(lambda: out.append(qmm.mul_mat(BF16, wdev(w), k, dev(x))))
    assert labels == (f"bf16_mfma_kernel<{tile}>",), labels
    want, absum = B.mul_mat_ref(w, x)
    check(out[0].cpu().numpy(), want, absum, k, f"M={m} K={k} N={n}")


# ----------------------------------------------------------------------------- 2. the rounding of x, to the bit

@pytest.mark.parametrize("n", [1, 16])
def test_x_is_rounded_to_nearest_even(qmm, n):
    k, m, k0 = 256, 17, 77
    w = np.zeros((m, k), np.uint16)
    w[:, k0] = 0x3F80                                           # 1.0 at k0, zeros elsewhere
    vals = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8)], np.float32)
    wants = np.array([1.0, 1 + 2.0 ** -6, -1.0], np.float32)
    for i, (v, want) in enumerate(zip(vals, wants)):
        x = normal_x(i, n, k)
        x[:, k0] = v
        got = qmm.mul_mat(BF16, wdev(w), k, dev(x)).cpu().numpy()
        assert got.shape == (n, m)
        assert np.array_equal(got, np.full((n, m), want, np.float32)), (float(v), got.ravel()[:4])


@pytest.mark.parametrize("n", [1, 16])
def test_subnormal_x_is_not_flushed(qmm, n):
    """ggml_compute_fp32_to_bf16 keeps subnormals: x = 2^-130 (an f32 subnormal that bf16 holds exactly) against a weight of 2^64 is 2^-66"""
    k, m, k0 = 64, 5, 33
    w = np.zeros((m, k), np.uint16)
    w[:, k0] = B.f32_to_bf16(np.array([2.0 ** 64], np.float32))[0]
    x = np.zeros((n, k), np.float32)
    x[:, k0] = np.float32(2.0 ** -130)
    got = qmm.mul_mat(BF16, wdev(w), k, dev(x)).cpu().numpy()
    assert np.array_equal(got, np.full((n, m), 2.0 ** -66, np.float32)), got.ravel()[:4]


# ----------------------------------------------------------------------------- 3. range: nothing passes through f16

@pytest.mark.parametrize("n", [3, 40])
def test_range_beyond_f16(qmm, n):
    m, k = 64, 256
    rng = np.random.default_rng(5)
    wf = rng.standard_normal((m, k)).astype(np.float32)
    wf[0::2] *= np.float32(2.0 ** 40)
    wf[1::2] *= np.float32(2.0 ** -40)
    w = B.f32_to_bf16(wf)
    x = normal_x(6, n, k)
    got = qmm.mul_mat(BF16, wdev(w), k, dev(x)).cpu().numpy()
    want, absum = B.mul_mat_ref(w, x)
    assert np.all(np.abs(got[:, 0::2]) > 2.0 ** 30) and np.all((np.abs(got[:, 1::2]) < 2.0 ** -30) & (got[:, 1::2] != 0))
    check(got, want, absum, k, f"range N={n}")


# ----------------------------------------------------------------------------- 4. strides and guard columns

@pytest.mark.parametrize("n", [3, 70])
def test_strides_and_guards(qmm, n):
    m, k = 83, 256
    w = synth.synth_weights_bf16(m, k, seed=9)
    wp = np.full((m, 2 * k + 16), 0xA5, np.uint8)               # w_row_bytes = 2 K + 16
    wp[:, :2 * k] = w.view(np.uint8)
    xp = np.full((n, k + 8), 1e30, np.float32)                  # ldx = K + 8
    x = normal_x(n, n, k)
    xp[:, :k] = x
    outp = torch.full((n, m + 16), 7.0, dtype=torch.float32, device="cuda")       # ldd = M + 16
    wd, xd = dev(wp), dev(xp)
    qmm.mul_mat(BF16, wd[:, :2 * k], k, xd[:, :k], out=outp[:, :m])
    res = outp.cpu().numpy()
    assert np.all(res[:, m:] == 7.0)
    want, absum = B.mul_mat_ref(w, x)
    check(res[:, :m], want, absum, k, f"strided N={n}")


# ----------------------------------------------------------------------------- 5. groups

@pytest.mark.parametrize("n", [1, 8, 40])
def test_group_equals_singles_bit_for_bit(qmm, n):
    k, ms = 256, (64, 16, 16)
    ws = [wdev(synth.synth_weights_bf16(m, k, seed=30 + i)) for i, m in enumerate(ms)]
    xd = dev(normal_x(n, n, k))
    singles = [qmm.mul_mat(BF16, w, k, xd).cpu().numpy() for w in ws]
    outs = [torch.zeros((n, m), dtype=torch.float32, device="cuda") for m in ms]
    labels = qmm.trace(lambda: qmm.mul_mat_group([(BF16, w) for w in ws], k, xd, outs))
    assert labels == ((f"bf16_matvec_kernel<{n},true>",) if n <= 8 else ("bf16_mfma_kernel<64>",) * 3), labels
    for o, s in zip(outs, singles):
        assert np.array_equal(o.cpu().numpy(), s)


@pytest.mark.parametrize("n", [2, 40])
def test_mixed_group_runs_type_by_type(qmm, n):
    """BF16 matrices among quantized ones: one launch per same-kind run, each with the bits of its single call"""
    k, m = 256, 48
    wb0, wb1 = (wdev(synth.synth_weights_bf16(m, k, seed=40 + i)) for i in range(2))
    wq = dev(synth.synth_weights(Q8_0, m, k, seed=42))
    xd = dev(normal_x(n, n, k))
    group = [(BF16, wb0), (Q8_0, wq), (BF16, wb1)]
    singles = [qmm.mul_mat(t, w, k, xd).cpu().numpy() for t, w in group]
    outs = [torch.zeros((n, m), dtype=torch.float32, device="cuda") for _ in group]
    labels = qmm.trace(lambda: qmm.mul_mat_group(group, k, xd, outs))
    bf = f"bf16_matvec_kernel<{n},true>" if n <= 8 else "bf16_mfma_kernel<64>"
    assert labels[0] == bf and labels[-1] == bf and len(labels) >= 3 and not any(l.startswith("bf16") for l in labels[1:-1]), labels
    for o, s in zip(outs, singles):
        assert np.array_equal(o.cpu().numpy(), s)


def test_one_token_group_inside_a_chain_recording_launches_directly(qmm):
    k, m = 256, 64
    w = wdev(synth.synth_weights_bf16(m, k, seed=50))
    xd = dev(normal_x(50, 1, k))
    plain = qmm.mul_mat(BF16, w, k, xd).cpu().numpy()
    before = qmm.chain_stats()
    out = torch.zeros((1, m), dtype=torch.float32, device="cuda")
    qmm.chain_begin()
    try:
        labels = qmm.trace(lambda: qmm.mul_mat_group([(BF16, w)], k, xd, [out]))
    finally:
        qmm.chain_end()
    assert labels == ("bf16_matvec_kernel<1,true>",) and qmm.chain_stats() == before
    assert np.array_equal(out.cpu().numpy(), plain)


# ----------------------------------------------------------------------------- 6. modes do not matter, and the same call gives the same bits

@pytest.mark.parametrize("n", [3, 40])
def test_precision_and_act_modes_do_not_matter(qmm, n):
    m, k = 83, 256
    w, xd = wdev(synth.synth_weights_bf16(m, k, seed=60)), dev(normal_x(60, n, k))
    res = []
    try:
        for prec in (PREC_BF16, PREC_F16_Q8, PREC_Q8_EXACT):
            for act in (0, 1):
                qmm.set_precision(prec)
                qmm.set_act_mode(act)
                res.append(qmm.mul_mat(BF16, w, k, xd).cpu().numpy())
    finally:
        qmm.set_precision(PREC_F16_Q8)
        qmm.set_act_mode(0)
    for r in res[1:]:
        assert np.array_equal(r, res[0])


@pytest.mark.parametrize("n", [3, 130])
def test_same_call_same_bits(qmm, n):
    m, k = 1057, 4128
    w, xd = wdev(synth.synth_weights_bf16(m, k, seed=70)), dev(normal_x(70, n, k))
    a = qmm.mul_mat(BF16, w, k, xd).cpu().numpy()
    b = qmm.mul_mat(BF16, w, k, xd).cpu().numpy()
    assert np.array_equal(a, b)


# ----------------------------------------------------------------------------- 7. refusals: an error with a message, and the context still computes

def test_refusals_leave_the_context_working(qmm):
    k, m = 64, 4
    w = synth.synth_weights_bf16(m, k, seed=80)
    x = normal_x(80, 2, k)
    want, absum = B.mul_mat_ref(w, x)

    def still_computes():
        check(qmm.mul_mat(BF16, wdev(w), k, dev(x)).cpu().numpy(), want, absum, k, "after a refusal")

    with pytest.raises(QmmError, match="multiple of 32"):      # K = 48
        qmm.mul_mat(BF16, dev(np.zeros((m, 96), np.uint8)), 48, dev(np.zeros((2, 48), np.float32)))
    still_computes()
    with pytest.raises(QmmError, match="16-byte"):              # a row stride off 16 bytes
        qmm.mul_mat(BF16, dev(np.zeros((m, 2 * k + 8), np.uint8))[:, :2 * k], k, dev(x))
    still_computes()
    out = torch.zeros((2, m), dtype=torch.float32, device="cuda")
    res = torch.zeros((2, m), dtype=torch.float32, device="cuda")
    with pytest.raises(QmmError, match="BF16"):                 # extras with a BF16 matrix
        qmm.mul_mat_group_ex([(BF16, wdev(w))], k, dev(x), [out], residuals=[res])
    with pytest.raises(QmmError, match="BF16"):
        qmm.mul_mat_group_ex([(BF16, wdev(w))], k, dev(x), [out], norm_w=dev(np.ones(k, np.float32)), eps=1e-5)
    xl = dev(normal_x(81, 16, k))
    outl = torch.zeros((16, m), dtype=torch.float32, device="cuda")
    with pytest.raises(QmmError, match="BF16"):                 # ... and at a prompt batch
        qmm.mul_mat_group_ex([(BF16, wdev(w))], k, xl, [outl], norm_w=dev(np.ones(k, np.float32)), eps=1e-5)
    still_computes()
    ids = dev(np.zeros((2, 1), np.int32))
    with pytest.raises(QmmError, match="type 30"):              # MUL_MAT_ID stays out of scope
        qmm.mul_mat_id(BF16, wdev(w).reshape(1, m, 2 * k), k, dev(x.reshape(2, 1, k)), ids)
    still_computes()


# ----------------------------------------------------------------------------- 8. qmm_dequantize(30, ...)

def test_dequantize_is_the_exact_widening(qmm):
    m, k = 83, 4128
    w = synth.synth_weights_bf16(m, k, seed=90)
    w[0, :4] = (0x0040, 0x8000, 0x7F7F, 0xFF80)                 # a subnormal, -0.0, the largest finite value, -inf
    got = qmm.dequantize(BF16, wdev(w), k).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), B.bf16_to_f32(w).view(np.uint32))
