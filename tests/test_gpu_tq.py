"""TQ1_0 / TQ2_0 on the device, through the C-ABI.  Expected values are the live reference's dequantizer (bit for bit) and the numpy
restatement of its scalar dot products (tests/tq_refs.py) on the reference's own Q8_K activations.

Bars (tests/test_gpu_iq1.py:24): mat-vec max |err| / rms <= 2e-5; prompt batches rel-L2 <= 1e-3 in the f16 mode, NMSE <= 5e-4 under
QMM_PREC_BF16 against the f32 product.  The fused SwiGLU form is held to ``swiglu_bar`` of tests/test_gpu_iq1.py.  The group entry
with the norm in front is compared with the numpy-normed rows at 5e-5, the bar of that entry in tests/test_gpu_layer_ops.py:78 (the
kernel's norm and numpy's differ in the last bit here and there; such a row quantizes one activation one step apart).  Every measured
value is printed.

A weight matrix is quantizer-made rows, then the crafted blocks of tq_refs.edge_rows (every byte value in every position class, d = 0
and subnormal, both signs; without the +-65504 blocks where a product is compared), then random bytes with bounded d."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import tq_refs as R  # noqa: E402

TYPES = [R.TQ1_0, R.TQ2_0]
IDS = [R.NAMES[t] for t in TYPES]
IQ2_XXS = 16
MV_BAR, F16_BAR, BF16_BAR = 2e-5, 1e-3, 5e-4
NORM_BAR = 5e-5
QROWS = 8


@pytest.fixture(scope="module")
def ref():
    return R.TqRef()


@pytest.fixture(scope="module")
def qmm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # (a copy: the cached cases are read-only)


def rms(a):
    return max(float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))), 1e-30)


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / rms(want))


def rel_l2(got, want):
    want = want.astype(np.float64)
    return float(np.sqrt(np.sum((got - want) ** 2) / max(np.sum(want ** 2), 1e-30)))


def nmse(got, want):
    return rel_l2(got, want) ** 2


_cache = {}


def weights(ref, t, m, k, seed):
    """[m, row]: QROWS quantizer rows, the crafted rows (|d| <= 2^-4), random bytes behind them; cut to m"""
    from ggml_hexagon_amd import synth
    rng = np.random.default_rng(77 * t + k)
    made = ref.quantize(t, rng.uniform(-1, 1, (QROWS, k)).astype(np.float32))
    w = np.concatenate([made, R.edge_rows(t, k, big=False, seed=seed), synth.synth_weights(t, m, k, seed=seed, sigma=0.02)])[:m]
    return np.ascontiguousarray(w)


def case(ref, t, m, k, n):
    """weights [m, row], activations x [n, k] and the expected product [n, m]; computed once per shape"""
    key = (t, m, k, n)
    if key not in _cache:
        rng = np.random.default_rng(1000 * t + m + k)
        w = weights(ref, t, m, k, seed=1000 * t + m + k)
        x = rng.uniform(-1, 1, (n, k)).astype(np.float32)
        want = R.mul_mat_np(t, w, k, ref.quantize_act(x))
        for a in (w, x, want):
            a.setflags(write=False)
        _cache[key] = (w, x, want)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ dequantize, GET_ROWS

@pytest.mark.parametrize("k", [256, 512, 768, 4096])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_dequantize_bit_exact(qmm, ref, t, k):
    rng = np.random.default_rng(k + t)
    made = ref.quantize(t, rng.uniform(-1, 1, (5, k)).astype(np.float32))
    edge = R.edge_rows(t, k)
    R.assert_edges(t, edge, k)
    for name, rows in (("quantizer", made), ("crafted", edge)):
        got = qmm.dequantize(t, dev(rows), k).cpu().numpy()
        want = ref.dequantize(t, rows, k)
        same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
        print(f"tq | dequantize {R.NAMES[t]} K={k} {name} rows {rows.shape[0]} | bit-exact {same}")
        assert same
        assert np.array_equal(R.dequantize_np(t, rows, k).view(np.uint32), want.view(np.uint32))


def get_rows_call(q, t, wd, k, idv):
    """QMM_OP_GET_ROWS of rows idv out of wd [rows, row_size]: returns (call, dst tensor [len(idv), k])"""
    from ggml_hexagon_amd.capi import OP_GET_ROWS, QmmTensor
    ids = torch.tensor(idv, dtype=torch.int32, device="cuda")
    dst = torch.full((len(idv), k), -7.0, dtype=torch.float32, device="cuda")
    ta = QmmTensor.make(t, [k, wd.shape[0]], nb=[1, wd.stride(0), wd.stride(0) * wd.shape[0], wd.stride(0) * wd.shape[0]], data=wd.data_ptr())
    ti = QmmTensor.make(26, [len(idv)], data=ids.data_ptr())
    td = QmmTensor.make(0, [k, len(idv)], data=dst.data_ptr())
    keep = (ids, wd)
    return (lambda: q.op(OP_GET_ROWS, td, ta, ti)), dst, keep


@pytest.mark.parametrize("k", [256, 768])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_get_rows_bit_exact(qmm, ref, t, k):
    w = R.edge_rows(t, k)                                           # the crafted blocks, +-65504 included
    last = w.shape[0] - 1
    for idv in ([3, last, 0, 3, 5, 1], list(range(last, -1, -1))):  # permuted with a repeated index and the last row; reversed
        call, dst, keep = get_rows_call(qmm, t, dev(w), k, idv)
        labels = qmm.trace(call)
        qmm.synchronize()
        want = ref.dequantize(t, w[idv], k)
        same = np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
        print(f"tq | get_rows {R.NAMES[t]} K={k} rows {len(idv)} | {labels} | bit-exact {same}")
        assert labels == (f"get_rows_q_kernel<{t}>",) and same


# ------------------------------------------------------------------------------------------------ refusals

def test_refusals_leave_the_context_computing(qmm, ref):
    from ggml_hexagon_amd.capi import QmmError
    for t in TYPES:
        assert qmm.row_size(t, 256) == R.BLOCK_BYTES[t] and qmm.row_size(t, 4096) == 16 * R.BLOCK_BYTES[t] and qmm.row_size(t, 4000) == 0
        assert qmm.q8_exact_supported(t, 4096) == 0 and qmm.planar_type(t, 4096, R.row_size(t, 4096)) == 0
        w, x, want = case(ref, t, 16, 256, 2)
        out = torch.full((2, 16), 123.0, dtype=torch.float32, device="cuda")
        wide = torch.zeros((16, 16 * R.BLOCK_BYTES[t]), dtype=torch.uint8, device="cuda")
        x4000 = torch.zeros((2, 4000), dtype=torch.float32, device="cuda")
        with pytest.raises(QmmError):                              # K = 4000 is no multiple of the block
            qmm.mul_mat(t, wide, 4000, x4000, out=out)
        print(f"tq | {R.NAMES[t]} K=4000 refused: {qmm.lib.qmm_last_error().decode()}")
        with pytest.raises(QmmError):
            qmm.dequantize(t, wide, 4000)
        with pytest.raises(QmmError):                              # a codebook for a type that has none
            qmm.set_codebook(t, np.zeros(4096, np.uint32))
        qmm.synchronize()
        assert bool((out == 123.0).all())
        got = qmm.mul_mat(t, dev(w), 256, dev(x)).cpu().numpy()    # the context still computes
        assert rel_rms(got, want) <= MV_BAR
    assert qmm.row_size(IQ2_XXS, 4096) == 0                        # IQ2_XXS is still no type of this library
    w16 = torch.zeros((16, 16 * 66), dtype=torch.uint8, device="cuda")
    x16 = torch.zeros((2, 4096), dtype=torch.float32, device="cuda")
    with pytest.raises(QmmError):
        qmm.mul_mat(IQ2_XXS, w16, 4096, x16)
    print(f"tq | type 16 refused: {qmm.lib.qmm_last_error().decode()}")
    t = R.TQ2_0
    w, x, want = case(ref, t, 16, 256, 2)
    assert rel_rms(qmm.mul_mat(t, dev(w), 256, dev(x)).cpu().numpy(), want) <= MV_BAR


# ------------------------------------------------------------------------------------------------ mat-vec

# one block (most lanes idle); the activation swizzle flips on bit 8 of k; an odd block count; more units than a wave.  M: fewer rows
# than a wave takes, a ragged count, more than the 64-row tile
MV_SHAPES = [(5, 256), (16, 512), (70, 768), (16, 4096)]


@pytest.mark.parametrize("m,k", MV_SHAPES)
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_matvec(qmm, ref, t, m, k):
    w, x, want = case(ref, t, m, k, 8)
    wd = dev(w)
    for n in range(1, 9):
        xd = dev(x[:n])
        labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd))
        got = qmm.mul_mat(t, wd, k, xd).cpu().numpy()
        err = rel_rms(got, want[:n])
        print(f"tq | matvec {R.NAMES[t]} M={m} K={k} N={n} | {labels} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert labels == (f"matvec_kernel<{t},{n},false>",)
        assert err <= MV_BAR
    live = ref.mul_mat(t, w[:4], k, x[:2])                         # the live reference's own (SIMD) dot on a corner of the case
    err = rel_rms(want[:2, :4], live)
    print(f"tq | matvec {R.NAMES[t]} M={m} K={k} | numpy restatement against the live dot, corner: max|err|/rms {err:.3e}")
    assert err <= MV_BAR


@pytest.mark.parametrize("n", [1, 8, 70])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_strides_and_guard_columns(qmm, ref, t, n):
    """w_row_bytes and ldd larger than the row and M: the padding is neither read as weights nor written.  The blocks stay on 2-byte
    boundaries (6 spare bytes), all the formats ask for"""
    m, k, pad = 33, 768, 6
    w, x, want = case(ref, t, m, k, 70)
    row = w.shape[1]
    wp = np.full((m, row + pad), 0xa5, np.uint8)
    wp[:, :row] = w
    wd = dev(wp)[:, :row]
    assert wd.stride(0) == row + pad
    xd = dev(x[:n])
    big = torch.full((n, m + 16), 123.0, dtype=torch.float32, device="cuda")
    labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd, out=big[:, :m]))
    qmm.synchronize()
    got = big.cpu().numpy()
    plain = qmm.mul_mat(t, dev(w), k, xd).cpu().numpy()
    err = rel_rms(got[:, :m], want[:n]) if n <= 8 else rel_l2(got[:, :m], want[:n])
    bar = MV_BAR if n <= 8 else F16_BAR
    print(f"tq | strides {R.NAMES[t]} M={m} K={k} N={n} row {row}+{pad} ldd {m}+16 | {labels} | {'max|err|/rms' if n <= 8 else 'rel-L2'} {err:.3e} (bar {bar})")
    assert np.all(got[:, m:] == 123.0)
    assert err <= bar
    assert np.array_equal(got[:, :m].view(np.uint32), plain.view(np.uint32))


# ------------------------------------------------------------------------------------------------ groups

def rms_norm(x, w, eps):
    x64 = x.astype(np.float64)
    return (x * (1.0 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + eps)).astype(np.float32) * w).astype(np.float32)


@pytest.mark.parametrize("n", [1, 5, 8])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_qkv_group_plain_and_with_norm_and_residual(qmm, ref, t, n):
    """attn_q / attn_k / attn_v of one type, as a stock dense TQ file lays a layer out: the plain group launch bit-equal to the single
    calls; with the norm staged in front and a residual behind, against the numpy-normed rows"""
    k = 1024
    ws_np = [case(ref, t, m, k, 8)[0] for m in (96, 33, 40)]
    x = case(ref, t, 96, k, 8)[1][:n]
    members = [(t, dev(w)) for w in ws_np]
    xd = dev(x)
    outs = [torch.full((n, w.shape[0] + 4), -3.0, dtype=torch.float32, device="cuda")[:, :w.shape[0]] for w in ws_np]
    labels = qmm.trace(lambda: qmm.mul_mat_group(members, k, xd, outs))
    qmm.synchronize()
    assert labels and set(labels) == {f"matvec_kernel<{t},{n},false>"}, labels
    for (tt, wd), o in zip(members, outs):
        assert torch.equal(o.contiguous().view(torch.int32), qmm.mul_mat(tt, wd, k, xd).view(torch.int32))
    print(f"tq | group 3 x {R.NAMES[t]} N={n} | {labels} | bit-equal to the single calls")
    rng = np.random.default_rng(5 + n)
    nw = rng.normal(1, 0.1, k).astype(np.float32)
    res = [rng.normal(0, 1, (n, w.shape[0])).astype(np.float32) for w in ws_np]
    acts = ref.quantize_act(rms_norm(x, nw, 1e-5))
    fused = [torch.zeros((n, w.shape[0]), device="cuda") for w in ws_np]
    labels = qmm.trace(lambda: qmm.mul_mat_group_ex(members, k, xd, fused, norm_w=dev(nw), eps=1e-5, residuals=[dev(r) for r in res]))
    qmm.synchronize()
    for w, o, r in zip(ws_np, fused, res):
        want = R.mul_mat_np(t, w, k, acts)
        err = float(np.max(np.abs(o.cpu().numpy() - r - want.astype(np.float64))) / rms(want))
        print(f"tq | group norm + residual {R.NAMES[t]} M={w.shape[0]} N={n} | {labels} | max|err|/rms {err:.3e} (bar {NORM_BAR})")
        assert err <= NORM_BAR


@pytest.mark.parametrize("n", [1, 4])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_gate_up_swiglu_group(qmm, ref, t, n):
    """ffn_gate / ffn_up as one few-token launch with SwiGLU fused: held to swiglu_bar"""
    from test_gpu_iq1 import swiglu_bar
    k, m = 1024, 96
    wg, x, want_g = case(ref, t, m, k, 8)
    wu = np.ascontiguousarray(wg[::-1])
    want_u = want_g[:, ::-1]
    outs = [torch.full((n, m), 7.0, device="cuda"), torch.full((n, m), 7.0, device="cuda")]
    labels = qmm.trace(lambda: qmm.mul_mat_group_ex([(t, dev(wg)), (t, dev(wu))], k, dev(x[:n]), outs, swiglu=1))
    qmm.synchronize()
    g, u = want_g[:n].astype(np.float64), want_u[:n].astype(np.float64)
    err, bar = float(np.abs(outs[0].cpu().numpy() - g / (1.0 + np.exp(-g)) * u).max()), swiglu_bar(g, u)
    print(f"tq | group swiglu {R.NAMES[t]} N={n} | {labels} | max|err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar
    assert bool((outs[1] == 7.0).all())


# ------------------------------------------------------------------------------------------------ prompt batches

@pytest.mark.parametrize("m,k", [(5, 256), (70, 512), (16, 768), (70, 4096)])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_prompt(qmm, ref, t, m, k):
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8
    w, x, want = case(ref, t, m, k, 70)
    wd = dev(w)
    deq = ref.dequantize(t, w, k).astype(np.float64)
    try:
        for n in (9, 12, 33, 70):
            xd = dev(x[:n])
            f32_want = x[:n].astype(np.float64) @ deq.T            # what QMM_PREC_BF16 approximates: no Q8 step
            for prec, name in ((PREC_F16_Q8, "f16"), (PREC_BF16, "bf16")):
                qmm.set_precision(prec)
                big = torch.full((n, m + 16), 123.0, dtype=torch.float32, device="cuda")
                labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd, out=big[:, :m]))
                qmm.synchronize()
                run = big.cpu().numpy()
                assert labels[-1] == f"mfma_kernel<{t},64>", labels
                assert np.all(run[:, m:] == 123.0)                 # guard columns of ldd = M + 16
                got = run[:, :m]
                if prec == PREC_F16_Q8:
                    err, bar = rel_l2(got, want[:n]), F16_BAR
                else:
                    err, bar = nmse(got, f32_want), BF16_BAR
                print(f"tq | prompt {R.NAMES[t]} M={m} K={k} N={n} {name} | {labels} | {'rel-L2' if prec == PREC_F16_Q8 else 'NMSE'} {err:.3e} (bar {bar})")
                assert err <= bar
    finally:
        qmm.set_precision(PREC_F16_Q8)


def test_f16_prefill_overflow_of_code_3_is_a_loud_error_and_bf16_handles_it(qmm, ref):
    """TQ2_0's code 3 under d = 65504 is +131008: valid GGUF bits that the f16 the default prompt mode rounds weights to cannot hold.
    The launch must not return silently wrong numbers: qmm_synchronize reports it, QMM_PREC_BF16 computes the product, the mat-vec
    kernels are exact integer arithmetic and not affected.  TQ1_0 only ever holds +-d, which f16 holds: it runs in both modes"""
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8, QmmError
    k, m, n = 512, 64, 40
    for t in TYPES:
        w = np.array(case(ref, t, m, k, 70)[0]).reshape(m, -1, R.BLOCK_BYTES[t])
        w[5, 1, :R.D_AT[t]] = 0xff                                  # TQ2_0: every code 3; TQ1_0: every trit 2
        w[5, 1, R.D_AT[t]:] = np.array([0x7BFF], np.uint16).view(np.uint8)         # d = 65504
        w = w.reshape(m, -1)
        x = case(ref, t, m, k, 70)[1][:n]
        want = R.mul_mat_np(t, w, k, ref.quantize_act(x))
        f32_want = x.astype(np.float64) @ ref.dequantize(t, w, k).astype(np.float64).T
        assert np.isfinite(want).all()
        got1 = qmm.mul_mat(t, dev(w), k, dev(x[:4])).cpu().numpy()
        err = rel_rms(got1, want[:4])
        print(f"tq | d = 65504 {R.NAMES[t]} mat-vec | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert err <= MV_BAR
        qmm.synchronize()
        try:
            got = qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy()
            if t == R.TQ2_0:
                with pytest.raises(QmmError, match="non-finite"):
                    qmm.synchronize()
                print(f"tq | d = 65504 tq2_0 f16 prompt | reported: {qmm.lib.qmm_last_error().decode()}")
                qmm.synchronize()                                   # the report clears the condition
            else:
                qmm.synchronize()
                err = rel_l2(got, want)
                print(f"tq | d = 65504 tq1_0 f16 prompt | rel-L2 {err:.3e} (bar {F16_BAR})")
                assert err <= F16_BAR
            qmm.set_precision(PREC_BF16)
            got = qmm.mul_mat(t, dev(w), k, dev(x)).cpu().numpy()
            qmm.synchronize()
            err = nmse(got, f32_want)
            print(f"tq | d = 65504 {R.NAMES[t]} bf16 prompt | NMSE {err:.3e} (bar {BF16_BAR})")
            assert err <= BF16_BAR
        finally:
            qmm.set_precision(PREC_F16_Q8)


# ------------------------------------------------------------------------------------------------ MUL_MAT_ID

N_EXPERT, N_USED = 8, 2


def moe_case(ref, t, n_tokens, seed, routing):
    """8 experts of [64, 512], 2 used per token: weights [8, 64, row], b [n_tokens, 1, 512], ids.  routing "uniform": two distinct
    experts drawn per token; "last": every pair goes to expert 7, the rest get no row"""
    m, k = 64, 512
    rng = np.random.default_rng(7 * t + n_tokens + seed)
    w, _, _ = case(ref, t, N_EXPERT * m, k, 1)
    w = np.roll(w.reshape(N_EXPERT, m, -1), seed, axis=0)          # (seed 1: the same experts in another order, a second tensor)
    b = rng.uniform(-1, 1, (n_tokens, 1, k)).astype(np.float32)
    if routing == "uniform":
        ids = np.stack([rng.permutation(N_EXPERT)[:N_USED] for _ in range(n_tokens)]).astype(np.int32)
    else:
        ids = np.full((n_tokens, N_USED), N_EXPERT - 1, np.int32)
    return w, b, ids


def moe_want(ref, t, w, b, ids):
    k = b.shape[-1]
    acts = ref.quantize_act(b[:, 0])
    per_expert = {e: R.mul_mat_np(t, w[e], k, acts) for e in np.unique(ids)}                       # [n_tokens, m] each
    return np.stack([np.stack([per_expert[ids[i, s]][i] for s in range(ids.shape[1])]) for i in range(ids.shape[0])])


@pytest.mark.parametrize("routing", ["uniform", "last"])
@pytest.mark.parametrize("n_tokens", [1, 2, 3, 4, 5, 6, 7, 8, 32])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_mul_mat_id(qmm, ref, t, n_tokens, routing):
    k = 512
    w, b, ids = moe_case(ref, t, n_tokens, 0, routing)
    want = moe_want(ref, t, w, b, ids)
    wd, bd, idd = dev(w), dev(b), dev(ids)
    labels = qmm.trace(lambda: qmm.mul_mat_id(t, wd, k, bd, idd))
    got = qmm.mul_mat_id(t, wd, k, bd, idd).cpu().numpy()
    qmm.synchronize()
    few = 2 * n_tokens <= 16
    err, bar = (rel_rms(got, want), MV_BAR) if few else (rel_l2(got, want), F16_BAR)
    print(f"tq | mul_mat_id {R.NAMES[t]} experts 8 used 2 tokens {n_tokens} {routing} | {labels} | {'max|err|/rms' if few else 'rel-L2'} {err:.3e} (bar {bar})")
    assert labels[-1] == (f"matvec_id_kernel<{t}>" if few else f"mfma_kernel<{t},64>"), labels
    assert err <= bar


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_mul_mat_id_pair_and_swiglu_forms(qmm, ref, t):
    """the gate / up pair in one launch and the fused SwiGLU launch at 3 tokens x 2 slots, against the same references"""
    from test_gpu_iq1 import swiglu_bar
    k, n_tokens = 512, 3
    w0, b, ids = moe_case(ref, t, n_tokens, 0, "uniform")
    w1, _, _ = moe_case(ref, t, n_tokens, 1, "uniform")
    want = [moe_want(ref, t, w, b, ids) for w in (w0, w1)]
    w0d, w1d, bd, idd = dev(w0), dev(w1), dev(b), dev(ids)
    shape = (n_tokens, 2, 64)
    pair = [torch.full(shape, 777.0, device="cuda") for _ in range(2)]
    fused = torch.full(shape, 777.0, device="cuda")
    labels = qmm.trace(lambda: (qmm.mul_mat_id_pair(t, w0d, w1d, k, bd, idd, pair[0], pair[1]), qmm.mul_mat_id_swiglu(t, w0d, w1d, k, bd, idd, fused)))
    qmm.synchronize()
    assert labels == (f"matvec_id_kernel<{t}>", f"matvec_id_swiglu_kernel<{t}>"), labels
    for i, wd in enumerate((w0d, w1d)):
        err = rel_rms(pair[i].cpu().numpy(), want[i])
        print(f"tq | mul_mat_id pair {R.NAMES[t]} tensor {i} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert err <= MV_BAR
        assert torch.equal(pair[i].view(torch.int32), qmm.mul_mat_id(t, wd, k, bd, idd).view(torch.int32))
    g, u = want[0].astype(np.float64), want[1].astype(np.float64)
    err, bar = float(np.abs(fused.cpu().numpy() - g / (1.0 + np.exp(-g)) * u).max()), swiglu_bar(g, u)
    print(f"tq | mul_mat_id swiglu {R.NAMES[t]} | max|err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar
