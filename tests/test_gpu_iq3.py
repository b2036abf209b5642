"""IQ3_XXS / IQ3_S on the device, through the C-ABI: the grids come from the live reference at run time (tests/iq3_refs.py) and go in
through qmm_set_codebook; expected values are the reference's dequantizer (bit for bit) and the numpy restatement of its scalar dot
products on the reference's own Q8_K activations.

Bars (tests/test_gpu_parity.py:6-9): mat-vec max |err| / rms <= 2e-5; prompt batches rel-L2 <= 1e-3 in the f16 mode, NMSE <= 5e-4
under QMM_PREC_BF16.  Every measured value is printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import iq3_refs as R  # noqa: E402

TYPES = [R.IQ3_XXS, R.IQ3_S]
IDS = [R.NAMES[t] for t in TYPES]
Q4_K, IQ2_XXS = 12, 16
MV_BAR, F16_BAR, BF16_BAR = 2e-5, 1e-3, 5e-4


@pytest.fixture(scope="module")
def ref():
    return R.Iq3Ref()


@pytest.fixture(scope="module")
def qmm(ref):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    for t in TYPES:
        q.set_codebook(t, ref.codebook(t))
    yield q
    q.close()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # (a copy: the cached cases are read-only)


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def rel_l2(got, want):
    want = want.astype(np.float64)
    return float(np.sqrt(np.sum((got - want) ** 2) / max(np.sum(want ** 2), 1e-30)))


def nmse(got, want):
    return rel_l2(got, want) ** 2


_cache = {}


def case(ref, t, m, k, n):
    """quantizer-made weights [m, row], activations x [n, k] and the expected product [n, m]; computed once per shape"""
    key = (t, m, k, n)
    if key not in _cache:
        rng = np.random.default_rng(1000 * t + m + k)
        w = ref.quantize(t, rng.uniform(-1, 1, (m, k)).astype(np.float32))
        x = rng.uniform(-1, 1, (n, k)).astype(np.float32)
        want = R.mul_mat_np(t, w, k, ref.quantize_act(x), ref.codebook(t))
        for a in (w, x, want):
            a.setflags(write=False)
        _cache[key] = (w, x, want)
    return _cache[key]


# ------------------------------------------------------------------------------------------------ dequantize

@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_dequantize_bit_exact(qmm, ref, t):
    k = 512
    rng = np.random.default_rng(t)
    made = ref.quantize(t, (rng.standard_normal((64, k)) * 0.05).astype(np.float32))
    cover = R.covering_rows(t, k, seed=5)
    fields = R._fields(t, cover, k)
    n_signs = 128 if t == R.IQ3_XXS else 256                       # IQ3_XXS: eight signs of even parity out of a 7-bit index
    assert len(np.unique(fields[1])) == R.ENTRIES[t] and len(np.unique(fields[2])) == n_signs and len(np.unique(fields[3])) == 16
    for name, rows in (("quantizer", made), ("covering", cover)):
        got = qmm.dequantize(t, dev(rows), k).cpu().numpy()
        want = ref.dequantize(t, rows, k)
        same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
        print(f"iq3 | dequantize {R.NAMES[t]} {name} rows {rows.shape[0]} | bit-exact {same}")
        assert same
        assert np.array_equal(R.dequantize_np(t, rows, k, ref.codebook(t)).view(np.uint32), want.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the codebook gate

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


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_without_a_codebook_nothing_runs(ref, t):
    from ggml_hexagon_amd.capi import Qmm, QmmError
    k, m = 512, 64
    w, x, _ = case(ref, t, m, k, 3)
    wd, xd = dev(w), dev(x)
    we = dev(np.stack([w] * 4))
    b = dev(x.reshape(3, 1, k))
    ids = torch.zeros((3, 2), dtype=torch.int32, device="cuda")
    q = Qmm(0)
    try:
        assert q.row_size(t, k) == R.row_size(t, k)                # geometry needs no table
        rows_call, rows_dst, keep = get_rows_call(q, t, wd, k, [1, 0])
        calls = {"mul_mat": lambda: q.mul_mat(t, wd, k, xd),
                 "mul_mat prompt": lambda: q.mul_mat(t, wd, k, dev(np.tile(x, (4, 1)))),
                 "mul_mat_id": lambda: q.mul_mat_id(t, we, k, b, ids),
                 "get_rows": rows_call,
                 "dequantize": lambda: q.dequantize(t, wd, k)}
        for name, fn in calls.items():
            with pytest.raises(QmmError, match="codebook"):
                fn()
            print(f"iq3 | no codebook | {R.NAMES[t]} {name} refused: {q.lib.qmm_last_error().decode()}")
        q.synchronize()
        assert float(rows_dst.min()) == -7.0 and float(rows_dst.max()) == -7.0          # nothing was computed
        q.set_codebook(t, ref.codebook(t))
        q.set_codebook(t, ref.codebook(t))                         # twice with the same table is fine
        for name, fn in calls.items():
            fn()
        q.synchronize()
        assert np.array_equal(rows_dst.cpu().numpy().view(np.uint32), ref.dequantize(t, w[[1, 0]], k).view(np.uint32))
    finally:
        q.close()


def test_bad_arguments(qmm, ref):
    from ggml_hexagon_amd.capi import QmmError
    for t, n in ((R.IQ3_XXS, 512), (R.IQ3_S, 256), (R.IQ3_XXS, 255), (R.IQ3_S, 0)):
        with pytest.raises(QmmError, match="entries"):
            qmm.set_codebook(t, np.full(n, 0x01010101, np.uint32))
    for t in (IQ2_XXS, Q4_K, 0, 23):
        with pytest.raises(QmmError, match="type"):
            qmm.set_codebook(t, np.full(256, 0x01010101, np.uint32))
    bad = ref.codebook(R.IQ3_XXS).copy()
    bad[17] = (bad[17] & 0xffff00ff) | (200 << 8)                  # a magnitude that is no int8 with its sign
    with pytest.raises(QmmError, match="1 .. 127"):
        qmm.set_codebook(R.IQ3_XXS, bad)
    bad[17] &= 0xffff00ff                                          # ... and a zero
    with pytest.raises(QmmError, match="1 .. 127"):
        qmm.set_codebook(R.IQ3_XXS, bad)
    # IQ2_XXS is still no type of this library
    assert qmm.row_size(IQ2_XXS, 4096) == 0
    x = torch.zeros((1, 256), dtype=torch.float32, device="cuda")
    w = torch.zeros((4, 66), dtype=torch.uint8, device="cuda")
    with pytest.raises(QmmError, match="type"):
        qmm.mul_mat(IQ2_XXS, w, 256, x)
    # the refusals left the tables as they were
    k = 256
    w3, x3, want = case(ref, R.IQ3_XXS, 3, k, 1)
    assert rel_rms(qmm.mul_mat(R.IQ3_XXS, dev(w3), k, dev(x3)).cpu().numpy(), want) <= MV_BAR


# ------------------------------------------------------------------------------------------------ mat-vec

MV_SHAPES = [(1, 256), (3, 512), (33, 768), (64, 4096), (17, 14336)]


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
        print(f"iq3 | matvec {R.NAMES[t]} M={m} K={k} N={n} | {labels} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert labels == (f"matvec_kernel<{t},{n},false>",)
        assert err <= MV_BAR
    live = ref.mul_mat(t, w[:4], k, x[:2])                         # the live reference's own (SIMD) dot on a corner of the case
    assert rel_rms(want[:2, :4], live) <= MV_BAR


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_matvec_sub_batches_where_the_rows_do_not_fit_lds(qmm, ref, t):
    """matvec_group_plan's other branch for a same-type run: 8 rows of K = 16384 exceed the LDS estimate and go out as two launches of 4"""
    m, k = 5, 16384
    w, x, want = case(ref, t, m, k, 8)
    wd, xd = dev(w), dev(x)
    labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd))
    assert labels == (f"matvec_kernel<{t},4,false>",) * 2, labels
    err = rel_rms(qmm.mul_mat(t, wd, k, xd).cpu().numpy(), want)
    print(f"iq3 | matvec {R.NAMES[t]} M={m} K={k} N=8 in two sub-batches | max|err|/rms {err:.3e} (bar {MV_BAR})")
    assert err <= MV_BAR


# ------------------------------------------------------------------------------------------------ groups

def run_group(qmm, members, k, xd, ldd_pad=0):
    outs = [torch.full((xd.shape[0], wd.shape[0] + ldd_pad), -3.0, dtype=torch.float32, device="cuda")[:, :wd.shape[0]] for _, wd in members]
    labels = qmm.trace(lambda: qmm.mul_mat_group(members, k, xd, outs))
    qmm.synchronize()
    return [o.cpu().numpy() for o in outs], labels


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_group_with_q4_k_equals_the_single_calls(qmm, ref, t, n):
    """attn_q / attn_k in IQ3 beside a Q4_K attn_v, as a stock IQ3_XXS file lays a layer out: the IQ3 pair is one launch, Q4_K another"""
    import ggml_hexagon_amd.synth as synth
    k = 1024
    wq, x, _ = case(ref, t, 96, k, 8)
    wk, _, _ = case(ref, t, 33, k, 8)
    wv = synth.synth_weights(Q4_K, 40, k, seed=9, sigma=0.3)
    members = [(t, dev(wq)), (t, dev(wk)), (Q4_K, dev(wv))]
    xd = dev(x[:n])
    got, labels = run_group(qmm, members, k, xd)
    assert labels == (f"matvec_kernel<{t},{n},false>", f"matvec_kernel<{Q4_K},{n},false>"), labels
    for (tt, wd), g in zip(members, got):
        single = qmm.mul_mat(tt, wd, k, xd).cpu().numpy()
        assert np.array_equal(g.view(np.uint32), single.view(np.uint32))
    print(f"iq3 | group ({R.NAMES[t]}, {R.NAMES[t]}, q4_K) N={n} | {labels} | bit-equal to the single calls")


@pytest.mark.parametrize("n", [1, 5])
def test_gate_up_pair_of_both_types_equals_the_single_calls(qmm, ref, n):
    k = 1024
    wg, x, _ = case(ref, R.IQ3_S, 96, k, 8)
    wu, _, _ = case(ref, R.IQ3_XXS, 96, k, 8)
    members = [(R.IQ3_S, dev(wg)), (R.IQ3_XXS, dev(wu))]
    xd = dev(x[:n])
    got, labels = run_group(qmm, members, k, xd)
    assert labels == (f"matvec_kernel<{R.IQ3_S},{n},false>", f"matvec_kernel<{R.IQ3_XXS},{n},false>"), labels
    for (tt, wd), g in zip(members, got):
        assert np.array_equal(g.view(np.uint32), qmm.mul_mat(tt, wd, k, xd).cpu().numpy().view(np.uint32))


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_one_token_group_inside_a_chain_recording_launches_directly(qmm, ref, t):
    k = 512
    w, x, want = case(ref, t, 64, k, 3)
    wd, xd = dev(w), dev(x[:1])
    before = qmm.chain_stats()
    qmm.chain_begin()
    try:
        labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd))
        got = qmm.mul_mat(t, wd, k, xd)
    finally:
        qmm.chain_end()
    qmm.synchronize()
    assert labels == (f"matvec_kernel<{t},1,false>",) and qmm.chain_stats() == before
    assert rel_rms(got.cpu().numpy(), want[:1]) <= MV_BAR


# ------------------------------------------------------------------------------------------------ prompt batches

@pytest.mark.parametrize("m,k", [(16, 256), (65, 512), (256, 4096)])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_prompt(qmm, ref, t, m, k):
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8
    w, x, want = case(ref, t, m, k, 130)
    wd = dev(w)
    deq = ref.dequantize(t, w, k).astype(np.float64)
    try:
        for n in (9, 33, 130):
            xd = dev(x[:n])
            f32_want = x[:n].astype(np.float64) @ deq.T            # what QMM_PREC_BF16 approximates: no Q8 step
            for prec, name in ((PREC_F16_Q8, "f16"), (PREC_BF16, "bf16")):
                qmm.set_precision(prec)
                runs = []
                for _ in range(2):
                    big = torch.full((n, m + 16), 123.0, dtype=torch.float32, device="cuda")
                    labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd, out=big[:, :m]))
                    qmm.synchronize()
                    runs.append(big.cpu().numpy())
                assert labels[-1] == f"mfma_kernel<{t},64>", labels
                assert np.all(runs[0][:, m:] == 123.0)             # guard columns of ldd = M + 16
                assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32))
                got = runs[0][:, :m]
                if prec == PREC_F16_Q8:
                    err, bar = rel_l2(got, want[:n]), F16_BAR
                else:
                    err, bar = nmse(got, f32_want), BF16_BAR
                print(f"iq3 | prompt {R.NAMES[t]} M={m} K={k} N={n} {name} | {labels} | {'rel-L2' if prec == PREC_F16_Q8 else 'NMSE'} {err:.3e} (bar {bar})")
                assert err <= bar
    finally:
        qmm.set_precision(PREC_F16_Q8)


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_prompt_on_128_row_tiles(qmm, ref, t):
    """the plan's other tile: 128 rows once 128-row tiles alone give every CU of the chip a workgroup"""
    m, k, n = 32768, 256, 130
    rng = np.random.default_rng(t)
    w = np.tile(ref.quantize(t, rng.uniform(-1, 1, (512, k)).astype(np.float32)), (m // 512, 1))
    x = rng.uniform(-1, 1, (n, k)).astype(np.float32)
    rows = np.concatenate([np.arange(0, 512), np.arange(m - 512, m)])
    want = R.mul_mat_np(t, w[rows], k, ref.quantize_act(x), ref.codebook(t))
    wd, xd = dev(w), dev(x)
    labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd))
    got = qmm.mul_mat(t, wd, k, xd).cpu().numpy()
    qmm.synchronize()
    err = rel_l2(got[:, rows], want)
    print(f"iq3 | prompt {R.NAMES[t]} M={m} K={k} N={n} f16 | {labels} | rel-L2 {err:.3e} (bar {F16_BAR})")
    assert labels[-1] == f"mfma_kernel<{t},128>", labels
    assert err <= F16_BAR
    assert np.array_equal(got[:, :512].view(np.uint32), got[:, m - 512:].view(np.uint32))       # the same rows, tiled


# ------------------------------------------------------------------------------------------------ MUL_MAT_ID

@pytest.mark.parametrize("routing", ["uniform", "one_hot"])
@pytest.mark.parametrize("n_expert,n_used,n_tokens", [(4, 2, 1), (8, 2, 3), (8, 2, 40)])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_mul_mat_id(qmm, ref, t, n_expert, n_used, n_tokens, routing):
    import moe_cases
    m, k = 64, 512
    rng = np.random.default_rng(7 * t + n_tokens)
    w, _, _ = case(ref, t, 8 * m, k, 1)                              # eight experts' rows; the first n_expert are used
    w = w.reshape(8, m, -1)[:n_expert]
    b = rng.uniform(-1, 1, (n_tokens, 1, k)).astype(np.float32)
    gen = moe_cases.uniform if routing == "uniform" else moe_cases.one_hot(-1)     # skewed: every pair to the last expert
    ids = gen(n_tokens, n_used, n_expert, rng)
    acts = ref.quantize_act(b[:, 0])
    per_expert = [R.mul_mat_np(t, w[e], k, acts, ref.codebook(t)) for e in range(n_expert)]      # [n_tokens, m] each
    want = np.stack([np.stack([per_expert[ids[i, s]][i] for s in range(n_used)]) for i in range(n_tokens)])
    wd, bd, idd = dev(w), dev(b), dev(ids)
    labels = qmm.trace(lambda: qmm.mul_mat_id(t, wd, k, bd, idd))
    got = qmm.mul_mat_id(t, wd, k, bd, idd).cpu().numpy()
    qmm.synchronize()
    few = n_used * n_tokens <= 16
    err, bar = (rel_rms(got, want), MV_BAR) if few else (rel_l2(got, want), F16_BAR)
    print(f"iq3 | mul_mat_id {R.NAMES[t]} experts {n_expert} used {n_used} tokens {n_tokens} {routing} | {labels} | "
          f"{'max|err|/rms' if few else 'rel-L2'} {err:.3e} (bar {bar})")
    assert labels[-1] == (f"matvec_id_kernel<{t}>" if few else f"mfma_kernel<{t},64>"), labels
    assert err <= bar


# ------------------------------------------------------------------------------------------------ GET_ROWS

@pytest.mark.parametrize("k", [256, 1024])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_get_rows_bit_exact(qmm, ref, t, k):
    w, _, _ = case(ref, t, 8, k, 1)
    idv = [3, 7, 0, 3, 5]                                           # a repeated index and the last row
    call, dst, keep = get_rows_call(qmm, t, dev(w), k, idv)
    labels = qmm.trace(call)
    qmm.synchronize()
    want = ref.dequantize(t, w[idv], k)
    same = np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
    print(f"iq3 | get_rows {R.NAMES[t]} K={k} rows {idv} | {labels} | bit-exact {same}")
    assert labels == (f"get_rows_q_kernel<{t}>",) and same
