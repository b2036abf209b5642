"""IQ2_XS / IQ2_S on the device, through the C-ABI: the grids come from the live reference at run time (tests/iq2_refs.py) and go in
through qmm_set_codebook; expected values are the reference's dequantizer (bit for bit) and the numpy restatement of its scalar dot
products on the reference's own Q8_K activations.

Bars (tests/test_gpu_parity.py:6-9): mat-vec max |err| / rms <= 2e-5; prompt batches rel-L2 <= 1e-3 in the f16 mode, NMSE <= 5e-4
under QMM_PREC_BF16.  The fused SwiGLU form has no bar of its own: silu(g) * u inherits the mat-vec bar of its two products through the
derivative of silu (``swiglu_bar``).  Every measured value is printed."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import iq2_refs as R  # noqa: E402

TYPES = [R.IQ2_XS, R.IQ2_S]
IDS = [R.NAMES[t] for t in TYPES]
Q4_K, IQ2_XXS = 12, 16
MV_BAR, F16_BAR, BF16_BAR = 2e-5, 1e-3, 5e-4


@pytest.fixture(scope="module")
def ref():
    return R.Iq2Ref()


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
    _, idx, signs, nib = R._fields(t, cover, k)
    assert len(np.unique(idx)) == R.ENTRIES[t] and len(np.unique(signs)) == R.N_SIGNS[t]
    assert len(np.unique(nib[..., 0])) == 16 and len(np.unique(nib[..., 1])) == 16
    for name, rows in (("quantizer", made), ("covering", cover)):
        got = qmm.dequantize(t, dev(rows), k).cpu().numpy()
        want = ref.dequantize(t, rows, k)
        same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
        print(f"iq2 | dequantize {R.NAMES[t]} {name} rows {rows.shape[0]} | bit-exact {same}")
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
        guards = {name: torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
                  for name, shape in (("mul_mat", (3, m)), ("mul_mat prompt", (12, m)), ("mul_mat_id", (3, 2, m)))}
        xp = dev(np.tile(x, (4, 1)))
        calls = {"mul_mat": lambda: q.mul_mat(t, wd, k, xd, out=guards["mul_mat"]),
                 "mul_mat prompt": lambda: q.mul_mat(t, wd, k, xp, out=guards["mul_mat prompt"]),
                 "mul_mat_id": lambda: q.mul_mat_id(t, we, k, b, ids, out=guards["mul_mat_id"]),
                 "get_rows": rows_call,
                 "dequantize": lambda: q.dequantize(t, wd, k)}
        for name, fn in calls.items():
            with pytest.raises(QmmError, match="codebook"):
                fn()
            print(f"iq2 | no codebook | {R.NAMES[t]} {name} refused: {q.lib.qmm_last_error().decode()}")
        q.synchronize()
        for g in (rows_dst, *guards.values()):                     # nothing was computed
            assert float(g.min()) == -7.0 and float(g.max()) == -7.0
        q.set_codebook(t, ref.codebook(t))
        q.set_codebook(t, ref.codebook(t))                         # twice with the same table is fine
        for name, fn in calls.items():
            fn()
        q.synchronize()
        assert np.array_equal(rows_dst.cpu().numpy().view(np.uint32), ref.dequantize(t, w[[1, 0]], k).view(np.uint32))
        for g in guards.values():
            assert not bool((g == -7.0).any())
    finally:
        q.close()


def test_bad_arguments(qmm, ref):
    from ggml_hexagon_amd.capi import QmmError
    for t, n in ((R.IQ2_XS, 512), (R.IQ2_XS, 2048), (R.IQ2_S, 1024), (R.IQ2_XS, 1023), (R.IQ2_S, 0)):       # the count is in words
        with pytest.raises(QmmError, match="entries"):
            qmm.set_codebook(t, np.full(n, 0x01010101, np.uint32))
    for t in (IQ2_XXS, Q4_K, 0, 23):
        with pytest.raises(QmmError, match="type"):
            qmm.set_codebook(t, np.full(1024, 0x01010101, np.uint32))
    for t in TYPES:
        bad = ref.codebook(t).copy()
        bad[-1] = (bad[-1] & 0x00ffffff) | (200 << 24)             # a magnitude that is no int8 with its sign, in the last byte
        with pytest.raises(QmmError, match="1 .. 127"):
            qmm.set_codebook(t, bad)
        bad[-1] &= 0x00ffffff                                      # ... and a zero
        with pytest.raises(QmmError, match="1 .. 127"):
            qmm.set_codebook(t, bad)
    # IQ2_XXS is still no type of this library
    assert qmm.row_size(IQ2_XXS, 4096) == 0
    x = torch.zeros((1, 256), dtype=torch.float32, device="cuda")
    w = torch.zeros((4, 66), dtype=torch.uint8, device="cuda")
    with pytest.raises(QmmError, match="type"):
        qmm.mul_mat(IQ2_XXS, w, 256, x)
    # the refusals left the tables as they were: rows that use every entry still dequantize bit for bit
    for t in TYPES:
        cover = R.covering_rows(t, 256, seed=3)
        assert np.array_equal(qmm.dequantize(t, dev(cover), 256).cpu().numpy().view(np.uint32), ref.dequantize(t, cover, 256).view(np.uint32))


# ------------------------------------------------------------------------------------------------ mat-vec

# one block; ragged rows against the waves; more rows than a workgroup's waves; two units per lane; a long K that is no power of two
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
        print(f"iq2 | matvec {R.NAMES[t]} M={m} K={k} N={n} | {labels} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert labels == (f"matvec_kernel<{t},{n},false>",)
        assert err <= MV_BAR
    live = ref.mul_mat(t, w[:4], k, x[:2])                         # the live reference's own (SIMD) dot on a corner of the case
    assert rel_rms(want[:2, :4], live) <= MV_BAR


@pytest.mark.parametrize("n", [1, 8, 70])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_strides_and_guard_columns(qmm, ref, t, n):
    """w_row_bytes and ldd larger than the row and M: the padding is neither read as weights nor written"""
    m, k = 33, 768
    w, x, want = case(ref, t, m, k, 70)
    row = w.shape[1]
    wp = np.full((m, row + 6), 0xa5, np.uint8)                     # 6 spare bytes keep the rows on 2-byte boundaries
    wp[:, :row] = w
    wd = dev(wp)[:, :row]
    assert wd.stride(0) == row + 6
    xd = dev(x[:n])
    big = torch.full((n, m + 16), 123.0, dtype=torch.float32, device="cuda")
    labels = qmm.trace(lambda: qmm.mul_mat(t, wd, k, xd, out=big[:, :m]))
    qmm.synchronize()
    got = big.cpu().numpy()
    plain = qmm.mul_mat(t, dev(w), k, xd).cpu().numpy()
    err = rel_rms(got[:, :m], want[:n]) if n <= 8 else rel_l2(got[:, :m], want[:n])
    bar = MV_BAR if n <= 8 else F16_BAR
    print(f"iq2 | strides {R.NAMES[t]} M={m} K={k} N={n} row {row}+6 ldd {m}+16 | {labels} | {'max|err|/rms' if n <= 8 else 'rel-L2'} {err:.3e} (bar {bar})")
    assert np.all(got[:, m:] == 123.0)
    assert err <= bar
    assert np.array_equal(got[:, :m].view(np.uint32), plain.view(np.uint32))


# ------------------------------------------------------------------------------------------------ groups

def run_group(qmm, members, k, xd, ldd_pad=0):
    outs = [torch.full((xd.shape[0], wd.shape[0] + ldd_pad), -3.0, dtype=torch.float32, device="cuda")[:, :wd.shape[0]] for _, wd in members]
    labels = qmm.trace(lambda: qmm.mul_mat_group(members, k, xd, outs))
    qmm.synchronize()
    return [o.cpu().numpy() for o in outs], labels


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_group_with_q4_k_equals_the_single_calls(qmm, ref, t, n):
    """attn_q / attn_k in IQ2 beside a Q4_K attn_v, as the stock IQ3_XXS and IQ2_XS files lay a layer out"""
    import ggml_hexagon_amd.synth as synth
    k = 1024
    wq, x, _ = case(ref, t, 96, k, 40)
    wk, _, _ = case(ref, t, 33, k, 40)
    wv = synth.synth_weights(Q4_K, 40, k, seed=9, sigma=0.3)
    members = [(t, dev(wq)), (t, dev(wk)), (Q4_K, dev(wv))]
    xd = dev(x[:n])
    got, labels = run_group(qmm, members, k, xd, ldd_pad=4)
    assert labels == (f"matvec_kernel<{t},{n},false>", f"matvec_kernel<{Q4_K},{n},false>"), labels
    for (tt, wd), g in zip(members, got):
        single = qmm.mul_mat(tt, wd, k, xd).cpu().numpy()
        assert np.array_equal(g.view(np.uint32), single.view(np.uint32))
    print(f"iq2 | group ({R.NAMES[t]}, {R.NAMES[t]}, q4_K) N={n} | {labels} | bit-equal to the single calls")


@pytest.mark.parametrize("n", [1, 5])
def test_gate_up_pair_of_both_types_equals_the_single_calls(qmm, ref, n):
    k = 1024
    wg, x, _ = case(ref, R.IQ2_S, 96, k, 40)
    wu, _, _ = case(ref, R.IQ2_XS, 96, k, 40)
    members = [(R.IQ2_S, dev(wg)), (R.IQ2_XS, dev(wu))]
    xd = dev(x[:n])
    got, labels = run_group(qmm, members, k, xd)
    assert labels == (f"matvec_kernel<{R.IQ2_S},{n},false>", f"matvec_kernel<{R.IQ2_XS},{n},false>"), labels
    for (tt, wd), g in zip(members, got):
        assert np.array_equal(g.view(np.uint32), qmm.mul_mat(tt, wd, k, xd).cpu().numpy().view(np.uint32))


# ------------------------------------------------------------------------------------------------ prompt batches

@pytest.mark.parametrize("m,k", [(100, 512), (100, 1024), (256, 512), (256, 1024)])     # a ragged last tile and whole tiles; 8 and 16 K steps
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_prompt(qmm, ref, t, m, k):
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8
    w, x, want = case(ref, t, m, k, 130)
    wd = dev(w)
    deq = ref.dequantize(t, w, k).astype(np.float64)
    try:
        for n in (9, 70, 130):
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
                print(f"iq2 | prompt {R.NAMES[t]} M={m} K={k} N={n} {name} | {labels} | {'rel-L2' if prec == PREC_F16_Q8 else 'NMSE'} {err:.3e} (bar {bar})")
                assert err <= bar
    finally:
        qmm.set_precision(PREC_F16_Q8)


# ------------------------------------------------------------------------------------------------ MUL_MAT_ID

def moe_case(ref, t, n_tokens, seed):
    """4 experts of [64, 512], 2 used per token: weights [4, 64, row], b [n_tokens, 1, 512], ids, expected [n_tokens, 2, 64]"""
    n_expert, n_used, m, k = 4, 2, 64, 512
    rng = np.random.default_rng(7 * t + n_tokens + seed)
    w, _, _ = case(ref, t, n_expert * m, k, 1)
    w = np.roll(w.reshape(n_expert, m, -1), seed, axis=0)          # (seed 1: the same experts in another order, a second tensor)
    b = rng.uniform(-1, 1, (n_tokens, 1, k)).astype(np.float32)
    ids = np.stack([rng.permutation(n_expert)[:n_used] for _ in range(n_tokens)]).astype(np.int32)
    return w, b, ids


def moe_want(ref, t, w, b, ids):
    k = b.shape[-1]
    acts = ref.quantize_act(b[:, 0])
    per_expert = [R.mul_mat_np(t, w[e], k, acts, ref.codebook(t)) for e in range(w.shape[0])]      # [n_tokens, m] each
    return np.stack([np.stack([per_expert[ids[i, s]][i] for s in range(ids.shape[1])]) for i in range(ids.shape[0])])


@pytest.mark.parametrize("n_tokens", [3, 40])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_mul_mat_id(qmm, ref, t, n_tokens):
    k = 512
    w, b, ids = moe_case(ref, t, n_tokens, 0)
    want = moe_want(ref, t, w, b, ids)
    wd, bd, idd = dev(w), dev(b), dev(ids)
    labels = qmm.trace(lambda: qmm.mul_mat_id(t, wd, k, bd, idd))
    got = qmm.mul_mat_id(t, wd, k, bd, idd).cpu().numpy()
    qmm.synchronize()
    few = 2 * n_tokens <= 16
    err, bar = (rel_rms(got, want), MV_BAR) if few else (rel_l2(got, want), F16_BAR)
    print(f"iq2 | mul_mat_id {R.NAMES[t]} experts 4 used 2 tokens {n_tokens} | {labels} | {'max|err|/rms' if few else 'rel-L2'} {err:.3e} (bar {bar})")
    assert labels[-1] == (f"matvec_id_kernel<{t}>" if few else f"mfma_kernel<{t},64>"), labels
    assert err <= bar


def swiglu_bar(g, u):
    """max |err| allowed on silu(g) * u when g and u each meet the mat-vec bar (max |err| <= MV_BAR * rms): first order,
    |silu'| <= 1.1 everywhere, so |err| <= 1.1 max|u| dg + max|silu(g)| du; and 2e-6 max|want| for the f32 exp, divide and product"""
    silu = g / (1.0 + np.exp(-g))
    return MV_BAR * (1.1 * np.abs(u).max() * rms(g) + np.abs(silu).max() * rms(u)) + 2e-6 * np.abs(silu * u).max()


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_mul_mat_id_pair_and_swiglu_forms(qmm, ref, t):
    """the gate / up pair in one launch and the fused SwiGLU launch at 3 tokens x 2 slots, against the same references"""
    k, n_tokens = 512, 3
    w0, b, ids = moe_case(ref, t, n_tokens, 0)
    w1, _, _ = moe_case(ref, t, n_tokens, 1)
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
        print(f"iq2 | mul_mat_id pair {R.NAMES[t]} tensor {i} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert err <= MV_BAR
        assert torch.equal(pair[i].view(torch.int32), qmm.mul_mat_id(t, wd, k, bd, idd).view(torch.int32))
    g, u = want[0].astype(np.float64), want[1].astype(np.float64)
    err, bar = float(np.abs(fused.cpu().numpy() - g / (1.0 + np.exp(-g)) * u).max()), swiglu_bar(g, u)
    print(f"iq2 | mul_mat_id swiglu {R.NAMES[t]} | max|err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ GET_ROWS

@pytest.mark.parametrize("k", [256, 1024])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_get_rows_bit_exact(qmm, ref, t, k):
    w, _, _ = case(ref, t, 8, k, 1)
    idv = [3, 7, 0, 3, 5, 1]                                        # permuted, a repeated index and the last row
    call, dst, keep = get_rows_call(qmm, t, dev(w), k, idv)
    labels = qmm.trace(call)
    qmm.synchronize()
    want = ref.dequantize(t, w[idv], k)
    same = np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
    print(f"iq2 | get_rows {R.NAMES[t]} K={k} rows {idv} | {labels} | bit-exact {same}")
    assert labels == (f"get_rows_q_kernel<{t}>",) and same
