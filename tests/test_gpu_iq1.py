"""IQ1_S / IQ1_M on the device, through the C-ABI: the grid both formats index comes from the live reference at run time
(tests/iq1_refs.py) and goes in through qmm_set_codebook; expected values are the reference's dequantizer (bit for bit) and the numpy
restatement of its scalar dot products on the reference's own Q8_K activations.

Bars (tests/test_gpu_parity.py:6-9): mat-vec max |err| / rms <= 2e-5; prompt batches rel-L2 <= 1e-3 in the f16 mode, NMSE <= 5e-4
under QMM_PREC_BF16.  The fused SwiGLU form has no bar of its own: silu(g) * u inherits the mat-vec bar of its two products through the
derivative of silu (``swiglu_bar``).  Every measured value is printed.

The IQ1 quantizers are slow, so a weight matrix is a few quantizer-made rows (QROWS, cached per K) followed by random-byte rows with
bounded scales (synth_weights): every byte pattern is a valid block, and random bytes reach indices, scales and delta signs a quantizer
seldom emits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import iq1_refs as R  # noqa: E402

TYPES = [R.IQ1_S, R.IQ1_M]
IDS = [R.NAMES[t] for t in TYPES]
Q4_K, IQ2_XXS = 12, 16
MV_BAR, F16_BAR, BF16_BAR = 2e-5, 1e-3, 5e-4
QROWS = 16


@pytest.fixture(scope="module")
def ref():
    return R.Iq1Ref()


@pytest.fixture(scope="module")
def qmm(ref):
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    q.set_codebook(R.IQ1_S, ref.codebook())                        # one table: either id enables both types
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


_cache, _made = {}, {}


def made_rows(ref, t, k):
    """QROWS rows of the reference's quantizer at this K; once per (type, K)"""
    if (t, k) not in _made:
        rng = np.random.default_rng(77 * t + k)
        _made[(t, k)] = ref.quantize(t, rng.uniform(-1, 1, (QROWS, k)).astype(np.float32))
    return _made[(t, k)]


def weights(ref, t, m, k, seed):
    from ggml_hexagon_amd import synth
    w = synth.synth_weights(t, m, k, seed=seed)
    q = made_rows(ref, t, k)[:m]
    w[:q.shape[0]] = q
    return w


def case(ref, t, m, k, n):
    """weights [m, row], activations x [n, k] and the expected product [n, m]; computed once per shape"""
    key = (t, m, k, n)
    if key not in _cache:
        rng = np.random.default_rng(1000 * t + m + k)
        w = weights(ref, t, m, k, seed=1000 * t + m + k)
        x = rng.uniform(-1, 1, (n, k)).astype(np.float32)
        want = R.mul_mat_np(t, w, k, ref.quantize_act(x), ref.codebook())
        for a in (w, x, want):
            a.setflags(write=False)
        _cache[key] = (w, x, want)
    return _cache[key]


def assert_covering(t, cover, k):
    d, idx, sign, scale = R._fields(t, cover, k)
    assert len(np.unique(idx)) == 2048 and set(np.unique(sign).tolist()) == {-1, 1}
    assert len(np.unique(scale[..., 0])) == 8 and len(np.unique(scale[..., 1])) == 8
    assert d.min() < 0 and np.abs(d).min() == 2.0 ** -24


# ------------------------------------------------------------------------------------------------ dequantize

@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_dequantize_bit_exact(qmm, ref, t):
    k = 512
    made = made_rows(ref, t, k)
    cover = R.covering_rows(t, k, seed=5)
    assert_covering(t, cover, k)
    for name, rows in (("quantizer", made), ("covering", cover)):
        got = qmm.dequantize(t, dev(rows), k).cpu().numpy()
        want = ref.dequantize(t, rows, k)
        same = np.array_equal(got.view(np.uint32), want.view(np.uint32))
        print(f"iq1 | dequantize {R.NAMES[t]} {name} rows {rows.shape[0]} | bit-exact {same}")
        assert same
        assert np.array_equal(R.dequantize_np(t, rows, k, ref.codebook()).view(np.uint32), want.view(np.uint32))


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


@pytest.mark.parametrize("set_as", TYPES, ids=[f"set-as-{n}" for n in IDS])
def test_without_a_codebook_nothing_runs_and_either_id_enables_both(ref, set_as):
    from ggml_hexagon_amd.capi import Qmm, QmmError
    k, m = 512, 64
    q = Qmm(0)
    try:
        calls, guards, wants = {}, [], []
        for t in TYPES:
            w, x, _ = case(ref, t, m, k, 3)
            wd, xd = dev(w), dev(x)
            we = dev(np.stack([w] * 4))
            b = dev(x.reshape(3, 1, k))
            ids = torch.zeros((3, 2), dtype=torch.int32, device="cuda")
            assert q.row_size(t, k) == R.row_size(t, k)            # geometry needs no table
            rows_call, rows_dst, keep = get_rows_call(q, t, wd, k, [1, 0])
            g = {name: torch.full(shape, -7.0, dtype=torch.float32, device="cuda")
                 for name, shape in (("mul_mat", (3, m)), ("mul_mat prompt", (12, m)), ("mul_mat_id", (3, 2, m)))}
            xp = dev(np.tile(x, (4, 1)))
            n = R.NAMES[t]
            calls[f"{n} mul_mat"] = lambda t=t, wd=wd, xd=xd, g=g: q.mul_mat(t, wd, k, xd, out=g["mul_mat"])
            calls[f"{n} mul_mat prompt"] = lambda t=t, wd=wd, xp=xp, g=g: q.mul_mat(t, wd, k, xp, out=g["mul_mat prompt"])
            calls[f"{n} mul_mat_id"] = lambda t=t, we=we, b=b, ids=ids, g=g: q.mul_mat_id(t, we, k, b, ids, out=g["mul_mat_id"])
            calls[f"{n} get_rows"] = rows_call
            calls[f"{n} dequantize"] = lambda t=t, wd=wd: q.dequantize(t, wd, k)
            guards += list(g.values())
            wants.append((rows_dst, ref.dequantize(t, w[[1, 0]], k), keep))
        for name, fn in calls.items():
            with pytest.raises(QmmError, match="codebook"):
                fn()
            print(f"iq1 | no codebook | {name} refused: {q.lib.qmm_last_error().decode()}")
        q.synchronize()
        for g in guards + [w[0] for w in wants]:                   # nothing was computed
            assert float(g.min()) == -7.0 and float(g.max()) == -7.0
        q.set_codebook(set_as, ref.codebook())
        q.set_codebook(set_as, ref.codebook())                     # twice with the same table is fine
        for name, fn in calls.items():
            fn()
        q.synchronize()
        for rows_dst, want, _ in wants:
            assert np.array_equal(rows_dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
        for g in guards:
            assert not bool((g == -7.0).any())
    finally:
        q.close()


def test_bad_arguments(qmm, ref):
    from ggml_hexagon_amd.capi import QmmError
    for t in TYPES:
        for n in (2048, 4095, 0):                                  # the count is in words: 2048 entries of two
            with pytest.raises(QmmError, match="entries"):
                qmm.set_codebook(t, np.zeros(n, np.uint32))
        for byte in (2, 0x7f):                                     # a byte that is none of -1, 0, +1, in the last place
            bad = ref.codebook().copy()
            bad[-1] = (bad[-1] & 0x00ffffff) | (byte << 24)
            with pytest.raises(QmmError, match=r"-1, 0, \+1"):
                qmm.set_codebook(t, bad)
    with pytest.raises(QmmError, match="type"):                    # IQ2_XXS is still no type of this library
        qmm.set_codebook(IQ2_XXS, np.zeros(4096, np.uint32))
    assert qmm.row_size(IQ2_XXS, 4096) == 0
    for t in TYPES:                                                # no Q8-exact mode and no planar rows for the new types
        assert qmm.q8_exact_supported(t, 4096) == 0 and qmm.planar_type(t, 4096, R.row_size(t, 4096)) == 0
    # the refusals left the table as it was: rows that use every entry still dequantize bit for bit
    for t in TYPES:
        cover = R.covering_rows(t, 256, seed=3)
        assert np.array_equal(qmm.dequantize(t, dev(cover), 256).cpu().numpy().view(np.uint32), ref.dequantize(t, cover, 256).view(np.uint32))


# ------------------------------------------------------------------------------------------------ mat-vec

# one block (most lanes killed); ragged rows against the waves; more rows than a workgroup's waves; two units per lane; a long K that
# is no power of two
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
        print(f"iq1 | matvec {R.NAMES[t]} M={m} K={k} N={n} | {labels} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert labels == (f"matvec_kernel<{t},{n},false>",)
        assert err <= MV_BAR
    live = ref.mul_mat(t, w[:4], k, x[:2])                         # the live reference's own (SIMD) dot on a corner of the case
    err = rel_rms(want[:2, :4], live)
    print(f"iq1 | matvec {R.NAMES[t]} M={m} K={k} | numpy restatement against the live dot, corner: max|err|/rms {err:.3e}")
    assert err <= MV_BAR


@pytest.mark.parametrize("n", [1, 8, 70])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_strides_and_guard_columns(qmm, ref, t, n):
    """w_row_bytes and ldd larger than the row and M: the padding is neither read as weights nor written.  IQ1_S blocks stay on 2-byte
    boundaries (6 spare bytes), IQ1_M blocks on 8-byte ones (8 spare bytes), the alignment the library requires of them"""
    m, k = 33, 768
    pad = 6 if t == R.IQ1_S else 8
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
    print(f"iq1 | strides {R.NAMES[t]} M={m} K={k} N={n} row {row}+{pad} ldd {m}+16 | {labels} | {'max|err|/rms' if n <= 8 else 'rel-L2'} {err:.3e} (bar {bar})")
    assert np.all(got[:, m:] == 123.0)
    assert err <= bar
    assert np.array_equal(got[:, :m].view(np.uint32), plain.view(np.uint32))


def test_iq1_m_rows_off_8_byte_boundaries_are_refused(qmm, ref):
    """block_iq1_m is 8-byte aligned (its scales are read as one 8-byte word): a row stride or a base address that is no multiple of 8
    is refused with a message, by every entry point, and nothing is written"""
    from ggml_hexagon_amd.capi import QmmError
    t, m, k = R.IQ1_M, 33, 768
    w, x, _ = case(ref, t, m, k, 70)
    row = w.shape[1]
    wp = np.full((m, row + 12), 0xa5, np.uint8)
    wp[:, :row] = w
    strided = dev(wp)[:, :row]                                     # stride row + 12: every other row on a 4-byte boundary only
    flat = torch.zeros(m * row + 16, dtype=torch.uint8, device="cuda")
    shifted = flat[4:4 + m * row].view(m, row)                     # base address 4 off
    xd = dev(x[:1])
    for name, wd in (("row stride", strided), ("base address", shifted)):
        out = torch.full((1, m), 123.0, dtype=torch.float32, device="cuda")
        with pytest.raises(QmmError, match="8-byte"):
            qmm.mul_mat(t, wd, k, xd, out=out)
        print(f"iq1 | iq1_m {name} off 8 bytes | mul_mat refused: {qmm.lib.qmm_last_error().decode()}")
        with pytest.raises(QmmError, match="8-byte"):
            qmm.dequantize(t, wd, k)
        qmm.synchronize()
        assert bool((out == 123.0).all())


# ------------------------------------------------------------------------------------------------ groups

def run_group(qmm, members, k, xd, ldd_pad=0):
    outs = [torch.full((xd.shape[0], wd.shape[0] + ldd_pad), -3.0, dtype=torch.float32, device="cuda")[:, :wd.shape[0]] for _, wd in members]
    labels = qmm.trace(lambda: qmm.mul_mat_group(members, k, xd, outs))
    qmm.synchronize()
    return [o.cpu().numpy() for o in outs], labels


@pytest.mark.parametrize("n", [1, 5])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_group_with_q4_k_equals_the_single_calls(qmm, ref, t, n):
    """attn_q / attn_k in IQ1 beside a Q4_K attn_v, as a stock dense IQ1_S or IQ1_M file lays a layer out"""
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
        single = qmm.mul_mat(tt, wd, k, xd)
        assert torch.equal(torch.from_numpy(g).view(torch.int32), single.cpu().view(torch.int32))
    print(f"iq1 | group ({R.NAMES[t]}, {R.NAMES[t]}, q4_K) N={n} | {labels} | bit-equal to the single calls")


@pytest.mark.parametrize("n", [1, 5])
def test_gate_up_pair_of_both_types_equals_the_single_calls(qmm, ref, n):
    k = 1024
    wg, x, _ = case(ref, R.IQ1_S, 96, k, 40)
    wu, _, _ = case(ref, R.IQ1_M, 96, k, 40)
    members = [(R.IQ1_S, dev(wg)), (R.IQ1_M, dev(wu))]
    xd = dev(x[:n])
    got, labels = run_group(qmm, members, k, xd)
    assert labels == (f"matvec_kernel<{R.IQ1_S},{n},false>", f"matvec_kernel<{R.IQ1_M},{n},false>"), labels
    for (tt, wd), g in zip(members, got):
        assert torch.equal(torch.from_numpy(g).view(torch.int32), qmm.mul_mat(tt, wd, k, xd).cpu().view(torch.int32))


# ------------------------------------------------------------------------------------------------ prompt batches

@pytest.mark.parametrize("m,k", [(100, 512), (100, 1024), (256, 512), (256, 1024)])     # a ragged last tile and whole tiles; 8 and 16 K steps
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_prompt(qmm, ref, t, m, k):
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8
    w, x, want = case(ref, t, m, k, 40)
    wd = dev(w)
    deq = ref.dequantize(t, w, k).astype(np.float64)
    try:
        for n in (9, 40) if (m, k) == (100, 512) else (40,):       # 9: the first prompt batch, once per type
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
                print(f"iq1 | prompt {R.NAMES[t]} M={m} K={k} N={n} {name} | {labels} | {'rel-L2' if prec == PREC_F16_Q8 else 'NMSE'} {err:.3e} (bar {bar})")
                assert err <= bar
    finally:
        qmm.set_precision(PREC_F16_Q8)


# ------------------------------------------------------------------------------------------------ MUL_MAT_ID

N_EXPERT, N_USED = 8, 2


def moe_case(ref, t, n_tokens, seed, routing):
    """8 experts of [64, 512], 2 used per token: weights [8, 64, row], b [n_tokens, 1, 512], ids, expected [n_tokens, 2, 64].  routing
    "uniform": two distinct experts drawn per token; "last": every pair goes to expert 7, the rest get no row"""
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
    per_expert = {e: R.mul_mat_np(t, w[e], k, acts, ref.codebook()) for e in np.unique(ids)}        # [n_tokens, m] each
    return np.stack([np.stack([per_expert[ids[i, s]][i] for s in range(ids.shape[1])]) for i in range(ids.shape[0])])


@pytest.mark.parametrize("routing", ["uniform", "last"])
@pytest.mark.parametrize("n_tokens", [3, 40])
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
    print(f"iq1 | mul_mat_id {R.NAMES[t]} experts 8 used 2 tokens {n_tokens} {routing} | {labels} | {'max|err|/rms' if few else 'rel-L2'} {err:.3e} (bar {bar})")
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
        print(f"iq1 | mul_mat_id pair {R.NAMES[t]} tensor {i} | max|err|/rms {err:.3e} (bar {MV_BAR})")
        assert err <= MV_BAR
        assert torch.equal(pair[i].view(torch.int32), qmm.mul_mat_id(t, wd, k, bd, idd).view(torch.int32))
    g, u = want[0].astype(np.float64), want[1].astype(np.float64)
    err, bar = float(np.abs(fused.cpu().numpy() - g / (1.0 + np.exp(-g)) * u).max()), swiglu_bar(g, u)
    print(f"iq1 | mul_mat_id swiglu {R.NAMES[t]} | max|err| {err:.3e} (bar {bar:.3e})")
    assert err <= bar


# ------------------------------------------------------------------------------------------------ GET_ROWS

@pytest.mark.parametrize("k", [256, 1024])
@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_get_rows_bit_exact(qmm, ref, t, k):
    w, _, _ = case(ref, t, 8, k, 1)
    for idv in ([3, 7, 0, 3, 5, 1], [7, 6, 5, 4, 3, 2, 1, 0]):     # permuted with a repeated index and the last row; reversed
        call, dst, keep = get_rows_call(qmm, t, dev(w), k, idv)
        labels = qmm.trace(call)
        qmm.synchronize()
        want = ref.dequantize(t, w[idv], k)
        same = np.array_equal(dst.cpu().numpy().view(np.uint32), want.view(np.uint32))
        print(f"iq1 | get_rows {R.NAMES[t]} K={k} rows {idv} | {labels} | bit-exact {same}")
        assert labels == (f"get_rows_q_kernel<{t}>",) and same
