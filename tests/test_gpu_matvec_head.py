"""The head of the few-token mat-vec kernels (csrc/qmm_matvec.hiph, csrc/qmm_moe.hiph): the thread's first activation loads, behind
them the lookup of the wave's first row, the workgroup barrier, the request of the first weight slice, then the staging.

A reordered head goes wrong where the lookup and the early request meet an edge, so the shapes are the smallest that have one:
fewer rows than waves (idle waves look up a clamped row and must store nothing), K = 256 (one block: 4 units in a 64-lane wave, the lane
clamp of the early request), K = 14336, matrix boundaries inside one workgroup (the first rows of its waves fall into different
matrices), 1 / 2 / 8 tokens, the mixed-type launch (the early request is used by Q4_K rows only), the folds of qmm_mul_mat_group_ex on
each staging path (one-pass norm, two-step norm, SwiGLU, residual), MUL_MAT_ID at its first and last expert, and a captured launch
replayed on rewritten input.  Every result against the C oracle at the mat-vec bar, max |err| / rms <= 2e-5 (only the order of the f32
sums differs from the CPU); for the folds the oracle is fed the numpy-normed row and its products go through numpy's SwiGLU / add."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from oracle.pyoracle import ACT_REF, Q4_0, Q4_K, Q6_K, Q8_0, TYPE_NAMES  # noqa: E402

BAR = 2e-5
MV_MAX_GROUP = 4
SENTINEL = -77.25
# (wire type, planar): Q4_K, Q6_K wire and planar, Q4_0 planar, Q8_0 planar
KINDS = [(Q4_K, False), (Q6_K, False), (Q6_K, True), (Q4_0, True), (Q8_0, True)]
KIND_IDS = ["q4_K", "q6_K", "q6_K-planar", "q4_0-planar", "q8_0-planar"]


@pytest.fixture(scope="module")
def qmm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
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


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


def rms_norm(x, w, eps):
    x64 = x.astype(np.float64)
    return (x * (1.0 / np.sqrt((x64 * x64).mean(axis=-1, keepdims=True) + eps)).astype(np.float32) * w).astype(np.float32)


_weights, _inputs, _products = {}, {}, {}


def weights(t, m, k, seed):
    """wire rows of type t (numpy), made once"""
    import ggml_hexagon_amd.synth as synth
    key = (t, m, k, seed)
    if key not in _weights:
        _weights[key] = synth.synth_weights(t, m, k, seed=seed, sigma=0.25)
    return _weights[key]


def inputs(n, k, seed=0):
    key = (n, k, seed)
    if key not in _inputs:
        _inputs[key] = np.random.default_rng(1000 + 17 * n + k + seed).normal(0, 1.0, (n, k)).astype(np.float32)
    return _inputs[key]


def product(oracle, t, m, k, seed, n, xseed=0):
    """the oracle's W x for weights(t, m, k, seed) and inputs(n, k, xseed), computed once and shared"""
    key = (t, m, k, seed, n, xseed)
    if key not in _products:
        _products[key] = oracle.mul_mat(t, weights(t, m, k, seed), k, inputs(n, k, xseed), ACT_REF)
    return _products[key]


def on_device(qmm, t, a, k, planar):
    """(type code, device rows) of wire rows a, repacked in place where the planar layout is asked for"""
    w = dev(a)
    return (qmm.repack_rows(t, w, k) if planar else t), w


def planar_ok(t, k, planar):
    """planar rows exist for Q4_0 / Q8_0 (K a multiple of 256) and Q6_K (of 2048)"""
    return not planar or (t in (Q4_0, Q8_0, Q6_K) and k % (2048 if t == Q6_K else 256) == 0)


def run_group(qmm, oracle, spec, k, n, planar=False, check=True):
    """spec: (type, rows, seed) per matrix, one launch; returns the labels.  Every output sits in a wider sentinel-filled buffer."""
    ws, outs, bufs = [], [], []
    for t, m, seed in spec:
        ws.append(on_device(qmm, t, weights(t, m, k, seed), k, planar and planar_ok(t, k, True)))
        buf = torch.full((n, m + 24), SENTINEL, device="cuda")
        bufs.append(buf)
        outs.append(buf[:, :m])
    x = dev(inputs(n, k))
    labels = qmm.trace(lambda: qmm.mul_mat_group(ws, k, x, outs))
    for (t, m, seed), buf in zip(spec, bufs):
        got = buf.cpu().numpy()
        assert np.all(got[:, m:] == np.float32(SENTINEL)), (TYPE_NAMES[t], m, k, n, "stored past the matrix's rows")
        if check:
            err = rel_rms(got[:, :m], product(oracle, t, m, k, seed, n))
            assert err <= BAR, (TYPE_NAMES[t], m, k, n, err)
    return labels


FEW_ROWS = [(kind, k) for k in (256, 4096) for kind in KINDS if planar_ok(kind[0], k, kind[1])]


@pytest.mark.parametrize("kind,k", FEW_ROWS, ids=[f"{KIND_IDS[KINDS.index(kind)]}-{k}" for kind, k in FEW_ROWS])
def test_fewer_rows_than_waves(qmm, oracle, kind, k):
    """one matrix of 8 rows: more waves in the launch than rows, the idle ones look up a clamped row; nothing lands beyond row 8"""
    t, planar = kind
    for n in (1, 2, 8):
        labels = run_group(qmm, oracle, [(t, 8, 3)], k, n, planar)
        assert len(labels) == 1 and labels[0].startswith("matvec_kernel<"), labels


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
def test_long_rows(qmm, oracle, kind):
    """K = 14336: rows of several slices, the staging of 14 waves (Q8_K) or of every thread in several trips (Q8_0)"""
    t, planar = kind
    for n in (1, 2):
        run_group(qmm, oracle, [(t, 40, 5)], 14336, n, planar)


@pytest.mark.parametrize("kind", KINDS, ids=KIND_IDS)
@pytest.mark.parametrize("n", [1, 2, 8])
def test_matrix_boundaries_inside_a_workgroup(qmm, oracle, kind, n):
    """40 + 24 + 8 rows, and MV_MAX_GROUP matrices of 8 rows: the first rows of one workgroup's waves belong to different matrices"""
    t, planar = kind
    for k in (256, 4096):
        if not planar_ok(t, k, planar):
            continue
        labels = run_group(qmm, oracle, [(t, 40, 11), (t, 24, 12), (t, 8, 13)], k, n, planar)
        assert len(labels) == 1 and labels[0].startswith("matvec_kernel<"), labels
        labels = run_group(qmm, oracle, [(t, 8, 20 + i) for i in range(MV_MAX_GROUP)], k, n, planar)
        assert len(labels) == 1 and labels[0].startswith("matvec_kernel<"), labels


@pytest.mark.parametrize("n", [1, 2, 8])
def test_mixed_type_launch(qmm, oracle, n):
    """Q4_K + Q4_K + Q6_K at 40 / 24 / 8 rows in matvec_kmix_kernel: planar Q6_K at K = 4096, wire Q6_K (rows that are not 16-byte
    aligned) at K = 256 and 4096; and the Q6_K matrix first, so that wave 0's first row is no Q4_K row"""
    for k, planar in ((4096, True), (4096, False), (256, False)):
        labels = run_group(qmm, oracle, [(Q4_K, 40, 11), (Q4_K, 24, 12), (Q6_K, 8, 13)], k, n, planar)
        assert labels == (f"matvec_kmix_kernel<{n},false>",), labels
        run_group(qmm, oracle, [(Q6_K, 8, 13), (Q4_K, 40, 11), (Q4_K, 24, 12)], k, n, planar)


@pytest.mark.parametrize("k", [1024, 4096, 5120])
def test_norm_fold(qmm, oracle, k):
    """rms_norm * w formed while staging: one pass at K = 1024 and 4096 (the hook behind stage_q8k_rows' loads), two steps at K = 5120
    (no early request); a same-type group, the mixed-type launch and planar Q4_0 (always two steps), 1 and 2 tokens"""
    rng = np.random.default_rng(k)
    nw = rng.normal(1, 0.1, k).astype(np.float32)
    for spec in ([(Q4_K, 40, 11), (Q4_K, 24, 12), (Q4_K, 8, 13)], [(Q4_K, 40, 11), (Q4_K, 24, 12), (Q6_K, 8, 13)], [(Q4_0, 40, 14), (Q4_0, 8, 15)]):
        for n in (1, 2):
            x = inputs(n, k, 1)
            xn = rms_norm(x, nw, 1e-5)
            ws = [on_device(qmm, t, weights(t, m, k, seed), k, t == Q4_0) for t, m, seed in spec]
            outs = [torch.full((n, m), SENTINEL, device="cuda") for _, m, _ in spec]
            qmm.mul_mat_group_ex(ws, k, dev(x), outs, norm_w=dev(nw), eps=1e-5)
            for (t, m, seed), o in zip(spec, outs):
                err = rel_rms(o.cpu().numpy(), oracle.mul_mat(t, weights(t, m, k, seed), k, xn, ACT_REF))
                assert err <= BAR, (TYPE_NAMES[t], m, k, n, err)


@pytest.mark.parametrize("which", [1, 2])
def test_swiglu_fold(qmm, oracle, which):
    """silu(W_gate x) * (W_up x) by row pairs, gate first (swiglu = 1: the early request is the gate row's) and up first (2)"""
    for t, planar, k, m in ((Q4_K, False, 4096, 40), (Q4_K, False, 256, 8), (Q4_0, True, 1024, 24)):
        for n in (1, 2):
            g = product(oracle, t, m, k, 31, n).astype(np.float64)
            u = product(oracle, t, m, k, 32, n).astype(np.float64)
            want = g / (1.0 + np.exp(-g)) * u
            wg, wu = on_device(qmm, t, weights(t, m, k, 31), k, planar), on_device(qmm, t, weights(t, m, k, 32), k, planar)
            outs = [torch.full((n, m), SENTINEL, device="cuda"), torch.full((n, m), SENTINEL, device="cuda")]
            qmm.mul_mat_group_ex([wg, wu] if which == 1 else [wu, wg], k, dev(inputs(n, k)), outs, swiglu=which)
            err = rel_rms(outs[0].cpu().numpy(), want)
            assert err <= BAR, (TYPE_NAMES[t], k, n, which, err)
            assert torch.all(outs[1] == SENTINEL)


@pytest.mark.parametrize("n", [1, 2, 8])
def test_residual_fold(qmm, oracle, n):
    """dst = W x + residual in the epilogue, same-type group and mixed-type launch, rows 40 / 24 / 8"""
    rng = np.random.default_rng(n)
    for k, types in ((4096, (Q4_K, Q4_K, Q4_K)), (4096, (Q4_K, Q4_K, Q6_K)), (256, (Q4_K, Q4_K, Q6_K))):
        spec = [(types[0], 40, 11), (types[1], 24, 12), (types[2], 8, 13)]
        ws = [on_device(qmm, t, weights(t, m, k, seed), k, False) for t, m, seed in spec]
        res = [rng.normal(0, 1, (n, m)).astype(np.float32) for _, m, _ in spec]
        outs = [torch.full((n, m), SENTINEL, device="cuda") for _, m, _ in spec]
        qmm.mul_mat_group_ex(ws, k, dev(inputs(n, k)), outs, residuals=[dev(r) for r in res])
        for (t, m, seed), o, r in zip(spec, outs, res):
            err = rel_rms(o.cpu().numpy(), product(oracle, t, m, k, seed, n).astype(np.float64) + r)
            assert err <= BAR, (TYPE_NAMES[t], m, k, n, err)


@pytest.mark.parametrize("k", [256, 4096])
def test_mul_mat_id_first_and_last_expert(qmm, oracle, k):
    """one token, 8 experts, two used, 16 rows: ids name expert 0 and expert 7; the single tensor and the pair that shares b and ids"""
    m, n_expert = 16, 8
    w0 = np.stack([weights(Q4_K, m, k, 40 + e) for e in range(n_expert)])
    w1 = np.stack([weights(Q4_K, m, k, 60 + e) for e in range(n_expert)])
    b = inputs(1, k, 2).reshape(1, 1, k)
    for pair in ((0, 7), (7, 0)):
        ids = np.array([pair], dtype=np.int32)
        want0, want1 = oracle.mul_mat_id(Q4_K, w0, k, m, b, ids), oracle.mul_mat_id(Q4_K, w1, k, m, b, ids)
        got = qmm.mul_mat_id(Q4_K, dev(w0), k, dev(b), dev(ids)).cpu().numpy()
        assert rel_rms(got, want0) <= BAR, (k, pair, rel_rms(got, want0))
        o0, o1 = torch.full((1, 2, m), SENTINEL, device="cuda"), torch.full((1, 2, m), SENTINEL, device="cuda")
        qmm.mul_mat_id_pair(Q4_K, dev(w0), dev(w1), k, dev(b), dev(ids), o0, o1)
        assert rel_rms(o0.cpu().numpy(), want0) <= BAR and rel_rms(o1.cpu().numpy(), want1) <= BAR, (k, pair)


def test_graph_replay_on_rewritten_input(qmm, oracle):
    """one group launch captured in a graph; the input buffer is rewritten between replays and each replay matches the oracle"""
    k, n = 4096, 1
    spec = [(Q4_K, 40, 11), (Q4_K, 24, 12), (Q4_K, 8, 13)]
    ws = [on_device(qmm, t, weights(t, m, k, seed), k, False) for t, m, seed in spec]
    outs = [torch.full((n, m), SENTINEL, device="cuda") for _, m, _ in spec]
    x = dev(inputs(n, k, 0))
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        qmm.mul_mat_group(ws, k, x, outs)                        # (warm-up outside the capture)
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=s):
            qmm.mul_mat_group(ws, k, x, outs)
    torch.cuda.current_stream().wait_stream(s)
    for xseed in (0, 3, 4):
        x.copy_(dev(inputs(n, k, xseed)))
        for o in outs:
            o.fill_(SENTINEL)
        gr.replay()
        torch.cuda.synchronize()
        for (t, m, seed), o in zip(spec, outs):
            err = rel_rms(o.cpu().numpy(), product(oracle, t, m, k, seed, n, xseed))
            assert err <= BAR, (TYPE_NAMES[t], m, xseed, err)
