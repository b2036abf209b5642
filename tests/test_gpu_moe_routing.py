"""MUL_MAT_ID against the CPU oracle under skewed routing, at longer K, through every gathered kernel variant (the case table and the
routing patterns: tests/moe_cases.py; the launch plan of every case is pinned without a GPU in test_moe_routing_host.py, and asserted here
through qmm.trace on a 256-CU device).

Bars: per (token, slot) ROW, not per tensor: one wrong row must not hide among 400.
  * prompt path (more than 16 pairs), default precision: rel-L2 < 1e-3 per row, the project's MFMA bar (f16 operand rounding; it does not
    depend on the number of pairs);  QMM_PREC_BF16: NMSE < 5e-4 per row, the reference's bar;
  * few pairs (mat-vec kernels): max|err| / rms < 2e-5, the project's mat-vec bar; the SwiGLU form: see SWIGLU_BAR.
Run with -s to see the measured figures (profiles/moe_routing_errors.txt is that output)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import moe_cases as mc  # noqa: E402
from oracle.pyoracle import ACT_REF, Q2_K, Q3_K, Q4_1, Q4_K, Q8_0, TYPE_NAMES, WEIGHT_TYPES  # noqa: E402

IDS = [TYPE_NAMES[t] for t in WEIGHT_TYPES]
SENTINEL = 777.0
MFMA_BAR, BF16_BAR, MATVEC_BAR = 1e-3, 5e-4, 2e-5
# matvec_id_swiglu_kernel against silu(g) * u formed in float64 from the oracle's two products, max|err| / rms(want): 4 x the worst value
# measured over FEW_CASES and the twelve types on the kernel as it stood before these tests, 5.83e-6 (Q5_1, M = 41, 8 tokens x 2).  The
# two cases left out of that maximum are Q4_1 / Q5_1 at M = 300: there the old kernel gave 4.0e-4 because one Q8_1 block sum of one token
# was an f16 ulp off (test_gpu_parity.py::test_q8_1_block_sum_f16_ties_bit_exact); fixed, they are in line (profiles/moe_routing_errors.txt)
SWIGLU_BAR = 4 * 5.83e-6


@pytest.fixture(scope="module")
def qmm():
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)          # raises if the HIP library is missing or the device is not gfx950: no fallback
    yield q
    q.close()


@pytest.fixture(scope="module")
def qmm_q23_off():
    """a context with Q2_K / Q3_K prefill on the LDS-tile kernel (the switch is read when a context is created)"""
    from ggml_hexagon_amd.capi import Qmm
    old = os.environ.get("GGML_MI355X_REGB_Q23")
    os.environ["GGML_MI355X_REGB_Q23"] = "0"
    try:
        q = Qmm(0)
    finally:
        if old is None:
            os.environ.pop("GGML_MI355X_REGB_Q23", None)
        else:
            os.environ["GGML_MI355X_REGB_Q23"] = old
    yield q
    q.close()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pins_hold():
    """the labels of moe_cases are pinned for a 256-CU device; elsewhere only the label assertions are left out, never a parity check"""
    return torch.cuda.get_device_properties(0).multi_processor_count == mc.CUS


def row_rel_l2(got, want):
    """rel-L2 of every (token, slot) row: [n_tokens, n_used]"""
    want = want.astype(np.float64)
    return np.sqrt(np.sum((got - want) ** 2, axis=-1) / np.maximum(np.sum(want ** 2, axis=-1), 1e-30))


def rel_rms(got, want):
    want = want.astype(np.float64)
    return float(np.max(np.abs(got - want)) / max(np.sqrt(np.mean(want ** 2)), 1e-30))


# ---- operands and references: made once per (type, case, K[, pattern, ne11]), shared by the tests of a type, never written to

_made = {"type": None}


def _cache(t):
    if _made["type"] != t:
        _made.clear()
        _made["type"] = t
    return _made


def expert_weights(t, M, n_expert, k, seed=0):
    import ggml_hexagon_amd.synth as synth
    c, key = _cache(t), ("w", M, n_expert, k, seed)
    if key not in c:
        w = synth.synth_weights(t, n_expert * M, k, seed=1000 * seed + M + n_expert, sigma=0.25).reshape(n_expert, M, -1)
        c[key] = (w, dev(w))
    return c[key]


def activations(t, n_tokens, ne11, k):
    c, key = _cache(t), ("b", n_tokens, ne11, k)
    if key not in c:
        b = np.random.default_rng(n_tokens * 7 + ne11 + k).uniform(-1, 1, (n_tokens, ne11, k)).astype(np.float32)
        c[key] = (b, dev(b))
    return c[key]


def reference(oracle, t, case, k, name, ids, ne11):
    c, key = _cache(t), ("want", case.name, k, name, ne11)
    if key not in c:
        w, _ = expert_weights(t, case.M, case.n_expert, k)
        b, _ = activations(t, case.n_tokens, ne11, k)
        c[key] = oracle.mul_mat_id(t, w, k, case.M, b, ids, ACT_REF)
    return c[key]


def run_case(q, t, case, k, ids_d, ne11, check_label=True, **prep):
    """one qmm.mul_mat_id call into an output filled with the sentinel; the traced labels are the case's pins"""
    _, wd = expert_weights(t, case.M, case.n_expert, k)
    _, bd = activations(t, case.n_tokens, ne11, k)
    out = torch.full((case.n_tokens, case.n_used, case.M), SENTINEL, device="cuda")
    labels = q.trace(lambda: q.mul_mat_id(t, wd, k, bd, ids_d, out=out))
    if check_label and pins_hold():
        assert labels == mc.labels_of(case, t, k, **prep), (case.name, TYPE_NAMES[t], k, labels)
    return out


# ---- a. parity per pair: every pattern x every shape case, default precision

@pytest.mark.parametrize("ki", [0, 1], ids=["k0", "k1"])
@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_every_pattern_and_case_per_row(qmm, oracle, t, ki):
    """every routing pattern of every shape case into a sentinel-filled output, rel-L2 < 1e-3 for every (token, slot) row, labels as pinned.

    Q4_1 and Q5_1 met this bar only after moe_q81_sum_fix_kernel: the CPU reference multiplies the weights' m with the Q8_1 block sum
    s = f16(d * sum), the prompt kernels carry m inside the f16 weights and so use d16 * sum; without the correction the worst rows were
    1.0e-3 .. 1.54e-3 on every kernel variant and routing pattern alike (the oracle itself is that far from the exact product of the same
    quantized operands), while the whole-tensor rel-L2 of the older tests stayed at 3e-4 .. 4e-4."""
    k = mc.k_values(t)[ki]
    n, over = 0, []
    for case in mc.DEFAULT_CASES:
        worst = (0.0, "-")
        for name, gen in mc.patterns(case, t):
            ids = mc.make_ids(case, t, name, gen)
            ne11 = (1, case.n_used)[n % 2]
            n += 1
            got = run_case(qmm, t, case, k, dev(ids), ne11).cpu().numpy()
            err = row_rel_l2(got, reference(oracle, t, case, k, name, ids, ne11))
            worst = max(worst, (float(err.max()), name))
            if not err.max() < MFMA_BAR:                     # every case runs; the assertion below names all that miss the bar
                over.append((case.name, name, ne11, float(err.max()), np.argwhere(err >= MFMA_BAR)[:4].tolist()))
        print(f"a | {TYPE_NAMES[t]} | {case.name} | K={k} | {mc.label_of(case, t)} | {mc.prep_label_of(case, t, k)} | {worst[0]:.3e} | {worst[1]}")
    qmm.synchronize()
    assert not over, (TYPE_NAMES[t], k, over)


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_strided_views(qmm, oracle, t):
    """b with a row pitch above K, ids as a column slice of a wider tensor, out with M + 12 columns: the guard columns keep the sentinel"""
    case = mc.DEFAULT_CASES[4]
    k = mc.k_values(t)[0]
    name, gen = mc.patterns(case, t)[-1]
    ids = mc.make_ids(case, t, name, gen)
    ne11 = case.n_used
    _, wd = expert_weights(t, case.M, case.n_expert, k)
    b, bd = activations(t, case.n_tokens, ne11, k)
    b_big = torch.full((case.n_tokens, ne11, k + 64), 9.0, device="cuda")
    b_big[:, :, :k] = bd
    ids_big = torch.full((case.n_tokens, case.n_used + 3), -7, dtype=torch.int32, device="cuda")
    ids_big[:, :case.n_used] = dev(ids)
    out = torch.full((case.n_tokens, case.n_used, case.M + 12), SENTINEL, device="cuda")
    labels = qmm.trace(lambda: qmm.mul_mat_id(t, wd, k, b_big[:, :, :k], ids_big[:, :case.n_used], out=out[:, :, :case.M]))
    if pins_hold():
        assert labels == mc.labels_of(case, t, k)
    o = out.cpu().numpy()
    assert (o[:, :, case.M:] == SENTINEL).all()
    err = row_rel_l2(o[:, :, :case.M], reference(oracle, t, case, k, name, ids, ne11))
    assert err.max() < MFMA_BAR, (TYPE_NAMES[t], float(err.max()))
    qmm.synchronize()


# ---- b. routing invariance and f. determinism, bit-exact

@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_a_pairs_product_does_not_depend_on_its_place_in_the_segment(qmm, t):
    """the plan depends on (type, M, K, P, n_expert) alone, and a pair's row of the product on its expert and its activations alone: a
    permutation of the tokens (b and ids together) gives the un-permuted outputs, permuted, bit for bit"""
    for case in mc.DEFAULT_CASES:
        if case.n_expert < 3:
            continue
        k = mc.k_values(t)[case.n_tokens % 2]
        ne11 = case.n_used
        _, wd = expert_weights(t, case.M, case.n_expert, k)
        _, bd = activations(t, case.n_tokens, ne11, k)
        for name, gen in mc.patterns(case, t):
            if not name.startswith("edge"):
                continue
            ids = mc.make_ids(case, t, name, gen)
            first = run_case(qmm, t, case, k, dev(ids), ne11)
            perm = np.random.default_rng(case.n_tokens).permutation(case.n_tokens)
            pd = dev(perm)
            out = torch.full_like(first, SENTINEL)
            qmm.mul_mat_id(t, wd, k, bd[pd].contiguous(), dev(ids[perm]), out=out)
            assert torch.equal(out.view(torch.int32), first[pd].view(torch.int32)), (TYPE_NAMES[t], case.name, k, name)
    qmm.synchronize()


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_second_run_is_bit_identical(qmm, t):
    for case in mc.DEFAULT_CASES:
        if case.n_expert < 3:
            continue
        k = mc.k_values(t)[1 - case.n_tokens % 2]
        for name, gen in mc.patterns(case, t):
            if not name.startswith("edge"):
                continue
            ids_d = dev(mc.make_ids(case, t, name, gen))
            first = run_case(qmm, t, case, k, ids_d, 1)
            again = run_case(qmm, t, case, k, ids_d, 1)
            assert torch.equal(first.view(torch.int32), again.view(torch.int32)), (TYPE_NAMES[t], case.name, k, name)
            assert not (first == SENTINEL).any()
    qmm.synchronize()


# ---- c. a bad id in a prompt batch

@pytest.mark.parametrize("t", (Q4_K, Q8_0, Q4_1), ids=["q4_K", "q8_0", "q4_1"])       # (Q4_1: the launches behind the MFMA kernel see the bad pairs too)
def test_bad_ids_in_a_prompt_batch_are_reported_and_their_rows_left_alone(qmm, oracle, t):
    """one pair names n_expert, one names -1: the call returns, the next synchronize raises (the library's own report, not a GPU fault), the
    one after is clean; the two pairs' rows keep the sentinel and every other row meets the bar"""
    from ggml_hexagon_amd.capi import QmmError
    case = mc.BAD_ID_CASE
    k = mc.k_values(t)[1]
    ids = mc.make_ids(case, t, "uniform", mc.uniform)
    good = ids.copy()
    bad = ((3, 1), (77, 0))
    ids[bad[0]] = case.n_expert
    ids[bad[1]] = -1
    qmm.synchronize()
    got = run_case(qmm, t, case, k, dev(ids), case.n_used).cpu().numpy()
    with pytest.raises(QmmError):
        qmm.synchronize()
    qmm.synchronize()
    for tok, slot in bad:
        assert (got[tok, slot] == SENTINEL).all()
    err = row_rel_l2(got, reference(oracle, t, case, k, "uniform", good, case.n_used))
    for tok, slot in bad:
        err[tok, slot] = 0.0
    assert not (got == SENTINEL)[err > 0].any() and err.max() < MFMA_BAR, (TYPE_NAMES[t], float(err.max()))


# ---- the pair call at prompt size

@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_pair_call_at_prompt_size_per_row(qmm, oracle, t):
    """mul_mat_id_pair (ffn_gate_exps + ffn_up_exps: one sort, one prep, two MFMA launches) beyond 16 pairs, on a skinny and a tiled case with
    edge routing: both tensors per (token, slot) row against the oracle and bit-equal to their single calls; launches as pinned"""
    for case in (mc.DEFAULT_CASES[2], mc.DEFAULT_CASES[5]):
        k = mc.k_values(t)[1]
        name, gen = mc.patterns(case, t)[-1]
        assert name.startswith("edge")
        ids = mc.make_ids(case, t, name, gen)
        ids_d = dev(ids)
        ne11 = case.n_used
        ws = [expert_weights(t, case.M, case.n_expert, k, seed=s) for s in (0, 3)]
        b, bd = activations(t, case.n_tokens, ne11, k)
        outs = [torch.full((case.n_tokens, case.n_used, case.M), SENTINEL, device="cuda") for _ in range(2)]
        labels = qmm.trace(lambda: qmm.mul_mat_id_pair(t, ws[0][1], ws[1][1], k, bd, ids_d, outs[0], outs[1]))
        if pins_hold():
            assert labels == mc.pair_labels_of(case, t, k), (case.name, TYPE_NAMES[t], labels)
        for (w, wd), o in zip(ws, outs):
            err = row_rel_l2(o.cpu().numpy(), oracle.mul_mat_id(t, w, k, case.M, b, ids, ACT_REF))
            print(f"p | {TYPE_NAMES[t]} | {case.name} | K={k} | {mc.label_of(case, t)} | pair call | {float(err.max()):.3e} | {name}")
            assert err.max() < MFMA_BAR, (TYPE_NAMES[t], case.name, float(err.max()))
            single = torch.full_like(o, SENTINEL)
            qmm.mul_mat_id(t, wd, k, bd, ids_d, out=single)
            assert torch.equal(o.view(torch.int32), single.view(torch.int32)), (TYPE_NAMES[t], case.name)
    qmm.synchronize()


# ---- d. the few-pair kernels past one wave of units

@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_few_pairs_second_slice(qmm, oracle, t):
    """matvec_id_kernel (one tensor, and two in one launch) and matvec_id_swiglu_kernel at K = 4352: 68 or 136 units, so the loop over
    u += WAVE runs with a partially filled slice (the 64-wide units again at K = 8448: 132 units, a third slice, where a wrong stride
    shows); M = 41 ragged against the 8 waves, M = 300 with the row loop iterating; repeated experts.
    Single and pair: max|err| / rms < 2e-5 against the oracle; the pair bit-equal to two single calls.  SwiGLU: silu(g) * u formed in
    float64 from the oracle's two products, max|err| / rms(want) < SWIGLU_BAR = 4 x the worst value measured on the kernel before this
    test existed."""
    for n, (k, fc) in enumerate(mc.few_k_cases(t)):
        ids = mc.few_ids(fc)
        ne11 = (1, fc.n_used)[n % 2]
        (w0, w0d), (w1, w1d) = expert_weights(t, fc.M, fc.n_expert, k, seed=1), expert_weights(t, fc.M, fc.n_expert, k, seed=2)
        b, bd = activations(t, fc.n_tokens, ne11, k)
        ids_d = dev(ids)
        shape = (fc.n_tokens, fc.n_used, fc.M)
        single = [torch.full(shape, SENTINEL, device="cuda") for _ in range(2)]
        pair = [torch.full(shape, SENTINEL, device="cuda") for _ in range(2)]
        fused = torch.full(shape, SENTINEL, device="cuda")
        labels = qmm.trace(lambda: (qmm.mul_mat_id(t, w0d, k, bd, ids_d, out=single[0]), qmm.mul_mat_id(t, w1d, k, bd, ids_d, out=single[1]),
                                    qmm.mul_mat_id_pair(t, w0d, w1d, k, bd, ids_d, pair[0], pair[1]), qmm.mul_mat_id_swiglu(t, w0d, w1d, k, bd, ids_d, fused)))
        assert labels == (f"matvec_id_kernel<{t}>",) * 3 + (f"matvec_id_swiglu_kernel<{t}>",), labels
        want = [oracle.mul_mat_id(t, w, k, fc.M, b, ids, ACT_REF) for w in (w0, w1)]
        errs = [rel_rms(single[i].cpu().numpy(), want[i]) for i in range(2)]
        g, u = want[0].astype(np.float64), want[1].astype(np.float64)
        swi = rel_rms(fused.cpu().numpy(), g / (1.0 + np.exp(-g)) * u)
        print(f"d | {TYPE_NAMES[t]} | K={k} M={fc.M} tokens={fc.n_tokens} used={fc.n_used} ne11={ne11} {fc.pattern} | matvec_id_kernel<{t}> | {max(errs):.3e} | "
              f"matvec_id_swiglu_kernel<{t}> | {swi:.3e}")
        for i in range(2):
            assert errs[i] < MATVEC_BAR, (TYPE_NAMES[t], fc, i, errs[i])
            assert torch.equal(pair[i].view(torch.int32), single[i].view(torch.int32)), (TYPE_NAMES[t], fc, i)
        assert swi < SWIGLU_BAR, (TYPE_NAMES[t], fc, swi)
    qmm.synchronize()


# ---- e. other modes

@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_bf16_precision_lds_tile_kernel_with_segments(qmm, oracle, t):
    """QMM_PREC_BF16: mfma_kernel<t,64> and <t,128> with segments, one-hot and edge routing; NMSE < 5e-4 per row"""
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8
    qmm.set_precision(PREC_BF16)
    try:
        n, over = 0, []
        for case in mc.LDS_CASES:
            for k in mc.k_values(t):
                worst = (0.0, "-")
                for name, gen in mc.patterns(case, t):
                    if name == "uniform":
                        continue
                    ids = mc.make_ids(case, t, name, gen)
                    ne11 = (1, case.n_used)[n % 2]
                    n += 1
                    got = run_case(qmm, t, case, k, dev(ids), ne11, f16=False).cpu().numpy()
                    err = row_rel_l2(got, reference(oracle, t, case, k, name, ids, ne11)) ** 2
                    worst = max(worst, (float(err.max()), name))
                    if not err.max() < BF16_BAR:
                        over.append((case.name, k, name, ne11, float(err.max())))
                print(f"e | {TYPE_NAMES[t]} | {case.name} | K={k} | {mc.label_of(case, t)} | bf16 | NMSE {worst[0]:.3e} | {worst[1]}")
        qmm.synchronize()
        assert not over, (TYPE_NAMES[t], over)
    finally:
        qmm.set_precision(PREC_F16_Q8)


@pytest.mark.parametrize("t", (Q2_K, Q3_K), ids=["q2_K", "q3_K"])
def test_regb_q23_off_lds_tile_kernel_with_segments_in_f16(qmm_q23_off, oracle, t):
    """GGML_MI355X_REGB_Q23=0: Q2_K / Q3_K prompt batches run mfma_kernel with segments in the default precision"""
    q = qmm_q23_off
    for case in mc.LDS_CASES:
        for k in mc.k_values(t):
            worst = (0.0, "-")
            for name, gen in mc.patterns(case, t):
                ids = mc.make_ids(case, t, name, gen)
                got = run_case(q, t, case, k, dev(ids), case.n_used, regb_q23=False).cpu().numpy()
                err = row_rel_l2(got, reference(oracle, t, case, k, name, ids, case.n_used))
                worst = max(worst, (float(err.max()), name))
                assert err.max() < MFMA_BAR, (TYPE_NAMES[t], case.name, k, name, float(err.max()))
            print(f"e | {TYPE_NAMES[t]} | {case.name} | K={k} | {mc.label_of(case, t)} | f16, REGB_Q23=0 | {worst[0]:.3e} | {worst[1]}")
    q.synchronize()
