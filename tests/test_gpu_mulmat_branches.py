"""Plain MUL_MAT prompt batches through every branch of the prefill plan and every class of split-K range, per token row AND per weight row
(the case table: tests/mulmat_cases.py; the launch plan of every case is pinned without a GPU in test_mulmat_plan_host.py, and asserted here
through qmm.trace on a 256-CU device).  Every output is a strided view (ldd = M + 12) into a sentinel-filled buffer whose guard columns must
keep the sentinel.

Two references, both computed on the CPU from the same operands:
  * exact:  the float64 product of the quantized operands: oracle.dequantize of the weights, and d * q of the wire blocks the oracle's own
    quantize_act makes of the activations (Q8_0 / Q8_1 / Q8_K).  This is the operation the kernels implement; they depart from it only by the
    f16 rounding of the weights and f32 accumulation.
  * oracle: oracle.mul_mat, the CPU backend's arithmetic.
Bars, for every row of either axis of the [N, M] output: one wrong token row, or one wrong weight row at a tile edge, must not hide in a tensor
  * default precision: rel-L2 < 1e-3 against exact (the project's MFMA bar; test_gpu_moe_routing.py uses it per row too), and < 1e-3 against
    the oracle, which is within 3e-7 of exact per row for ten of the twelve types.  Q4_1 / Q5_1: the CPU multiplies the block minimum with
    s = f16(d * sum), plain MUL_MAT prefill carries the minimum inside the f16 weights (MUL_MAT_ID has a correction launch for it, plain
    MUL_MAT deliberately not), so the oracle itself is up to 1.54e-3 from exact on a token row of the cases here (Q5_1, 100 tokens x 8224
    rows, K = 1056); there the bar against the oracle is 1e-3 + that row's own oracle-to-exact distance (the triangle inequality; both
    terms come from the references alone);
  * QMM_PREC_BF16: NMSE < 5e-4 against exact, the reference's own bar.
The row closest to its bar is a weight row of 32 samples: Q4_K, mfma_skinny_kernel<12,8,1>, M = 300, K = 768, N = 32, weight row 3 at 9.18e-4.
That is the row, not the kernel: the float64 product of the same operands with every weight and every scaled activation rounded to f16 ONCE
has its worst weight row there too (5.0e-4 against a median of 2.6e-4; the row's 32 outputs are small, rms 7.9 against 11.5), and the
Q4_K kernels, which form d * sc * q - dmin * m in f16, sit 1.8 - 2.1 x above that single rounding on every row and label.
Run with -s to see the measured figures (profiles/mulmat_branch_errors.txt is that output behind the summary of
profiles/tools/mulmat_branch_summary.py)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import mulmat_cases as mm  # noqa: E402
from oracle.pyoracle import ACT_REF, Q4_1, Q4_K, Q5_1, Q8_0, Q8_1, Q8_K, TYPE_NAMES, WEIGHT_TYPES, vec_dot_type  # noqa: E402

IDS = [TYPE_NAMES[t] for t in WEIGHT_TYPES]
SENTINEL = 777.0
GUARD = 12
MFMA_BAR, BF16_BAR = 1e-3, 5e-4
CPU_MIN_TYPES = (Q4_1, Q5_1)                 # the oracle's f16(d * sum) against the minimum carried in the f16 weights


@pytest.fixture(scope="module")
def contexts():
    """name -> context, created on first use with the environment switches of mulmat_cases.CONTEXTS (the library reads them when a context is
    created, as tests/test_gpu_full_size.py::_contexts relies on); QMM_PREC_BF16 is a mode of the default context"""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    made = {}
    prop = torch.cuda.get_device_properties(0)
    print(f"\n# {prop.name}, {prop.multi_processor_count} CUs: labels {'asserted' if pins_hold() else 'NOT asserted (the pins are for %d CUs)' % mm.CUS}")

    def get(name):
        env = mm.CONTEXTS[name][0]
        key = tuple(sorted(env.items()))
        if key not in made:
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                made[key] = Qmm(0)      # raises if the HIP library is missing or the device is not gfx950: no fallback
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
        return made[key]
    yield get
    for q in made.values():
        q.close()
    _made.clear()                       # the last type's operands and references


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pins_hold():
    """the labels of mulmat_cases are pinned for a 256-CU device; elsewhere only the label assertions are left out, never a parity check"""
    return torch.cuda.get_device_properties(0).multi_processor_count == mm.CUS


def rel_l2_rows(got, want, axis):
    """rel-L2 of every row along `axis` (1: per token row, 0: per weight row); want is float64"""
    return np.sqrt(np.sum((got - want) ** 2, axis=axis) / np.maximum(np.sum(want ** 2, axis=axis), 1e-30))


# ---- operands and references: made once per (type, shape), shared by the tests of a type, never written to

_made = {"type": None}


def _cache(t):
    if _made["type"] != t:
        _made.clear()
        _made["type"] = t
    return _made


def weights(t, m, k, seed=0):
    import ggml_hexagon_amd.synth as synth
    c, key = _cache(t), ("w", m, k, seed)
    if key not in c:
        w = synth.synth_weights(t, m, k, seed=1000 * seed + m + k, sigma=0.25)
        c[key] = (w, dev(w))
    return c[key]


def activations(t, n, k):
    c, key = _cache(t), ("x", n, k)
    if key not in c:
        x = np.random.default_rng(n * 7 + k).uniform(-1, 1, (n, k)).astype(np.float32)
        c[key] = (x, dev(x))
    return c[key]


def quantized_activations(oracle, t, x):
    """d * q of the oracle's wire blocks of x, float64 [N, K]: block_q8_0 = f16 d, 32 x int8; block_q8_1 = f16 d, f16 s, 32 x int8;
    block_q8_K = f32 d, 256 x int8, 16 x int16 sums"""
    n, k = x.shape
    vt = vec_dot_type(t)
    nq, head, size, dt = {Q8_0: (32, 2, 34, np.float16), Q8_1: (32, 4, 36, np.float16), Q8_K: (256, 4, 292, np.float32)}[vt]
    raw = oracle.quantize_act(t, x, ACT_REF)
    assert raw.shape == (n, k // nq * size)
    blk = raw.reshape(n, k // nq, size)
    d = np.ascontiguousarray(blk[:, :, :dt().itemsize]).view(dt).astype(np.float64)
    q = np.ascontiguousarray(blk[:, :, head:head + nq]).view(np.int8).astype(np.float64)
    return (d * q).reshape(n, k)


def references(oracle, t, m, k, n, seed=0):
    """(exact, oracle) of one matrix, float64 [N, M] each"""
    c, key = _cache(t), ("ref", m, k, n, seed)
    if key not in c:
        w, _ = weights(t, m, k, seed)
        x, _ = activations(t, n, k)
        exact = quantized_activations(oracle, t, x) @ oracle.dequantize(t, w, k).astype(np.float64).T
        c[key] = (exact, oracle.mul_mat(t, w, k, x, ACT_REF).astype(np.float64))
    return c[key]


# ---- one case: the call, the labels, the guard columns, both axes against both references

def call(q, t, case, wds, xd, outs):
    views = [o[:, :m] for o, m in zip(outs, case.Ms)]
    if len(wds) == 1:
        q.mul_mat(t, wds[0], case.K, xd, out=views[0])
    else:
        q.mul_mat_group([(t, w) for w in wds], case.K, xd, views)


def dirty_workspace(q, t, case, xd):
    """in front of a case with an empty or a past-the-end range: a larger split-K launch in the same context whose slab 0 (partial sums of a
    range with work) lies over all slabs of the case (mulmat_cases.dirty_rows), so that a slab the case fails to zero is caught whichever
    cases ran before, or none"""
    _, wd = weights(t, mm.dirty_rows(case), case.K, seed=9)
    labels = q.trace(lambda: q.mul_mat(t, wd, case.K, xd))
    if pins_hold():
        assert any(l == "splitk_reduce_kernel" or l.endswith("+combine") for l in labels), (TYPE_NAMES[t], case.name, labels)


def run_case(q, t, case, wds, xd):
    """the case's call into sentinel-filled buffers of M + 12 columns, `repeat` times into re-filled buffers (every run the bits of the
    first); the traced labels of the first run are the case's pins.  Returns the outputs [N, M] as numpy arrays"""
    outs = [torch.full((case.N, m + GUARD), SENTINEL, device="cuda") for m in case.Ms]
    labels = q.trace(lambda: call(q, t, case, wds, xd, outs))
    if pins_hold():
        assert labels == mm.labels_of(case, t), (TYPE_NAMES[t], case.name, labels)
    first = [o.clone() for o in outs]
    for _ in range(case.repeat - 1):
        for o in outs:
            o.fill_(SENTINEL)
        call(q, t, case, wds, xd, outs)
        for o, f in zip(outs, first):
            assert torch.equal(o.view(torch.int32), f.view(torch.int32)), (TYPE_NAMES[t], case.name, "a repeated run differs")
    got = []
    for o, m in zip(outs, case.Ms):
        a = o.cpu().numpy()
        assert (a[:, m:] == SENTINEL).all(), (TYPE_NAMES[t], case.name, "guard columns written")
        assert not (a[:, :m] == SENTINEL).any(), (TYPE_NAMES[t], case.name, "outputs left unwritten", np.argwhere(a[:, :m] == SENTINEL)[:4].tolist())
        got.append(a[:, :m].astype(np.float64))
    return got


def check(t, case, got, refs, over):
    """one printed line per (type, case, matrix), and every row of either axis over its bar appended to `over`"""
    bf16 = mm.CONTEXTS[case.ctx][2]
    for i, (g, (exact, orc)) in enumerate(zip(got, refs)):
        launch = [l for l in case.launches if l.first <= i < l.first + l.n][0]
        fig = {}
        for axis, what in ((1, "token"), (0, "weight")):
            e, o, d = rel_l2_rows(g, exact, axis), rel_l2_rows(g, orc, axis), rel_l2_rows(exact, orc, axis)
            if bf16:
                e, o = e ** 2, o ** 2
                bad = np.flatnonzero(~(e < BF16_BAR))
            else:
                bad = np.flatnonzero(~((e < MFMA_BAR) & (o < MFMA_BAR + (d if t in CPU_MIN_TYPES else 0.0))))
            # the references themselves: apart from the two types above the oracle differs from exact by its f32 sum of K / 32 <= 140 block
            # terms alone, 6e-8 * sqrt(140) = 7e-7 (measured on the CPU: <= 3.1e-7)
            assert t in CPU_MIN_TYPES or d.max() < 1e-6, (TYPE_NAMES[t], case.name, what, float(d.max()))
            fig[what] = (float(e.max()), int(e.argmax()), float(o.max()), int(o.argmax()), float(d.max()))
            if len(bad):
                over.append((case.name, i, what + " rows", [(int(j), float(e[j]), float(o[j])) for j in bad[:4]], len(bad)))
        (te, ta, to, toa, td), (we, wa, wo, woa, wd) = fig["token"], fig["weight"]
        print(f"{case.section} | {TYPE_NAMES[t]} | {case.name} | M={case.Ms[i]} K={case.K} N={case.N} | {mm.label_of(launch, t)} | {case.ctx} | "
              f"ranges {'-' if case.ranges is None else ','.join(map(str, case.ranges))} {mm.range_class(case.ranges) or '-'} | "
              f"{'NMSE' if bf16 else 'rel-L2'} exact: token row {te:.3e} @{ta}, weight row {we:.3e} @{wa} | oracle: token row {to:.3e} @{toa}, weight row {wo:.3e} @{woa} | "
              f"oracle-to-exact: token row {td:.3e}, weight row {wd:.3e}")


def run_section(contexts, oracle, t, sections):
    from ggml_hexagon_amd.capi import PREC_BF16, PREC_F16_Q8
    over = []
    for case in mm.cases(t):
        if case.section not in sections:
            continue
        q = contexts(case.ctx)
        ws = [weights(t, m, case.K, seed=i) for i, m in enumerate(case.Ms)]
        _, xd = activations(t, case.N, case.K)
        bf16 = mm.CONTEXTS[case.ctx][2]
        if bf16:
            q.set_precision(PREC_BF16)
        try:
            if mm.dirty_rows(case):
                dirty_workspace(q, t, case, xd)
            got = run_case(q, t, case, [wd for _, wd in ws], xd)
            q.synchronize()
        finally:
            if bf16:
                q.set_precision(PREC_F16_Q8)
        check(t, case, got, [references(oracle, t, m, case.K, case.N, seed=i) for i, m in enumerate(case.Ms)], over)
    assert not over, (TYPE_NAMES[t], over)


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_tile_variants_per_row(contexts, oracle, t):
    """a. without split-K: mfma_regb_kernel<t,4,32>, <t,4,64> and <t,4,128> (the 128-wide units: <t,4,64> on the grid that would be <t,4,128>),
    the 65..128-token band that the few-token kernel declines (<t,8,128>, two ranges), mfma_skinny_kernel<t,8,1> and <t,8,2> at 32 / 64 / 128
    tokens; K = 736 pads the operand row (Kp = 768)"""
    run_section(contexts, oracle, t, "a")


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_splitk_range_classes_per_row(contexts, oracle, t):
    """b, c. mfma_regb_kernel<t,8,128> with K cut 2 .. 8 ways: even ranges, a ragged last range, an empty last range (a slab of zeros for
    splitk_reduce_kernel) and ranges that begin past the end of K (clamped loads); M = 300 takes the float4 reduce, M = 253 the scalar one;
    K = 1024 / 2048 take the register-resident prep"""
    run_section(contexts, oracle, t, "b")


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_groups_per_row(contexts, oracle, t):
    """d. three matrices of 300, 70 and 257 rows as one <t,8,128> launch of 5 row tiles with four K ranges and one reduce over mtot = 627
    columns; two matrices at K = 736 as two launches on one prep"""
    run_section(contexts, oracle, t, "d")


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_splitk_combined_in_the_launch_per_row(contexts, oracle, t):
    """e. GGML_MI355X_SPLITK_COMBINE=1: splitk_finish_wave instead of the reduce kernel, one matrix and a group of three, four runs each into
    re-filled outputs: a wave whose range is empty (Q4_K and the 128-wide units at K = 2304) must still store its zeros and bump the
    arrival counter, and the counters must be back at zero for the next run"""
    run_section(contexts, oracle, t, "e")


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=IDS)
def test_bf16_precision_per_row(contexts, oracle, t):
    """g. QMM_PREC_BF16: mfma_kernel<t,64> and <t,128> on a plain MUL_MAT; NMSE < 5e-4 per row of either axis"""
    run_section(contexts, oracle, t, "g")


def test_q4k_r64_kernel_range_classes_per_row(contexts, oracle):
    """f. GGML_MI355X_R64=1: the split-K cases of (b) and the group of (d) through mfma_r64_q4k_kernel<4>"""
    run_section(contexts, oracle, Q4_K, "f")


WIDE_ROWS = 7100                             # the wide cases cut their matrices from one set of rows: 7000 alone, 3500 + 3600 as a pair


@pytest.mark.parametrize("ctx", ["r64=0", "default", "r64s=0"])
def test_q4k_wide_tiles_per_row(contexts, oracle, ctx):
    """f. 256-token tiles at M = 7000, K = 512, N = 1950 (28 x 8 tiles, ragged rows and ragged tokens): mfma_regb_q4k_wide_kernel<8>
    (GGML_MI355X_R64=0), mfma_r64s_q4k_kernel<2> (default) and mfma_r64_q4k_kernel<8> (GGML_MI355X_R64S=0), and the same rows as two
    matrices of 3500 and 3600 in one launch of 29 row tiles.  Every token row on every weight row: both references over all 7100 rows
    take about 3 s on the CPU, once for the three contexts"""
    t, k, n = Q4_K, 512, 1950
    _, wd = weights(t, WIDE_ROWS, k)
    _, xd = activations(t, n, k)
    exact, orc = references(oracle, t, WIDE_ROWS, k, n)
    over, seen = [], 0
    for case in mm.cases(t):
        if case.section != "w" or case.ctx != ctx:
            continue
        assert (case.K, case.N) == (k, n) and sum(case.Ms) in (7000, WIDE_ROWS)
        q = contexts(case.ctx)
        first = np.cumsum((0,) + case.Ms[:-1])
        got = run_case(q, t, case, [wd[f:f + m] for f, m in zip(first, case.Ms)], xd)
        q.synchronize()
        check(t, case, got, [(exact[:, f:f + m], orc[:, f:f + m]) for f, m in zip(first, case.Ms)], over)
        seen += 1
    assert seen == 2 and not over, over
