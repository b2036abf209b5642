"""The folds of qmm_mul_mat_group_ex at N <= 8 (the RMS norm formed while staging, the SwiGLU of a gate / up pair, the residual added in the
epilogue) for all 23 weight type codes, on every staging path and workgroup geometry: the case table tests/matvec_fold_cases.py, whose launch
plans test_matvec_fold_host.py pins without a GPU; the traced labels are asserted against those pins in every case (a label carries no
geometry: block size and grid are pinned on the host side, for the 256 CUs the fixture reports).

References.  The C oracle (Oracle.mul_mat, ACT_REF) for its 12 types (planar rows are the same wire rows, repacked on the device);
tq_refs.mul_mat_np and iq{1,2,3}_refs.mul_mat_np for the others, fed the oracle's own Q8_K blocks; the codebook types take their grids from
the live reference as their own test files do and are skipped, type by type, where oracle/_ref is not built.  With a norm the references are
fed the numpy-normed row (helpers.rms_norm_f32); SwiGLU and the residual add are float64 numpy.

Inputs of every norm case are rounding-stable rows (helpers.rounding_stable_rows): their normed elements keep clear of every rounding boundary
of the activation quantizer, so the kernel's f32 norm and numpy's, which differ in the last bit here and there, hand the same int8 values
and block scales to the dot products, and every norm case is held to the mat-vec bar itself.

Bars, none of them new: products and residual sums max |err| / rms(want) <= 2e-5 (test_gpu_parity.py); SwiGLU: swiglu_bar of
test_gpu_iq1.py; the geometry and one-pass comparisons, the outputs of an all-zero row and the guard columns: exact.  Run with -s for one
line per launch and, behind them, one `folds ==` line per test (profiles/matvec_fold_errors.txt holds those: the full output is
some 2000 lines)."""
import os
import zlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import helpers as H  # noqa: E402
import iq1_refs  # noqa: E402
import iq2_refs  # noqa: E402
import iq3_refs  # noqa: E402
import matvec_fold_cases as F  # noqa: E402
import tq_refs  # noqa: E402
from oracle.pyoracle import ACT_REF, WEIGHT_TYPES, ref_available  # noqa: E402
from test_gpu_iq1 import swiglu_bar  # noqa: E402

BAR = 2e-5
SENTINEL = -77.25
GUARD = 24
MV_SLOTS = 4                                 # qmm_mv_extra.residual[]
EPS = 1e-5
NP_REFS = {F.TQ1_0: tq_refs, F.TQ2_0: tq_refs, F.IQ3_XXS: iq3_refs, F.IQ3_S: iq3_refs, F.IQ2_XS: iq2_refs, F.IQ2_S: iq2_refs,
           F.IQ1_S: iq1_refs, F.IQ1_M: iq1_refs}
HAVE_REF = ref_available()
no_ref = pytest.mark.skipif(not HAVE_REF, reason="oracle/_ref not built: no grid for this codebook type (run `make -C oracle ref`)")


def param(t, *more):
    """one parametrized type (with further values): a codebook type is skipped, visibly, where the live reference is not built"""
    return pytest.param(t, *more, id="-".join([F.NAMES.get(t, str(t))] + [str(m) for m in more]), marks=[no_ref] if t in F.CODEBOOK_TYPES else [])


# ------------------------------------------------------------------------------------------------- references and contexts

class Refs:
    """the CPU references; the grids of the codebook types come from the live reference where it is built"""

    def __init__(self):
        from oracle.pyoracle import Oracle
        self.oracle = Oracle()
        self.grids = {}
        if HAVE_REF:
            r3, r2, r1 = iq3_refs.Iq3Ref(), iq2_refs.Iq2Ref(), iq1_refs.Iq1Ref()
            self.grids = {F.IQ3_XXS: r3.codebook(F.IQ3_XXS), F.IQ3_S: r3.codebook(F.IQ3_S), F.IQ2_XS: r2.codebook(F.IQ2_XS),
                          F.IQ2_S: r2.codebook(F.IQ2_S), F.IQ1_S: r1.codebook(F.IQ1_S)}
            self.grids[F.IQ1_M] = self.grids[F.IQ1_S]
        self._products = {}

    def product(self, key, t, w, k, x):
        """W x of wire rows w [m, row bytes] of type code t and f32 rows x [n, k] (normed already, where a norm is folded): float64 [n, m];
        computed once per key"""
        if key not in self._products:
            tb = F.base(t)
            if tb in WEIGHT_TYPES:
                p = self.oracle.mul_mat(tb, w, k, x, ACT_REF)
            else:
                acts = self.oracle.quantize_act(F.Q4_K, x)                   # the Q8_K blocks of the rows
                p = NP_REFS[tb].mul_mat_np(tb, w, k, acts, *([self.grids[tb]] if tb in F.CODEBOOK_TYPES else []))
            p = p.astype(np.float64)
            p.setflags(write=False)
            self._products[key] = p
        return self._products[key]

    def forget(self):
        self._products.clear()


@pytest.fixture(scope="module")
def refs():
    return Refs()


@pytest.fixture(scope="module")
def contexts(refs):
    """name -> context, created on first use under the environment of matvec_fold_cases.CONTEXTS (the library reads its switches when a
    context is created, as test_gpu_mulmat_branches.py::contexts relies on); every context gets the codebooks"""
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    from ggml_hexagon_amd.capi import Qmm
    made = {}
    prop = torch.cuda.get_device_properties(0)
    print(f"\n# {prop.name}, {prop.multi_processor_count} CUs: the host pins of block size and grid are for {F.CUS} CUs"
          f"{'' if prop.multi_processor_count == F.CUS else ' (NOT this device: the geometry cases run, their geometry differs)'}")

    def get(name):
        if name not in made:
            env = F.CONTEXTS[name][0]
            old = {k: os.environ.get(k) for k in env}
            os.environ.update(env)
            try:
                q = Qmm(0)                  # raises if the HIP library is missing or the device is not gfx950: no fallback
            finally:
                for k, v in old.items():
                    if v is None:
                        os.environ.pop(k, None)
                    else:
                        os.environ[k] = v
            for t in (F.IQ3_XXS, F.IQ3_S, F.IQ2_XS, F.IQ2_S, F.IQ1_S):
                if t in refs.grids:
                    q.set_codebook(t, refs.grids[t])
            made[name] = q
        return made[name]
    yield get
    for q in made.values():
        q.close()
    _np.clear()
    _dev.clear()
    refs.forget()


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()                    # (a copy: the cached operands are read-only)


def rms(a):
    return max(float(np.sqrt(np.mean(np.asarray(a, np.float64) ** 2))), 1e-30)


# ------------------------------------------------------------------------------------------------- operands: made once, never written to

_np, _dev = {}, {}


def weights(t, m, k, seed):
    """wire rows of the base type of t, [m, row bytes]"""
    import ggml_hexagon_amd.synth as synth
    key = ("w", F.base(t), m, k, seed)
    if key not in _np:
        w = synth.synth_weights(F.base(t), m, k, seed=seed, sigma=0.25)
        w.setflags(write=False)
        _np[key] = w
    return _np[key]


def on_device(q, t, w, k, wkey):
    """(type code, device rows) of wire rows w, repacked in place for a planar code; once per (context, key)"""
    key = (id(q), t, wkey)
    if key not in _dev:
        wd = dev(w)
        if F.planar(t):
            assert q.repack_rows(F.base(t), wd, k) == t
        _dev[key] = (t, wd)
        if len(_dev) > 64:
            _dev.pop(next(iter(_dev)))
    return _dev[key]


def norm_weight(k):
    key = ("nw", k)
    if key not in _np:
        _np[key] = np.random.default_rng(k).normal(1, 0.1, k).astype(np.float32)
    return _np[key]


def inputs(fmt, k, norm):
    """8 token rows of K: N(0, 1); with a norm, rounding-stable for the activation format under norm_weight(k) and EPS"""
    key = ("x", fmt if norm else None, k)
    if key not in _np:
        if norm:
            x, redraws = H.rounding_stable_rows(fmt, F.MV_MAX_N, k, norm_weight(k), EPS, seed=1000 * fmt + k)
            print(f"folds | rounding-stable rows, activation format {fmt}, K={k}: redraws per row {redraws.tolist()}")
        else:
            x = np.random.default_rng(7000 + k).normal(0, 1, (F.MV_MAX_N, k)).astype(np.float32)
        x.setflags(write=False)
        _np[key] = x
    return _np[key]


def case_inputs(case):
    """the token rows of a case: stable for every activation format among its matrices (a mixed-format group with a norm stages both)"""
    fmts = sorted({F.act(t) for t in case.types})
    if case.norm and len(fmts) > 1:
        key = ("x2", tuple(fmts), case.K)
        if key not in _np:
            nw = norm_weight(case.K)
            rng = np.random.default_rng(31 + case.K)
            rows = []
            while len(rows) < F.MV_MAX_N:
                row = rng.normal(0, 1, case.K).astype(np.float32)
                if all(H.rounding_stable(f, H.rms_norm_f64(row, nw, EPS)) for f in fmts):
                    rows.append(row)
            _np[key] = np.stack(rows)
        return _np[key][:case.N]
    return inputs(fmts[0], case.K, case.norm)[:case.N]


def residual(case, i):
    key = ("res", case.N, case.Ms[i], i)
    if key not in _np:
        _np[key] = np.random.default_rng(100 * case.N + case.Ms[i] + i).normal(0, 1, (case.N, case.Ms[i])).astype(np.float32)
    return _np[key]


def case_weights(case, seed0=11):
    """(wire rows, key) per matrix: seeds by place in the call"""
    return [(weights(t, m, case.K, seed0 + i), (F.base(t), m, case.K, seed0 + i)) for i, (t, m) in enumerate(zip(case.types, case.Ms))]


# ------------------------------------------------------------------------------------------------- one case

def run_case(q, case, ws, x, nw=None, res=None):
    """the case's call: every dst (and every residual) a view of row stride M + 24 into a sentinel-filled buffer.  Returns (labels, outputs
    [N, M] as numpy arrays); asserts the labels, the guard columns, the untouched residual and the untouched second SwiGLU destination"""
    k, n = case.K, case.N
    wd = [on_device(q, t, w, k, wkey) for t, (w, wkey) in zip(case.types, ws)]
    bufs, outs, res_bufs, res_d = [], [], {}, [None] * MV_SLOTS
    for i, m in enumerate(case.Ms):
        buf = torch.full((n, m + GUARD), SENTINEL, device="cuda")
        if i in case.res:
            r = dev(res[i])
            if case.form == "inplace":
                buf[:, :m] = r
                res_d[i] = buf[:, :m]
            else:
                rb = torch.full((n, m + GUARD), SENTINEL, device="cuda")
                rb[:, :m] = r
                res_bufs[i], res_d[i] = rb, rb[:, :m]
        bufs.append(buf)
        outs.append(buf[:, :m])
    xd = dev(x)
    nwd = dev(nw) if case.norm else None
    labels = q.trace(lambda: q.mul_mat_group_ex(wd, k, xd, outs, norm_w=nwd, eps=EPS if case.norm else 0.0, residuals=res_d if case.res else None,
                                                swiglu=case.swiglu))
    q.synchronize()
    assert labels == F.labels_of(case), (case.name, labels, F.labels_of(case))
    got = []
    for i, (buf, m) in enumerate(zip(bufs, case.Ms)):
        a = buf.cpu().numpy()
        assert (a[:, m:] == np.float32(SENTINEL)).all(), (case.name, i, "guard columns written")
        if case.swiglu and i == 1:
            assert (a == np.float32(SENTINEL)).all(), (case.name, "the second destination of a SwiGLU launch written")
        else:
            assert not (a[:, :m] == np.float32(SENTINEL)).any(), (case.name, i, "outputs left unwritten")
        if i in res_bufs:
            rb = res_bufs[i].cpu().numpy()
            assert np.array_equal(rb[:, :m], res[i]) and (rb[:, m:] == np.float32(SENTINEL)).all(), (case.name, i, "the residual buffer written")
        got.append(a[:, :m].astype(np.float64))
    return labels, got


def expected(refs, case, ws, x, nw=None, res=None, rows=None):
    """(want float64 [N, M], bar, is SwiGLU) per written destination of the matrices in ws.  rows: a slice of every matrix's rows"""
    xin = H.rms_norm_f32(x, nw, EPS) if case.norm else x
    xkey = (xin.shape, zlib.crc32(np.ascontiguousarray(xin).tobytes()))
    prods = []
    for t, (w, wkey) in zip(case.types, ws):
        prods.append(refs.product((wkey, rows and (rows.start, rows.stop), xkey), t, w if rows is None else w[rows], case.K, xin))
    if case.swiglu:
        g, u = prods[case.swiglu - 1], prods[2 - case.swiglu]
        with np.errstate(over="ignore"):                               # exp(-g) of a large negative g: silu is -0 there
            return [(g / (1.0 + np.exp(-g)) * u, swiglu_bar(g, u), True)]
    out = []
    for i, p in enumerate(prods):
        r = res[i].astype(np.float64) if i in case.res else 0.0
        out.append((p + (r if rows is None or i not in case.res else r[:, rows]), BAR, False))
    return out


def error(got, want, is_swiglu):
    """SwiGLU: max |err| (swiglu_bar is absolute); else max |err| / rms(want)"""
    e = float(np.abs(got - want).max())
    return e if is_swiglu else e / rms(want)


def names(case):
    return "+".join(F.NAMES[t] for t in dict.fromkeys(case.types))


_seen = []                                   # (err / bar, err, bar, is SwiGLU, where) of every comparison of the running test


def note(err, bar, sw, where):
    _seen.append((err / bar, err, bar, sw, where))


@pytest.fixture(autouse=True)
def digest(request):
    """one line per test behind its launches' lines: how many comparisons, and the one closest to its bar (the lines of
    profiles/matvec_fold_errors.txt)"""
    _seen.clear()
    yield
    if _seen:
        _, err, bar, sw, where = max(_seen)
        print(f"\nfolds == {request.node.name} | {len(_seen)} comparisons | closest to its bar: {'max|err|' if sw else 'max|err|/rms'} {err:.3e} (bar {bar:.3e}) at {where}")


def check(refs, case, labels, got, ws, x, nw=None, res=None, what=""):
    """one printed line per launch of the case's call (the worst of its matrices); returns what is over its bar"""
    over, worst = [], None
    for i, (want, bar, sw) in enumerate(expected(refs, case, ws, x, nw, res)):
        err = error(got[i], want, sw)
        note(err, bar, sw, f"{case.name}{what} m{i}")
        if worst is None or err / bar > worst[0] / worst[1]:
            worst = (err, bar, sw, i)
        if not err <= bar:
            over.append((case.name, i, err, bar))
    err, bar, sw, i = worst
    print(f"folds | {names(case)} | {case.section} {case.name}{what} | {case.path} | {';'.join(labels)} | {'max|err|' if sw else 'max|err|/rms'} {err:.3e} at m{i} (bar {bar:.3e})")
    return over


def run_and_check(q, refs, case, what=""):
    ws = case_weights(case)
    x = case_inputs(case)
    nw = norm_weight(case.K) if case.norm else None
    res = {i: residual(case, i) for i in case.res}
    labels, got = run_case(q, case, ws, x, nw, res)
    return got, check(refs, case, labels, got, ws, x, nw, res, what=what)


def a_params(section):
    out = []
    for t in F.TYPES:
        for k in sorted({c.K for c in F.cases_a(t) if c.section == section}):
            out.append(param(t, k))
    return out


# ------------------------------------------------------------------------------------------------- a. every type, every fold

@pytest.mark.parametrize("t,k", a_params("a-norm"))
def test_a_norm(contexts, refs, t, k):
    """three same-type matrices of 40 / 24 / 8 rows behind one folded norm: every NTOK instantiation at K = 1024, the largest token counts
    mv_fits_norm takes at K = 4096 and 5120, the ragged K = 768 and (wire blocks of 32) 1056"""
    over = []
    for case in [c for c in F.cases_a(t) if c.section == "a-norm" and c.K == k]:
        over += run_and_check(contexts("default"), refs, case)[1]
    assert not over, over


@pytest.mark.parametrize("t,k", a_params("a-res"))
def test_a_residual(contexts, refs, t, k):
    """dst = W x + residual on one matrix of 40 rows (the plugin's form), out of place and in place, padded strides; and on the second of three
    matrices only"""
    over = []
    for case in [c for c in F.cases_a(t) if c.section == "a-res" and c.K == k]:
        over += run_and_check(contexts("default"), refs, case)[1]
    assert not over, over


@pytest.mark.parametrize("t,k", a_params("a-swiglu"))
def test_a_swiglu(contexts, refs, t, k):
    """silu(W_gate x) * (W_up x) on two matrices of 24 rows, gate first and up first, without and with the norm; the second destination keeps
    its sentinel"""
    over = []
    for case in [c for c in F.cases_a(t) if c.section == "a-swiglu" and c.K == k]:
        over += run_and_check(contexts("default"), refs, case)[1]
    assert not over, over


# ------------------------------------------------------------------------------------------------- b. mixed launches

@pytest.mark.parametrize("k", sorted({c.K for c in F.cases_b()}))
def test_b_mixed_launches(contexts, refs, k):
    """matvec_kmix_kernel with a norm (one pass and two steps), with residuals on all matrices and on one, wire and planar Q6_K, a Q6_K matrix
    first; the mixed-format group with residuals (one launch up to 4 tokens, per-type runs at 5) and with a norm (per-type runs, asserted in
    order by the labels)"""
    over = []
    for case in [c for c in F.cases_b() if c.K == k]:
        over += run_and_check(contexts("default"), refs, case)[1]
    assert not over, over


# ------------------------------------------------------------------------------------------------- c. geometry

GEO = [param(t, f"{fold}-{k}-{n}") for t in tuple(F.REPS.values()) + (F.MIXED,) for fold, k, n, _, sw, _ in F.GEOMETRY_FOLDS if not (t == F.MIXED and sw)]


@pytest.mark.parametrize("t,fold", GEO)
def test_c_geometry(contexts, refs, t, fold):
    """the same weight rows in launches of 2304, 1280 and 40 rows (16-, 8- and 4-wave workgroups on 256 CUs): rows are independent and the norm's
    order is fixed, so the rows the three launches share are bit-identical; the 40-row launch and the last 40 rows of the 2304-row launch
    (the `row += W` walk, locate) against the reference"""
    q = contexts("default")
    cases = [c for c in F.cases_c(t) if c.name.startswith(f"geo-{fold}-")]
    assert [max(c.Ms) for c in cases] == [2304 if t != F.MIXED else 2272, 1280 if t != F.MIXED else 1248, 40 if t != F.MIXED else 24]
    big = cases[0]
    big_ws = case_weights(big, seed0=51)
    x = case_inputs(big)
    nw = norm_weight(big.K) if big.norm else None
    shared, over = [], []
    for case in cases:
        if t == F.MIXED:                                               # (M - 32, 24, 8): the first rows of the big first matrix, the others whole
            ws = [(big_ws[0][0][:case.Ms[0]], big_ws[0][1] + (case.Ms[0],))] + big_ws[1:]
            cut = 8
        else:
            ws = [(w[:m], wkey + (m,)) for (w, wkey), m in zip(big_ws, case.Ms)]
            cut = 40
        res = {i: np.ascontiguousarray(residual(big, i)[:, :case.Ms[i]]) if i == 0 else residual(big, i) for i in case.res}
        labels, got = run_case(q, case, ws, x, nw, res)
        shared.append([got[0][:, :cut]] + got[1:] if not case.swiglu else [got[0][:, :cut]])
        m = case.Ms[0]
        print(f"folds | {names(case)} | c {case.name} | {case.path} | {';'.join(labels)} | block {case.launches[0].waves * 64} grid {case.launches[0].grid} (pinned for {F.CUS} CUs)")
        if case is cases[-1]:
            over += check(refs, case, labels, got, ws, x, nw, res)
        if case is cases[0]:                                           # the last rows of the first matrix (the mixed group's small matrices: bit for bit below)
            last = slice(m - cut, m)
            want = expected(refs, case, ws if case.swiglu else ws[:1], x, nw, res, rows=last)
            w0, bar, sw = want[0]
            err = error(got[0][:, last], w0, sw)
            note(err, bar, sw, f"{case.name} last {cut} rows")
            print(f"folds | {names(case)} | c {case.name} last {cut} rows | {case.path} | {';'.join(labels)} | {'max|err|' if sw else 'max|err|/rms'} {err:.3e} (bar {bar:.3e})")
            if not err <= bar:
                over.append((case.name, "last rows", err, bar))
    for other, case in zip(shared[1:], cases[1:]):
        for a, b in zip(shared[0], other):
            assert np.array_equal(a.astype(np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)), (case.name, "differs from the 16-wave launch")
    assert not over, over


# ------------------------------------------------------------------------------------------------- d. one pass == two steps

D_PARAMS = [param(t, k) for t in F.q8k_types() + (F.MIXED,) for k in sorted({c.K for c in F.cases_d(t)})]


@pytest.mark.parametrize("t,k", D_PARAMS)
def test_d_one_pass_equals_two_step(contexts, refs, t, k):
    """the norm launch in the default context (stage_q8k_rows) and in one created under GGML_MI355X_MV_ONEPASS=0 (stage_rms_norm +
    quantize_rows): the same bits, as stage_q8k_rows' comment claims; both against the reference"""
    cases = [c for c in F.cases_d(t) if c.K == k]
    over = []
    for on, off in zip(cases[0::2], cases[1::2]):
        assert (on.ctx, off.ctx, on.N) == ("default", "onepass=0", off.N)
        got_on, o1 = run_and_check(contexts("default"), refs, on)
        got_off, o2 = run_and_check(contexts("onepass=0"), refs, off)
        over += o1 + o2
        for a, b in zip(got_on, got_off):
            assert np.array_equal(a.astype(np.float32).view(np.uint32), b.astype(np.float32).view(np.uint32)), (on.name, "one pass and two steps differ")
    assert not over, over


# ------------------------------------------------------------------------------------------------- e. sub-batches with a residual

@pytest.mark.parametrize("t", [param(t) for t in F.REPS.values()])
def test_e_sub_batches_with_a_residual(contexts, refs, t):
    """K = 16384 x 8 tokens (4 + 4) and K = 28672 x 7 (4 + 3): the second launch's dst and residual start n0 rows down their padded
    buffers; every token row against the reference"""
    over = []
    for case in F.cases_e(t):
        assert [l.n0 for l in case.launches] == [0, 4]
        got, o = run_and_check(contexts("default"), refs, case)
        over += o
        ws, x, res = case_weights(case), case_inputs(case), {0: residual(case, 0)}
        want = expected(refs, case, ws, x, None, res)[0][0]
        for row in range(case.N):
            err = error(got[0][row], want[row], False)
            note(err, BAR, False, f"{case.name} token {row}")
            print(f"folds | {names(case)} | e {case.name} token {row} | max|err|/rms {err:.3e} (bar {BAR:.3e})")
            if not err <= BAR:
                over.append((case.name, "token", row, err))
    assert not over, over


# ------------------------------------------------------------------------------------------------- f. activation value edges

def edge_rows(fmt, k, nw):
    """4 rounding-stable token rows: all zeros; one element 1e4 times the rest; every 256-block's largest magnitude negative (Q8_K's signed
    maximum); a plain one"""
    def shape(r, row):
        if r == 1:
            row[k // 2 + 3] = 1e4 * np.sign(row[k // 2 + 3])
        if r == 2:
            blk = row.reshape(-1, 256)
            at = np.abs(blk).argmax(axis=1)
            blk[np.arange(blk.shape[0]), at] = -1.5 * np.abs(blk[np.arange(blk.shape[0]), at])
        return row
    x, _ = H.rounding_stable_rows(fmt, 4, k, nw, EPS, seed=99 + fmt, shape=shape)
    x[0] = 0.0
    return x


@pytest.mark.parametrize("t", [param(t) for t in F.REPS.values()])
def test_f_value_edges(contexts, refs, t):
    """K = 1024, 4 tokens, eps = 1e-5 through the norm launch, the norm + residual launch and the norm + SwiGLU launch, with a plain norm weight
    and with one that has zero and negative entries.  The all-zero row gives exactly 0 (exactly the residual)"""
    q = contexts("default")
    k = 1024
    plain = norm_weight(k)
    holed = plain.copy()
    holed[::7] = 0.0
    holed[3::5] *= -1.0
    over = []
    for wname, nw in (("plain weight", plain), ("zero and negative weights", holed)):
        x = edge_rows(F.act(t), k, nw)
        for case in F.cases_f(t):
            ws = case_weights(case)
            res = {i: residual(case, i) for i in case.res}
            labels, got = run_case(q, case, ws, x, nw, res)
            over += check(refs, case, labels, got, ws, x, nw, res, what=f" ({wname})")
            for i, g in enumerate(got[:1] if case.swiglu else got):
                zero = res[i][0].astype(np.float64) if i in case.res else np.zeros(case.Ms[i])
                assert np.array_equal(g[0], zero), (case.name, wname, "the all-zero row", g[0][:8])
    assert not over, over


# ------------------------------------------------------------------------------------------------- g. refusals

def test_g_refusals(contexts):
    """a norm on more tokens than mv_fits_norm takes, SwiGLU on unequal row counts or with a residual: QmmError, and nothing written"""
    from ggml_hexagon_amd.capi import QmmError
    q = contexts("default")
    for case in F.cases_g():
        ws = case_weights(case)
        wd = [on_device(q, t, w, case.K, wkey) for t, (w, wkey) in zip(case.types, ws)]
        outs = [torch.full((case.N, m + GUARD), SENTINEL, device="cuda") for m in case.Ms]
        res = [torch.full((case.N, m + GUARD), 3.0, device="cuda")[:, :m] if i in case.res else None for i, m in enumerate(case.Ms)]
        x = dev(inputs(H.Q8_K, case.K, False)[:case.N])
        with pytest.raises(QmmError) as e:
            q.mul_mat_group_ex(wd, case.K, x, [o[:, :m] for o, m in zip(outs, case.Ms)], norm_w=dev(norm_weight(case.K)) if case.norm else None,
                               eps=EPS, residuals=res if case.res else None, swiglu=case.swiglu)
        q.synchronize()
        print(f"folds | g {case.name} | refused: {e.value}")
        assert case.refusal in str(e.value)
        assert all(bool((o == SENTINEL).all()) for o in outs), case.name
