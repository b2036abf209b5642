"""GPU parity of the per-node glue kernels behind qmm_op_compute / qmm_op_add_rms_norm (csrc/qmm_ops.hip) against the numpy references
of tests/glue_refs.py, one case per launcher branch (tests/glue_cases.py), with no need of the reference build.  Every case asks
qmm_op_supported (1), runs under qmm.trace, asserts the label of the branch it was written for, then compares:

  * single IEEE operations and data movement (ADD, SUB, MUL, DIV, NEG, RELU, SCALE, CPY, GET_ROWS, ARGSORT, the sum of add_rms_norm):
    bit for bit against numpy float32;
  * everything else against the float64 reference: NMSE <= 1e-7 (the bar of test-backend-ops) and max|got - want| / rms(want) at most
    4 x the same figure of the sequential float32 restatement of the op on the same inputs, never below 2e-6 (the kernels sum in a
    tree over lanes, waves and LDS where the restatement sums in sequence); YaRN rope carries a derived addition (glue_cases.py);
  * every byte of the destination's buffer outside the destination view, and every source, is compared with what was uploaded.

Each comparison prints `glue-parity | op | label | shape | nmse | rel_rms | restatement nmse | restatement rel_rms | bound`
(profiles/glue_parity_errors.txt is that table from one run)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import glue_cases as G  # noqa: E402
import glue_refs as R  # noqa: E402
from glue_refs import F32, I32, Buf  # noqa: E402
from oracle.pyoracle import TYPE_NAMES, WEIGHT_TYPES  # noqa: E402

# every label the glue launches can emit (tests/test_glue_refs.py holds this list against the label table of qmm_glue_plan.h and
# against the labels the cases assert)
LABELS = ("binary_kernel<vec>", "binary_kernel<scalar>", "unary_kernel", "rms_norm_vec_kernel<1024>", "rms_norm_vec_kernel<256>", "rms_norm_kernel",
          "norm_kernel", "soft_max_wave_kernel<1>", "soft_max_wave_kernel<2>", "soft_max_wave_kernel<4>", "soft_max_kernel<lds>", "soft_max_kernel<dst>",
          "rope_kernel", "memcpy", "cpy_kernel", "cpy_transpose_kernel", "get_rows_kernel", "get_rows_q_kernel<%d>", "mul_mat_f16_kernel<vec>",
          "mul_mat_f16_kernel<scalar>", "mul_mat_dot_block_kernel", "mul_mat_dot_kernel", "argsort_kernel", "sum_rows_kernel")
NMSE_BAR = 1e-7


@pytest.fixture(scope="module")
def qmm():
    from ggml_hexagon_amd.capi import Qmm
    q = Qmm(0)
    yield q
    q.close()


def ref_of(t):
    from ggml_hexagon_amd import capi
    return capi.C.byref(t) if t is not None else None


def launch(qmm, c):
    """supported -> traced launch -> the label; returns the destination buffer's bytes after the launch.  A device fault ends the
    session: nothing further is launched on a device that has faulted"""
    try:
        return launch_checked(qmm, c)
    except (RuntimeError, OSError) as e:                         # QmmError is a RuntimeError; torch raises RuntimeError too
        if any(m in str(e) for m in ("illegal memory access", "hipErrorIllegalAddress", "unspecified launch failure", "hipErrorLaunchFailure")):
            pytest.exit(f"device fault, nothing further is launched: {e}", returncode=3)
        raise


def launch_checked(qmm, c):
    srcs = [s.tensor() if s is not None else None for s in c.src]
    dst = c.dst.tensor(c.params)
    if c.op == G.OP_ADD_RMS_NORM:
        a, b, w = srcs
        s = c.sum.tensor()
        assert qmm.lib.qmm_op_add_rms_norm_supported(ref_of(a), ref_of(b), ref_of(w), ref_of(s), ref_of(dst)) == 1
        labels = qmm.trace(lambda: qmm._chk(qmm.lib.qmm_op_add_rms_norm(qmm.ctx, ref_of(a), ref_of(b), ref_of(w), ref_of(s), ref_of(dst), c.eps, qmm._stream())))
    else:
        assert qmm.lib.qmm_op_supported(c.op, ref_of(srcs[0]), ref_of(srcs[1]), ref_of(srcs[2]), ref_of(dst)) == 1
        labels = qmm.trace(lambda: qmm.op(c.op, dst, *srcs))
    assert labels == (c.label,), labels
    qmm.synchronize()
    return c.dst.download()


def check_untouched(c, raw):
    """the bytes around the destination view, and every operand that is not written, hold what was uploaded"""
    assert c.dst.outside_untouched(raw), "bytes outside the destination view were written"
    written = {id(c.dst.root)} | ({id(c.sum.root)} if c.sum is not None else set())
    if c.sum is not None:
        assert c.sum.outside_untouched(), "bytes outside the sum view were written"
    for s in c.src:
        if s is not None and id(s.root) not in written:
            assert np.array_equal(s.download(), s.root.before), "a source operand was written"


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(np.ascontiguousarray(got).view(np.uint8), np.ascontiguousarray(want).view(np.uint8))


def compare(c, cid, got, want=None, rest=None):
    want = c.want if want is None else want
    rest = c.rest if rest is None else rest
    assert np.isfinite(got).all(), cid
    nm, rr, bound = R.nmse(got, want), R.rel_rms(got, want), c.bound()
    print(f"glue-parity | {cid} | {c.label} | {c.shape} | {nm:.3e} | {rr:.3e} | {R.nmse(rest, want):.3e} | {R.rel_rms(rest, want):.3e} | {bound:.3e}")
    assert nm <= NMSE_BAR, (cid, nm)
    assert rr <= bound, (cid, rr, bound)


@pytest.mark.parametrize("cid", G.IDS)
def test_glue_op(qmm, cid):
    c = G.BUILDERS[cid]()
    raw = launch(qmm, c)
    check_untouched(c, raw)
    got = c.dst.read(raw)
    if c.op == G.OP_CPY:
        assert np.array_equal(raw, c.want_bytes), cid                  # the whole buffer: the copied elements and every byte around them
    if c.exact:
        want = c.want.astype(c.dst.dt)
        if c.untouched is not None:                                    # rows whose id is out of range keep what the buffer held
            want = np.where(c.untouched, c.dst.read(c.dst.root.before), want)
        ulp = 0
        if not same_bits(got, want) and c.op == G.OP_DIV:
            ulp = int(np.max(np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))))
        print(f"glue-parity | {cid} | {c.label} | {c.shape} | exact | max ulp {ulp} | - | - | 0")
        assert same_bits(got, want), cid
    else:
        compare(c, cid, got)
    if c.sum is not None:                                              # s = a + b of add_rms_norm: one IEEE addition
        assert same_bits(c.sum.read(), c.want_sum), cid


def test_labels_listed_here_are_the_labels_the_cases_assert():
    assert {G.BUILDERS[cid]().label for cid in G.IDS} | {"get_rows_q_kernel<%d>"} == set(LABELS)


def test_add_rms_norm_refuses_a_row_beyond_the_vector_kernel(qmm):
    """ne0 = 16388 is past the 16384 values a workgroup of rms_norm_vec_kernel holds; the scalar kernel has no sum output: refused, not emulated"""
    from ggml_hexagon_amd.capi import QmmError
    ne = [16388, 2]
    a, b, s, d = (Buf(F32, ne, seed=i).put(np.ones(ne[::-1])) for i in range(4))
    w = Buf(F32, [16388], seed=5).put(np.ones(16388))
    ts = [x.tensor() for x in (a, b, w, s, d)]
    assert qmm.lib.qmm_op_add_rms_norm_supported(*(ref_of(t) for t in ts)) == 0
    with pytest.raises(QmmError):
        qmm._chk(qmm.lib.qmm_op_add_rms_norm(qmm.ctx, *(ref_of(t) for t in ts), 1e-6, qmm._stream()))
    qmm.synchronize()
    assert np.array_equal(d.download(), d.root.before) and np.array_equal(s.download(), s.root.before)
    # at the limit itself it is supported (the case add_rms_norm-2x16384 runs it)
    ne = [16384, 2]
    ts = [Buf(F32, ne, seed=i).tensor() for i in range(2)] + [Buf(F32, [16384], seed=5).tensor()] + [Buf(F32, ne, seed=i).tensor() for i in (3, 4)]
    assert qmm.lib.qmm_op_add_rms_norm_supported(*(ref_of(t) for t in ts)) == 1


def long_row(t):
    """a row length whose units (32 or 64 weights, csrc/qmm_device.hiph Traits<T>::UNIT_W) do not fit the 256 threads of one trip: 260 units"""
    import ggml_hexagon_amd.synth as synth
    if synth.BLCK[t] == 32:
        return 260 * 32
    return 65 * 256 if t in (synth.Q6_K, synth.Q2_K, synth.Q3_K) else 33 * 256            # 64-weight units: 260 of them; 32-weight units: 264


@pytest.mark.parametrize("t", WEIGHT_TYPES, ids=[TYPE_NAMES[t] for t in WEIGHT_TYPES])
def test_get_rows_quantized(qmm, oracle, t):
    """GET_ROWS on every weight type against the oracle's dequantize_row, bit for bit: one block per row, three blocks, a row of 260
    units (a second, ragged trip of the 256 threads); rows further apart than their bytes; batched ids [3, 3, 2] through a strided view;
    ids -1 and ne1 leave their destination row as it was (src0 has a spare row either side, so even a broken guard reads allocated memory)"""
    import ggml_hexagon_amd.synth as synth
    from ggml_hexagon_amd.capi import QmmTensor
    rng = np.random.default_rng(40 + t)
    n_rows, ne11, ne12, ne10 = 5, 3, 2, 3
    for ne0, pad, batched in ((synth.BLCK[t], 0, False), (3 * synth.BLCK[t], 6, True), (long_row(t), 2, False)):
        b11, b12 = (ne11, ne12) if batched else (1, 1)
        rb = synth.row_size(t, ne0)
        nb1 = rb + pad
        w = synth.synth_weights(t, b12 * b11 * (n_rows + 2), ne0, seed=t + ne0, sigma=0.3).reshape(b12, b11, n_rows + 2, rb)
        host = rng.integers(0, 256, (b12, b11, n_rows + 2, nb1), dtype=np.uint8)
        host[..., :rb] = w
        dw = torch.from_numpy(host).cuda()
        deq = oracle.dequantize(t, w[:, :, 1:n_rows + 1].reshape(-1, rb), ne0).reshape(b12, b11, n_rows, ne0)
        idv = rng.integers(0, n_rows, (b12, b11, ne10)).astype(np.int32)
        idv[0, 0, 0], idv[-1, -1, -1] = -1, n_rows
        ids = Buf(I32, [ne10, b11, b12], [8, 8 * ne10 + 4, (8 * ne10 + 4) * b11 + 12, ((8 * ne10 + 4) * b11 + 12) * b12], seed=2).put(idv)
        d_ne = [ne0, ne10, b11, b12]
        d = Buf(F32, d_ne, G.nbytes_of(d_ne, 4, 16), seed=3)
        ta = QmmTensor.make(t, [ne0, n_rows, b11, b12], nb=[1, nb1, nb1 * (n_rows + 2), nb1 * (n_rows + 2) * b11], data=dw.data_ptr() + nb1)
        ti, td = ids.tensor(), d.tensor()
        assert qmm.lib.qmm_op_supported(G.OP_GET_ROWS, ref_of(ta), ref_of(ti), None, ref_of(td)) == 1, TYPE_NAMES[t]
        labels = qmm.trace(lambda: qmm.op(G.OP_GET_ROWS, td, ta, ti))
        assert labels == (f"get_rows_q_kernel<{t}>",), labels
        qmm.synchronize()
        raw = d.download()
        want = R.get_rows(deq, np.clip(idv, 0, n_rows - 1))
        untouched = np.zeros(want.shape, bool)
        untouched[0, 0, 0] = untouched[-1, -1, -1] = True
        want = np.where(untouched, d.read(d.root.before), want)
        print(f"glue-parity | get_rows-{TYPE_NAMES[t]}-{ne0} | get_rows_q_kernel<{t}> | ne0={ne0} pad{pad} batched{int(batched)} | exact | max ulp 0 | - | - | 0")
        assert same_bits(d.read(raw), want), (TYPE_NAMES[t], ne0)
        assert d.outside_untouched(raw) and np.array_equal(dw.cpu().numpy(), host) and np.array_equal(ids.download(), ids.root.before)
