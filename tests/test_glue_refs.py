"""The numpy references of tests/glue_refs.py against independent implementations (torch on the CPU, properties written out by hand),
so that a shared misunderstanding between a reference and its kernel cannot hide; the float32 restatements of every GPU case against
their float64 references; and the trace labels of csrc/qmm_glue_plan.h against the cases, so that a new launcher branch cannot arrive
untested.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest

import glue_cases as G
import glue_refs as R
from glue_refs import F16, F32, f32, f64

torch = pytest.importorskip("torch")
F = torch.nn.functional
ROOT = Path(__file__).resolve().parents[1]


def t64(a):
    return torch.from_numpy(np.asarray(a, f64))


def close(a, b, tol=1e-12):
    return R.rel_rms(np.asarray(a, f64), np.asarray(b, f64)) < tol


# ------------------------------------------------------------------------------------------------ references against torch
def test_binary_broadcast_is_ggml_repeat():
    rng = np.random.default_rng(0)
    a = rng.normal(size=(2, 3, 5, 8))
    for bshape in ((2, 3, 5, 8), (1, 3, 1, 8), (1, 1, 5, 1), (1, 1, 1, 1), (1, 3, 5, 4), (2, 1, 1, 2)):
        b = rng.normal(size=bshape) + 3.0
        want = a.copy()
        for idx in np.ndindex(*a.shape):                     # element i of dst reads b[i mod ne]
            want[idx] = b[tuple(i % n for i, n in zip(idx, bshape))]
        assert np.array_equal(R.repeat_to(b, a.shape), want)
        for op, fn in (("add", torch.add), ("sub", torch.sub), ("mul", torch.mul), ("div", torch.div)):
            assert np.array_equal(R.binary(op, a, b), fn(t64(a), t64(want)).numpy())
            assert R.binary(op, a, b, f32).dtype == f32


def test_unaries_against_torch():
    x = np.concatenate([np.linspace(-20, 20, 4001), [0.0, -0.0, 88.0, -88.0]])
    tx = t64(x)
    want = {"silu": F.silu(tx), "gelu": F.gelu(tx, approximate="tanh"), "gelu_quick": tx * torch.sigmoid(1.702 * tx), "relu": torch.relu(tx),
            "tanh": torch.tanh(tx), "sigmoid": torch.sigmoid(tx), "neg": -tx, "exp": torch.exp(tx), "scale": tx * float(f32(0.37))}
    assert set(want) == set(R.UNARIES)
    for name, w in want.items():
        # (the kernel's constants are float32 values: sqrt(2 / pi) and 1.702 differ from the double ones in the eighth digit)
        assert close(R.unary(name, x, 0.37), w.numpy(), 1e-6 if name in ("gelu", "gelu_quick") else 1e-12), name
    b = np.linspace(3, -3, len(x))
    assert close(R.silu_mul(x, b), (F.silu(tx) * t64(b)).numpy())


def test_norms_against_torch():
    rng = np.random.default_rng(1)
    x = rng.normal(0.5, 2, (2, 3, 4, 257)).astype(f32)
    w = rng.normal(1, 0.2, 257).astype(f32)
    b = rng.normal(0, 1, x.shape).astype(f32)
    for eps in (0.0, 1e-6):
        assert close(R.rms_norm(x, eps), F.rms_norm(t64(x), (257,), eps=float(f32(eps))).numpy())
        assert close(R.rms_norm(x, eps, w), F.rms_norm(t64(x), (257,), weight=t64(w), eps=float(f32(eps))).numpy())
        y, s = R.rms_norm(x, eps, w, b)
        assert s.dtype == f32 and np.array_equal(s, x + b)
        assert close(y, F.rms_norm(t64(x + b), (257,), weight=t64(w), eps=float(f32(eps))).numpy())
        assert close(R.norm(x, eps), F.layer_norm(t64(x), (257,), eps=float(f32(eps))).numpy())
    assert np.array_equal(R.norm(np.full((1, 9), 3.25), 1e-5), np.zeros((1, 9)))


def test_alibi_slopes_written_out():
    # n_head = 8, max_bias = 8: m0 = 2^-1, slope(h) = m0^(h + 1)
    assert np.array_equal(R.alibi_slopes(8, 8.0), [1 / 2, 1 / 4, 1 / 8, 1 / 16, 1 / 32, 1 / 64, 1 / 128, 1 / 256])
    # n_head = 6: n_head_log2 = 4, m0 = 2^-2 for heads 0..3; m1 = 2^-1 for heads 4, 5 with exponents 1, 3
    assert np.array_equal(R.alibi_slopes(6, 8.0), [1 / 4, 1 / 16, 1 / 64, 1 / 256, 1 / 2, 1 / 8])
    assert np.array_equal(R.alibi_slopes(6, 0.0), np.ones(6))
    assert np.array_equal(R.alibi_slopes(6, 8.0, f32), R.alibi_slopes(6, 8.0).astype(f32))


def test_soft_max_against_torch():
    rng = np.random.default_rng(2)
    x = rng.normal(0, 2, (2, 6, 5, 77)).astype(f32)
    m32 = rng.normal(0, 1, (8, 77)).astype(f32)
    m32[np.triu_indices(8, 1, 77)] = -np.inf
    m16 = m32.astype(np.float16)
    assert close(R.soft_max(x), torch.softmax(t64(x), -1).numpy())
    for m, bias in ((m32, 0.0), (m16, 0.0), (m32, 8.0), (m16, 8.0)):
        slopes = t64([1 / 4, 1 / 16, 1 / 64, 1 / 256, 1 / 2, 1 / 8] if bias else np.ones(6))
        v = t64(x) * float(f32(0.1)) + slopes[None, :, None, None] * t64(m.astype(f64)[:5])[None, None]      # mask row i1 for every head and batch
        assert close(R.soft_max(x, m, 0.1, bias), torch.softmax(v, -1).numpy())
    assert R.soft_max(x, m32, 0.1, 0.0, f32).dtype == f32


def test_rope_properties():
    rng = np.random.default_rng(3)
    pos = [0, 1, 4095, 100000]
    x = rng.normal(0, 1, (2, 4, 3, 80)).astype(f32)
    ff = rng.uniform(0.8, 4, 16).astype(f32)
    yarn = dict(freq_scale=0.25, ext_factor=1.0, attn_factor=1.25)
    for kw in ({}, dict(ff=ff), yarn, dict(ff=ff, **yarn), dict(attn_factor=0.5)):
        th, mscale = R.rope_angles(pos, 32, **kw)
        for neox in (False, True):
            y = R.rope(x, pos, 32, neox, **kw)
            # position 0 is the identity times the magnitude scale (attn_factor, times 1 + 0.1 ln(1 / freq_scale) with YaRN)
            want0 = x[:, 0].astype(f64).copy()
            want0[..., :32] *= float(mscale)
            assert close(y[:, 0], want0)
            assert np.array_equal(y[..., 32:], x[..., 32:])                       # channels from n_dims on pass through
            ia = np.arange(16) if neox else 2 * np.arange(16)
            ib = ia + 16 if neox else ia + 1
            n_in = x[..., ia].astype(f64) ** 2 + x[..., ib].astype(f64) ** 2
            n_out = y[..., ia] ** 2 + y[..., ib] ** 2
            assert np.allclose(n_out, n_in * float(mscale) ** 2, rtol=1e-12)      # the pair norm is kept up to mscale
        # NEOX is normal mode under the channel permutation that puts pair p at (p, p + n_dims / 2)
        perm = np.concatenate([2 * np.arange(16), 2 * np.arange(16) + 1, np.arange(32, 80)])
        assert np.array_equal(R.rope(x[..., perm], pos, 32, True, **kw), R.rope(x, pos, 32, False, **kw)[..., perm])
        # the angle itself: pos * theta_scale^p / ff, scaled; without YaRN exactly freq_scale * that in float32 steps
        if "ext_factor" not in kw:
            ts = float(R.powf(10000.0, -2.0 / 32))
            ideal = np.array(pos, f64)[:, None] * ts ** np.arange(16)[None, :] / (ff.astype(f64) if "ff" in kw else 1.0)
            assert np.allclose(th, ideal, rtol=16 * 2.0 ** -23)
    assert float(R.rope_angles(pos, 32, **yarn)[1]) == pytest.approx(1.25 * (1 + 0.1 * np.log(4.0)), rel=1e-6)
    # YaRN: pairs below the ramp keep the extrapolated angle, pairs above it the interpolated one (a quarter of it)
    c0, c1 = R.rope_corr_dims(128, 8192, 10000.0, 32.0, 1.0)
    assert (c0, c1) == (25.0, 50.0)                    # 128 ln(8192 / (32 * 2 pi)) / (2 ln 10000) = 25.76, ... (1 * 2 pi) = 49.85
    th_y, _ = R.rope_angles(pos, 128, **yarn)
    th_n, _ = R.rope_angles(pos, 128)
    assert np.array_equal(th_y[:, :26], th_n[:, :26]) and np.array_equal(th_y[:, 50:], f32(0.25) * th_n[:, 50:])


def test_rope_matches_the_earlier_layer_test_reference():
    """the normal-mode reference that test_gpu_layer_ops.py carried before (theta by repeated float32 multiply, cos / sin in double, the
    rotation in float32) agrees with this one to float32 rounding"""
    rng = np.random.default_rng(4)
    x = rng.normal(0, 1, (5, 8, 128)).astype(f32)
    pos = np.arange(17, 22)
    ts = R.powf(10000.0, -2.0 / 128)
    out = x.copy()
    for t in range(5):
        theta = f32(pos[t])
        for p in range(64):
            c, s = f32(np.cos(f64(theta))), f32(np.sin(f64(theta)))
            x0, x1 = x[t, :, 2 * p].copy(), x[t, :, 2 * p + 1].copy()
            out[t, :, 2 * p], out[t, :, 2 * p + 1] = x0 * c - x1 * s, x0 * s + x1 * c
            theta = f32(theta * ts)
    assert R.rel_rms(out, R.rope(x[None], pos, 128)[0]) < 1e-6


def test_cpy_against_as_strided():
    rng = np.random.default_rng(5)
    as_strided = np.lib.stride_tricks.as_strided
    src = rng.integers(0, 256, 4096, dtype=np.uint8)
    src.view(np.float16)[:] = rng.normal(0, 3, 2048).astype(np.float16)
    dst0 = rng.integers(0, 256, 8192, dtype=np.uint8)
    # f16 [7, 5, 3] permuted view (dim 1 fastest) at byte offset 6 -> f32 [21, 5] with padded rows at byte offset 8
    s_ne, s_nb, d_ne, d_nb = [7, 5, 3, 1], [10, 2, 80, 240], [21, 5, 1, 1], [4, 100, 500, 500]
    got = R.cpy(src, F16, s_ne, s_nb, 6, dst0, F32, d_ne, d_nb, 8)
    sv = as_strided(src[6:].view(np.float16), shape=(3, 5, 7), strides=(80, 2, 10))
    want = dst0.copy()
    as_strided(want[8:].view(f32), shape=(5, 21), strides=(100, 4))[...] = np.ascontiguousarray(sv).reshape(5, 21).astype(f32)
    assert np.array_equal(got, want)
    assert np.array_equal(R.strided_offsets([3, 2], [4, 40, 0, 0]), [0, 4, 8, 40, 44, 48])
    # the operand helper reads and writes the same elements
    b = R.Buf(F16, s_ne, s_nb, off=6)
    b.root.host[:] = src[:len(b.root.host)]
    assert np.array_equal(b.values()[0], sv)
    assert b.inside().sum() == 7 * 5 * 3 * 2


def test_get_rows_mul_mat_argsort_sum_rows_against_torch():
    rng = np.random.default_rng(6)
    a = rng.normal(0, 1, (2, 3, 9, 20)).astype(f32)
    ids = rng.integers(0, 9, (2, 3, 4)).astype(np.int32)
    want = torch.gather(torch.from_numpy(a), 2, torch.from_numpy(ids.astype(np.int64))[..., None].expand(2, 3, 4, 20)).numpy()
    assert np.array_equal(R.get_rows(a, ids), want)
    # MUL_MAT: a [K, M, 2, 1] broadcast to b [K, N, 8, 2]: head i12 of b uses head i12 / 4 of a
    wa = rng.normal(0, 1, (1, 2, 13, 37)).astype(np.float16)
    xb = rng.normal(0, 1, (2, 8, 5, 37)).astype(f32)
    ta = t64(wa.astype(f64)).repeat_interleave(4, dim=1).expand(2, 8, 13, 37)
    assert close(R.mul_mat(wa, xb, True), torch.matmul(t64(xb.astype(np.float16).astype(f64)), ta.transpose(-1, -2)).numpy())
    assert close(R.mul_mat(wa.astype(f32), xb), torch.matmul(t64(xb), ta.transpose(-1, -2)).numpy())
    assert R.rel_rms(R.mul_mat_f32(wa, xb, True), R.mul_mat(wa, xb, True)) < 2e-6
    x = rng.normal(0, 1, (3, 300)).astype(f32)
    x[:, rng.integers(0, 300, 100)] = 0.5
    x[0, 5], x[0, 9], x[1, 0] = np.inf, np.inf, -np.inf
    assert np.array_equal(R.argsort(x), torch.argsort(torch.from_numpy(x), dim=-1, stable=True).numpy())
    assert np.array_equal(R.argsort(x, True), torch.argsort(torch.from_numpy(x), dim=-1, descending=True, stable=True).numpy())
    assert close(R.sum_rows(x[1:, 10:]), t64(x[1:, 10:]).sum(-1, keepdim=True).numpy())
    assert R.seq_sum_f32(np.array([1e8, 1.0, 1.0, 1.0, 1.0], f32)) == f32(1e8)         # sequential: every 1 is lost; a pairwise sum keeps them


# ------------------------------------------------------------------------------------------------ the cases of the GPU test
@pytest.mark.parametrize("cid", G.IDS)
def test_case_restatement_has_room(cid):
    """every GPU case builds on the CPU; its float32 restatement meets the NMSE bar the kernels are held to with ten times room (a
    case whose own restatement could not would be a bar the format, not the kernel, fails); exact cases carry an exact array of the
    destination's shape and type"""
    c = G.BUILDERS[cid]()
    assert c.label and c.want.shape == c.dst.shape, (c.want.shape, c.dst.shape)
    if c.exact:
        assert c.rest is None and c.want.dtype == c.dst.dt
        return
    assert c.rest.dtype == f32 and c.want.dtype == f64 and np.isfinite(c.want).all() and np.isfinite(c.rest).all()
    assert R.nmse(c.rest, c.want) <= 1e-8, R.nmse(c.rest, c.want)
    assert c.bound() >= G.FLOOR


def test_no_case_has_a_fully_masked_row_or_a_nan():
    for cid in G.IDS:
        if cid.startswith("soft_max"):
            c = G.BUILDERS[cid]()
            assert np.isfinite(c.want).all() and np.all(c.want.sum(-1) > 0.999), cid
            if c.src[1] is not None:
                m = c.src[1].values().astype(f64)[0, 0][:c.dst.ne[1]]
                assert np.isfinite(m).any(axis=-1).all(), cid


# ------------------------------------------------------------------------------------------------ labels
def glue_labels():
    """the label strings of the one table of csrc/qmm_glue_plan.h (GLUE_LABELS) that every glue plan takes its label from; a %d stands for a
    template argument"""
    src = (ROOT / "ggml-hexagon_amd" / "csrc" / "qmm_glue_plan.h").read_text()
    table = re.search(r"GLUE_LABELS\[GL_COUNT\]\s*=\s*\{(.*?)\};", src, re.S).group(1)
    labels = re.findall(r'"([^"]+)"', table)
    assert len(labels) == len(set(labels))
    rest = re.sub(r"GLUE_LABELS\[GL_COUNT\]\s*=\s*\{.*?\};", "", src, flags=re.S)
    assert not [t for t in re.findall(r'"([^"]+)"', rest) if "_kernel" in t or t == "memcpy"]          # no label is spelled outside the table
    return sorted(labels)


def test_every_trace_label_of_the_glue_launchers_has_a_case():
    labels = glue_labels()
    assert len(labels) >= 20, labels
    text = (ROOT / "tests" / "test_gpu_glue_ops.py").read_text()
    asserted = {G.BUILDERS[cid]().label for cid in G.IDS}
    for lab in labels:
        assert f'"{lab}"' in text, f"tests/test_gpu_glue_ops.py does not list the label {lab}"
        if "%" in lab:                          # get_rows_q_kernel<%d>: test_get_rows_quantized asserts it per weight type
            assert 'f"' + lab.replace("%d", "{t}") + '"' in text, lab
        else:
            assert lab in asserted, f"no case of tests/glue_cases.py expects the label {lab}"
    # ... and no case expects a label the launchers cannot emit
    assert asserted <= set(labels), asserted - set(labels)
