"""TQ1_0 / TQ2_0 without a GPU: the numpy restatement of tests/tq_refs.py against the live reference (quantizer-made and crafted
blocks), the crafted blocks' coverage, and the kernel library's row geometry."""
import ctypes

import numpy as np
import pytest

import tq_refs as R

TYPES = [R.TQ1_0, R.TQ2_0]
IDS = [R.NAMES[t] for t in TYPES]


@pytest.fixture(scope="module")
def ref():
    return R.TqRef()


@pytest.fixture(scope="module")
def made(ref):
    """rows from the reference's quantizers: 6 rows of K = 1024 per type"""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((6, 1024)) * 0.05).astype(np.float32)
    return {t: ref.quantize(t, x) for t in TYPES}


def test_the_reference_has_the_block_sizes_of_the_restatement(ref):
    for t in TYPES:
        assert ref.ref.row_size(t, 256) == R.BLOCK_BYTES[t]


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_edge_rows_cover(t):
    for k in (256, 512, 768, 1024, 4096):
        for big in (True, False):
            rows = R.edge_rows(t, k, big=big)
            assert rows.shape == (R.N_EDGE // (k // 256), R.row_size(t, k))
            R.assert_edges(t, rows, k, big=big)


def test_trits_of_every_byte_follow_the_formula_past_242():
    """the restatement spelled out once more in plain integers, for all 256 byte values and the five powers: bytes 243 .. 255 wrap"""
    for b in range(256):
        for n in range(5):
            q = (b * 3 ** n) % 256
            assert int(R._trit(np.array([b], np.uint8), n)[0]) == (q * 3) // 256
    assert [int(R._trit(np.array([255], np.uint8), n)[0]) for n in range(5)] == [2, 2, 2, 2, 2]


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_numpy_dequantize_is_the_reference_bit_for_bit(ref, made, t):
    for k, rows in ((1024, made[t]), (256, R.edge_rows(t, 256)), (768, R.edge_rows(t, 768, seed=4))):
        want = ref.dequantize(t, rows, k)
        got = R.dequantize_np(t, rows, k)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if t == R.TQ2_0:                                                         # code 3 under d = 65504 is +131008, finite in f32
        assert np.abs(ref.dequantize(t, R.edge_rows(t, 256), 256)).max() == 2 * R.F16_MAX


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_numpy_dot_is_the_reference_within_f32_order(ref, made, t):
    rng = np.random.default_rng(10 + t)
    k = 1024
    x = rng.uniform(-1, 1, (3, k)).astype(np.float32)
    acts = ref.quantize_act(x)
    for rows in (made[t], R.edge_rows(t, k, big=False)[:12]):
        want = np.array([[ref.vec_dot(t, k, rows[j], acts[i]) for j in range(rows.shape[0])] for i in range(3)], np.float32)
        got = R.mul_mat_np(t, rows, k, acts)
        # the integer sums are exact; the SIMD branch adds the f32 terms in another order than the scalar one
        err = np.abs(got.astype(np.float64) - want).max() / np.sqrt(np.mean(want.astype(np.float64) ** 2))
        print(f"{R.NAMES[t]}: max |numpy - reference| / rms(reference) = {err:.3e}")
        assert err <= 2e-5


def test_row_geometry_of_the_kernel_library():
    from ggml_hexagon_amd import build
    lib = ctypes.CDLL(str(build.build_qmm()))
    lib.qmm_row_size.restype = ctypes.c_size_t
    lib.qmm_row_size.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert [lib.qmm_row_size(t, 256) for t in TYPES] == [54, 66]
    assert [lib.qmm_row_size(t, 4096) for t in TYPES] == [864, 1056]
    assert [lib.qmm_row_size(t, 4000) for t in TYPES] == [0, 0]
    assert lib.qmm_row_size(16, 4096) == 0                         # IQ2_XXS stays unsupported


def test_synth_weights_are_whole_rows_with_bounded_scales():
    from ggml_hexagon_amd import capi, synth
    assert (capi.TQ1_0, capi.TQ2_0) == (synth.TQ1_0, synth.TQ2_0) == (R.TQ1_0, R.TQ2_0)
    for t in TYPES:
        assert (synth.BLCK[t], synth.TYPE_SIZE[t], synth.NAMES[t]) == (256, R.BLOCK_BYTES[t], R.NAMES[t])
        w = synth.synth_weights(t, 5, 768, seed=3, sigma=0.02)
        assert w.shape == (5, R.row_size(t, 768)) and w.dtype == np.uint8
        d, v = R.fields(t, w, 768)
        assert np.isfinite(d).all() and 0.0099 <= np.abs(d).min() and np.abs(d).max() <= 0.0301 and d.min() < 0 < d.max()
        q = w.reshape(-1, R.BLOCK_BYTES[t])[:, :R.D_AT[t]]         # 15 blocks: random bytes over the full range
        assert len(np.unique(q)) > 200 and q.max() > 242
