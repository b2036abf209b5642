"""IQ1_S / IQ1_M without a GPU: the numpy restatement of tests/iq1_refs.py against the live reference, the run-time derivation of the
one grid both formats index, the covering rows, and the kernel library's row geometry."""
import ctypes

import numpy as np
import pytest

import iq1_refs as R

TYPES = [R.IQ1_S, R.IQ1_M]
IDS = [R.NAMES[t] for t in TYPES]


@pytest.fixture(scope="module")
def ref():
    return R.Iq1Ref()


@pytest.fixture(scope="module")
def made(ref):
    """a few rows from the reference's quantizers (slow ones: 4 rows of K = 1024 per type, made once)"""
    rng = np.random.default_rng(3)
    x = (rng.standard_normal((4, 1024)) * 0.05).astype(np.float32)
    return {t: ref.quantize(t, x) for t in TYPES}


def test_derivation_yields_the_ternary_table_through_either_dequantizer(ref):
    grid = ref.codebook(R.IQ1_S)
    assert grid.dtype == np.uint32 and grid.shape == (4096,)                   # two words per entry of eight values
    assert set(np.unique(grid.view(np.uint8)).tolist()) == {0xff, 0x00, 0x01}
    assert len(np.unique(grid.view(np.uint64))) == R.ENTRIES                   # a codebook: no entry twice
    # IQ1_M's blocks spell the same table: scale words with the top nibbles 0, 0, 8, 4 (f16 8.0)
    blk = R.crafted_blocks(R.IQ1_M)
    assert blk[:, 48:56].copy().view("<u2").tolist() == [[0x0000, 0x0000, 0x8000, 0x4000]] * 64
    assert np.array_equal(ref.codebook(R.IQ1_M), grid)


def test_grid_from_floats_refuses_what_is_no_grid_value():
    ok = np.array([-7, 1, 9, 1, 9, 9, -7, -7], np.float32)
    assert R.grid_from_floats(ok).tolist() == [0x000100ff, 0xffff0101]
    for bad in (0.0, 2.0, 8.0, -6.5, np.nan):
        v = ok.copy()
        v[5] = bad
        assert R.grid_from_floats(v) is None


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_covering_rows_cover(t):
    for k in (256, 512, 1024):
        rows = R.covering_rows(t, k, seed=5)
        d, idx, sign, scale = R._fields(t, rows, k)
        assert len(np.unique(idx)) == 2048
        assert len(np.unique(scale[..., 0])) == 8 and len(np.unique(scale[..., 1])) == 8
        assert np.isfinite(d).all() and d.min() < 0 < d.max() and np.abs(d).min() == 2.0 ** -24
        if t == R.IQ1_S:
            assert set(np.unique(sign).tolist()) == {-1, 1}
        else:                                                                   # all 16 patterns of a sub-block's four delta signs
            pat = ((sign < 0) * (1 << np.arange(4))).sum(-1)
            assert len(np.unique(pat)) == 16
            sc = rows.reshape(-1, 56)[:, 48:56].copy().view("<u2").astype(np.uint32)
            for f in range(4):                                                  # every 3-bit field of a scale word takes all 8 values
                assert len(np.unique((sc >> (3 * f)) & 7)) == 8


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_numpy_dequantize_is_the_reference_bit_for_bit(ref, made, t):
    grid = ref.codebook()
    for k, rows in ((1024, made[t]), (512, R.covering_rows(t, 512, seed=1))):
        want = ref.dequantize(t, rows, k)
        got = R.dequantize_np(t, rows, k, grid)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", TYPES, ids=IDS)
def test_numpy_dot_is_the_reference_within_f32_order(ref, made, t):
    rng = np.random.default_rng(10 + t)
    k = 1024
    grid = ref.codebook()
    x = rng.uniform(-1, 1, (3, k)).astype(np.float32)
    acts = ref.quantize_act(x)
    for rows in (made[t], R.covering_rows(t, k, seed=2)[:8]):
        want = np.array([[ref.vec_dot(t, k, rows[j], acts[i]) for j in range(rows.shape[0])] for i in range(3)], np.float32)
        got = R.mul_mat_np(t, rows, k, acts, grid)
        # the integer sums are exact; the SIMD branch adds the f32 terms in another order than the scalar one
        err = np.abs(got.astype(np.float64) - want).max() / np.sqrt(np.mean(want.astype(np.float64) ** 2))
        print(f"{R.NAMES[t]}: max |numpy - reference| / rms(reference) = {err:.3e}")
        assert err <= 2e-5


def test_row_geometry_of_the_kernel_library():
    from ggml_hexagon_amd import build
    lib = ctypes.CDLL(str(build.build_qmm()))
    lib.qmm_row_size.restype = ctypes.c_size_t
    lib.qmm_row_size.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert [lib.qmm_row_size(t, 256) for t in TYPES] == [50, 56]
    assert [lib.qmm_row_size(t, 4096) for t in TYPES] == [800, 896]
    assert [lib.qmm_row_size(t, 4000) for t in TYPES] == [0, 0]
    assert lib.qmm_row_size(16, 4096) == 0                         # IQ2_XXS stays unsupported


def test_synth_weights_are_whole_rows_with_bounded_scales():
    from ggml_hexagon_amd import synth
    for t in TYPES:
        w = synth.synth_weights(t, 5, 768, seed=3)
        assert w.shape == (5, R.row_size(t, 768)) and w.dtype == np.uint8
        d = np.abs(R._fields(t, w, 768)[0])
        assert np.isfinite(d).all() and d.min() >= 2.0 ** -10 * 0.999 and d.max() <= 2.0 ** -4
