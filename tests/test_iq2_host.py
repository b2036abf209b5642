"""IQ2_XS / IQ2_S without a GPU: the numpy restatement of tests/iq2_refs.py against the live reference, the run-time derivation of the
grids, the sign formula, the covering rows, and the kernel library's row geometry."""
import ctypes

import numpy as np
import pytest

import iq2_refs as R

TYPES = [R.IQ2_XS, R.IQ2_S]


@pytest.fixture(scope="module")
def ref():
    return R.Iq2Ref()


@pytest.mark.parametrize("t", TYPES)
def test_derivation_yields_a_full_table_of_bytes_in_range(ref, t):
    grid = ref.codebook(t)
    assert grid.dtype == np.uint32 and grid.shape == (2 * R.ENTRIES[t],)       # two words per entry of eight magnitudes
    b = grid.view(np.uint8)
    assert b.min() >= 1 and b.max() <= 255
    assert b.max() <= 127                              # what the kernel library takes: a magnitude with its sign is an int8
    assert len(np.unique(grid.view(np.uint64))) == R.ENTRIES[t]                # a codebook: no entry twice


def test_grid_from_floats_refuses_what_is_no_byte():
    ok = np.arange(1, 9, dtype=np.float32)
    assert R.grid_from_floats(ok).tolist() == [0x04030201, 0x08070605]
    for bad in (0.0, 256.0, 2.5, -3.0, np.nan):
        v = ok.copy()
        v[5] = bad
        assert R.grid_from_floats(v) is None


@pytest.mark.parametrize("t", TYPES)
def test_covering_rows_cover(t):
    k = 512
    _, idx, signs, nib = R._fields(t, R.covering_rows(t, k, seed=5), k)
    assert len(np.unique(idx)) == R.ENTRIES[t] and len(np.unique(signs)) == R.N_SIGNS[t]
    assert len(np.unique(nib[..., 0])) == 16 and len(np.unique(nib[..., 1])) == 16


@pytest.mark.parametrize("t", TYPES)
def test_numpy_dequantize_is_the_reference_bit_for_bit(ref, t):
    rng = np.random.default_rng(t)
    k = 512
    grid = ref.codebook(t)
    w = ref.quantize(t, (rng.standard_normal((16, k)) * 0.05).astype(np.float32))
    for rows in (w, R.covering_rows(t, k, seed=1)):
        want = ref.dequantize(t, rows, k)
        got = R.dequantize_np(t, rows, k, grid)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize("t", TYPES)
def test_numpy_dot_is_the_reference_within_f32_order(ref, t):
    rng = np.random.default_rng(10 + t)
    k = 1024
    grid = ref.codebook(t)
    x = rng.uniform(-1, 1, (3, k)).astype(np.float32)
    acts = ref.quantize_act(x)
    w = ref.quantize(t, (rng.standard_normal((8, k)) * 0.05).astype(np.float32))
    for rows in (w, R.covering_rows(t, k, seed=2)[:8]):
        want = np.array([[ref.vec_dot(t, k, rows[j], acts[i]) for j in range(rows.shape[0])] for i in range(3)], np.float32)
        got = R.mul_mat_np(t, rows, k, acts, grid)
        # the integer sums are exact; the SIMD branch adds the blocks' f32 terms in another order than the scalar one
        scale = np.abs(want).max()
        err = np.abs(got.astype(np.float64) - want).max() / scale
        print(f"type {t}: max |numpy - reference| / max |reference| = {err:.3e}")
        assert err <= 1e-6


def test_sign_formula_is_what_the_reference_applies(ref):
    """all 128 sign indices of IQ2_XS, seen through the signs of dequantized values"""
    blk = np.zeros((4, R.BLOCK_BYTES[R.IQ2_XS]), np.uint8)
    blk[:, 0:2] = np.array([8.0], np.float16).view(np.uint8)
    blk[:, 2:66] = (np.arange(128, dtype=np.uint16) << 9).view(np.uint8).reshape(4, 64)     # sign index s on entry s, grid index 0
    y = ref.dequantize(R.IQ2_XS, blk, 256).reshape(128, 8)
    seen = (np.signbit(y).astype(np.uint32) << np.arange(8)).sum(1)
    assert seen.tolist() == R.sign_byte(np.arange(128)).tolist()
    assert all(bin(int(v)).count("1") % 2 == 0 for v in seen)     # eight signs of even parity


def test_row_geometry_of_the_kernel_library():
    from ggml_hexagon_amd import build
    lib = ctypes.CDLL(str(build.build_qmm()))
    lib.qmm_row_size.restype = ctypes.c_size_t
    lib.qmm_row_size.argtypes = [ctypes.c_int, ctypes.c_int64]
    assert [lib.qmm_row_size(t, 256) for t in TYPES] == [74, 82]
    assert [lib.qmm_row_size(t, 4096) for t in TYPES] == [1184, 1312]
    assert [lib.qmm_row_size(t, 100) for t in TYPES] == [0, 0]
    assert lib.qmm_row_size(16, 4096) == 0                         # IQ2_XXS stays unsupported


def test_synth_weights_are_whole_rows_with_bounded_scales():
    from ggml_hexagon_amd import synth
    for t in TYPES:
        w = synth.synth_weights(t, 5, 768, seed=3)
        assert w.shape == (5, R.row_size(t, 768)) and w.dtype == np.uint8
        d = np.abs(w.reshape(-1, R.BLOCK_BYTES[t])[:, 0:2].copy().view(np.float16).astype(np.float32))
        assert np.isfinite(d).all() and d.min() >= 2.0 ** -10 * 0.999 and d.max() <= 2.0 ** -4
