"""llama.cpp's attention block on a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 (-ctk q4_0 / q4_1 / q5_0 / q5_1, no flash attention) through the plugin:
the nodes build_attn / build_attn_mha emit, built on ggml's public API (tests/kblk_graph.py), computed once by the ggml CPU backend and once
by this backend, each in a fresh child process.  The second of the helper's two blocks runs its nodes one by one: that is what covers
MUL_MAT on a permuted src0 of the Q5 types, which the reference harness has no case for.  Skipped when oracle/_ref is not built (it needs
the reference tree at build time)."""
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
REF = ROOT / "oracle" / "_ref"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"
HELPER = ROOT / "tests" / "kblk_graph.py"

sys.path.insert(0, str(ROOT / "tests"))

import kblk_refs as R  # noqa: E402

CODE = {R.NAMES[t]: t for t in R.TYPES}


def run_block(backend, k_type, n, j0, n_kv, out):
    env = dict(os.environ, GGML_MI355X_DEBUG="1")
    p = subprocess.run([sys.executable, str(HELPER), backend, k_type, str(n), str(j0), str(n_kv), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (backend, p.returncode, (p.stdout + p.stderr)[-3000:])
    return dict(np.load(out)), p.stderr


def f16_ulps(a, b):
    """distance of two arrays of f16 bit patterns in representable values (sign-magnitude patterns put on one line first)"""
    line = lambda u: np.where(u & 0x8000, -(u & 0x7FFF).astype(np.int32), (u & 0x7FFF).astype(np.int32))
    return np.abs(line(a) - line(b))


@pytest.mark.parametrize("n,j0,n_kv", [(2, 37, 64), (40, 0, 64)], ids=["few-tokens", "prompt"])
@pytest.mark.parametrize("k_type", list(CODE))
def test_attention_block_on_a_k_cache_of_the_type_matches_the_cpu_backend(tmp_path, k_type, n, j0, n_kv):
    if not (REF / "libggml.so").exists() or not (REF / "libggml-cpu.so").exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref or the plugin module is not built (needs the reference tree at build time)")
    t = CODE[k_type]
    want, _ = run_block("cpu", k_type, n, j0, n_kv, tmp_path / "cpu.npz")
    got, log = run_block("mi355x", k_type, n, j0, n_kv, tmp_path / "dev.npz")
    fused = [l for l in log.splitlines() if l.startswith("fused: attention")]
    print(f"{k_type} K cache, N = {n}, j0 = {j0}, n_kv = {n_kv}: fused lines {fused}")
    nmse = float(np.sum((got["out"].astype(np.float64) - want["out"]) ** 2) / np.sum(want["out"].astype(np.float64) ** 2))
    print(f"{k_type} K cache, N = {n}, j0 = {j0}, n_kv = {n_kv}: NMSE of the output {nmse:.3g}")
    assert nmse <= 5e-4                                                 # the reference harness's MUL_MAT bound (tests/test-backend-ops.cpp:1982-1984)
    for l in range(2):
        a = got[f"k_rows{l}"].reshape(n, -1, R.BLOCK[t])
        b = want[f"k_rows{l}"].reshape(n, -1, R.BLOCK[t])
        # the rope's f32 sin / cos may flip a rounding: one count per code, one f16 ulp of d and m
        dq = np.abs(R.codes(t, a) - R.codes(t, b))
        (da, ma), (db, mb) = R.scales(t, a), R.scales(t, b)
        dd = f16_ulps(da, db)
        dm = f16_ulps(ma, mb) if R.HAS_M[t] else np.zeros(1, np.int32)
        print(f"  block {l}: K rows differ in {int((dq > 0).sum())} of {dq.size} codes (max {int(dq.max())}), d in {int((dd > 0).sum())} of {dd.size} "
              f"(max {int(dd.max())} ulp), m max {int(dm.max())} ulp")
        assert dq.max() <= 1 and dd.max() <= 1 and dm.max() <= 1
        # the V store is the existing f32 -> f16 copy: the same bytes, and nothing outside the batch's columns
        assert np.array_equal(got[f"v_cache{l}"].view(np.uint16), want[f"v_cache{l}"].view(np.uint16))
    if n <= 8:
        assert any("few tokens" in l for l in fused), log[-3000:]
