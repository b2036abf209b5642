"""llama.cpp's attention block on a Q8_0 K cache (-ctk q8_0, no flash attention) through the plugin: the nodes build_attn / build_attn_mha
emit, built on ggml's public API (tests/kcache_q8_graph.py), computed once by the ggml CPU backend and once by this backend, each in a
fresh child process.  Skipped when oracle/_ref is not built (it needs the reference tree at build time)."""
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
HELPER = ROOT / "tests" / "kcache_q8_graph.py"


def run_block(backend, n, j0, n_kv, out):
    env = dict(os.environ, GGML_MI355X_DEBUG="1")
    p = subprocess.run([sys.executable, str(HELPER), backend, str(n), str(j0), str(n_kv), str(out)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (backend, p.returncode, (p.stdout + p.stderr)[-3000:])
    return dict(np.load(out)), p.stderr


def f16_ulps(a, b):
    """distance of two arrays of f16 bit patterns (same sign) in representable values"""
    return np.abs(a.astype(np.int32) - b.astype(np.int32))


@pytest.mark.parametrize("n,j0,n_kv", [(2, 37, 64), (40, 0, 64)], ids=["few-tokens", "prompt"])
def test_attention_block_on_a_q8_0_k_cache_matches_the_cpu_backend(tmp_path, n, j0, n_kv):
    if not (REF / "libggml.so").exists() or not (REF / "libggml-cpu.so").exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref or the plugin module is not built (needs the reference tree at build time)")
    want, _ = run_block("cpu", n, j0, n_kv, tmp_path / "cpu.npz")
    got, log = run_block("mi355x", n, j0, n_kv, tmp_path / "dev.npz")
    fused = [l for l in log.splitlines() if l.startswith("fused: attention")]
    print(f"q8_0 K cache, N = {n}, j0 = {j0}, n_kv = {n_kv}: fused lines {fused}")
    nmse = float(np.sum((got["out"].astype(np.float64) - want["out"]) ** 2) / np.sum(want["out"].astype(np.float64) ** 2))
    print(f"q8_0 K cache, N = {n}, j0 = {j0}, n_kv = {n_kv}: NMSE of the output {nmse:.3g}")
    assert nmse <= 5e-4                                                 # the reference harness's MUL_MAT bound (tests/test-backend-ops.cpp:1982-1984)
    for l in range(2):
        a = got[f"k_rows{l}"].reshape(n, -1, 34)
        b = want[f"k_rows{l}"].reshape(n, -1, 34)
        # the rope's f32 sin / cos may flip a rounding: one count per int8, one f16 ulp of d
        dq = np.abs(a[:, :, 2:].view(np.int8).astype(np.int32) - b[:, :, 2:].view(np.int8).astype(np.int32))
        dd = f16_ulps(np.ascontiguousarray(a[:, :, 0:2]).view(np.uint16), np.ascontiguousarray(b[:, :, 0:2]).view(np.uint16))
        print(f"  block {l}: K rows differ in {int((dq > 0).sum())} of {dq.size} int8 values (max {int(dq.max())}), d in {int((dd > 0).sum())} of {dd.size} (max {int(dd.max())} ulp)")
        assert dq.max() <= 1 and dd.max() <= 1
        # the V store is the existing f32 -> f16 copy: the same bytes, and nothing outside the batch's columns
        assert np.array_equal(got[f"v_cache{l}"].view(np.uint16), want[f"v_cache{l}"].view(np.uint16))
    if n <= 8:
        assert any("few tokens" in l for l in fused), log[-3000:]
