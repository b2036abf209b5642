"""The one-launch rope + quantized K store inside the plugin: llama.cpp's attention block on a K cache of Q8_0, Q4_0, Q4_1, Q5_0 or Q5_1
blocks (the unchanged helpers tests/kcache_q8_graph.py and tests/kblk_graph.py, a fresh child process per run), computed three ways: by the
ggml CPU backend, by this backend, and by this backend with fusion off (GGML_MI355X_FUSE=0: rope(k) and its CPY as their own nodes).  The
default run must take the new launch for both blocks and still take the attention chain at its kq; the two device runs must store the same
bytes; against the CPU backend the neighbours' bounds hold.  Skipped when oracle/_ref is not built (it needs the reference tree at build
time)."""
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

sys.path.insert(0, str(ROOT / "tests"))

import kblk_refs as R  # noqa: E402

Q8_0 = 8
CODE = {"q8_0": Q8_0, **{R.NAMES[t]: t for t in R.TYPES}}
BLOCK = {Q8_0: 34, **R.BLOCK}


def run_block(backend, k_type, n, j0, n_kv, out, fuse=True):
    env = dict(os.environ, GGML_MI355X_DEBUG="1")
    env.pop("GGML_MI355X_FUSE", None)
    if not fuse:
        env["GGML_MI355X_FUSE"] = "0"
    if k_type == "q8_0":
        cmd = [sys.executable, str(ROOT / "tests" / "kcache_q8_graph.py"), backend, str(n), str(j0), str(n_kv), str(out)]
    else:
        cmd = [sys.executable, str(ROOT / "tests" / "kblk_graph.py"), backend, k_type, str(n), str(j0), str(n_kv), str(out)]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (backend, p.returncode, (p.stdout + p.stderr)[-3000:])
    return dict(np.load(out)), p.stderr


def f16_ulps(a, b):
    """distance of two arrays of f16 bit patterns in representable values (sign-magnitude patterns put on one line first)"""
    line = lambda u: np.where(u & 0x8000, -(u & 0x7FFF).astype(np.int32), (u & 0x7FFF).astype(np.int32))
    return np.abs(line(a) - line(b))


def block_fields(t, rows):
    """(codes, d bits, m bits or None) of rows of blocks of type t"""
    if t == Q8_0:
        return rows[:, :, 2:].copy().view(np.int8).astype(np.int32), rows[:, :, 0:2].copy().view(np.uint16), None
    d, m = R.scales(t, rows)
    return R.codes(t, rows).astype(np.int32), d, m if R.HAS_M[t] else None


@pytest.mark.parametrize("n,j0,n_kv", [(2, 37, 64), (40, 0, 64)], ids=["few-tokens", "prompt"])
@pytest.mark.parametrize("k_type", list(CODE))
def test_block_takes_the_one_launch_store(tmp_path, k_type, n, j0, n_kv):
    if not (REF / "libggml.so").exists() or not (REF / "libggml-cpu.so").exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref or the plugin module is not built (needs the reference tree at build time)")
    t = CODE[k_type]
    want, _ = run_block("cpu", k_type, n, j0, n_kv, tmp_path / "cpu.npz")
    got, log = run_block("mi355x", k_type, n, j0, n_kv, tmp_path / "dev.npz")
    plain, log0 = run_block("mi355x", k_type, n, j0, n_kv, tmp_path / "dev0.npz", fuse=False)
    store = [l for l in log.splitlines() if l.startswith("fused: rope + quantized k store")]
    attn = [l for l in log.splitlines() if l.startswith("fused: attention")]
    print(f"{k_type} K cache, N = {n}: {store} {attn}")
    assert len(store) == 2 and all(l.endswith(f", {k_type})") for l in store), log[-3000:]          # once per block
    assert attn, log[-3000:]
    assert not [l for l in log0.splitlines() if l.startswith("fused: rope")], log0[-3000:]
    nmse = float(np.sum((got["out"].astype(np.float64) - want["out"]) ** 2) / np.sum(want["out"].astype(np.float64) ** 2))
    print(f"{k_type} K cache, N = {n}, j0 = {j0}, n_kv = {n_kv}: NMSE of the output {nmse:.3g}")
    assert nmse <= 5e-4                                                 # the reference harness's MUL_MAT bound (tests/test-backend-ops.cpp:1982-1984)
    for l in range(2):
        # one launch or three: the same bytes in both caches
        assert np.array_equal(got[f"k_rows{l}"], plain[f"k_rows{l}"])
        assert np.array_equal(got[f"v_cache{l}"].view(np.uint16), plain[f"v_cache{l}"].view(np.uint16))
        # against the CPU backend the rope's f32 sin / cos may flip a rounding: one count per code, one f16 ulp of d and m
        (qa, da, ma), (qb, db, mb) = block_fields(t, got[f"k_rows{l}"].reshape(n, -1, BLOCK[t])), block_fields(t, want[f"k_rows{l}"].reshape(n, -1, BLOCK[t]))
        dq, dd = np.abs(qa - qb), f16_ulps(da, db)
        dm = f16_ulps(ma, mb) if ma is not None else np.zeros(1, np.int32)
        print(f"  block {l}: K rows differ in {int((dq > 0).sum())} of {dq.size} codes (max {int(dq.max())}), d max {int(dd.max())} ulp, m max {int(dm.max())} ulp")
        assert dq.max() <= 1 and dd.max() <= 1 and dm.max() <= 1
        assert np.array_equal(got[f"v_cache{l}"].view(np.uint16), want[f"v_cache{l}"].view(np.uint16))
