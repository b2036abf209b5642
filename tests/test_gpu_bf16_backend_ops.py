"""BF16 src0 through the reference's own parity harness (tests/test-backend-ops.cpp, built unmodified into oracle/_ref): its MUL_MAT
cases with type_a = bf16, type_b = f32 at m = 16, k = 256, n = 1 .. 9 (both kernels: the mat-vec up to 8 tokens, the MFMA kernel at 9)
against the ggml CPU backend, NMSE <= 5e-4.  Ten cases match the pattern (n = 1 .. 8 from the harness's loop over the base types, n = 1
and n = 9 from its loop over the other types); its k = 1 case does not.  Before BF16 was a weight type all ten were "not supported"."""
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TBO = ROOT / "oracle" / "_ref" / "test-backend-ops"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"


def run_tbo(*args, timeout=900):
    if not TBO.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/test-backend-ops or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    p = subprocess.run([str(TBO), *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(TBO.parent))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)


def test_bf16_mul_mat_passes_the_reference_harness():
    rc, out = run_tbo("test", "-o", "MUL_MAT", "-p", r"type_a=bf16,type_b=f32,m=16,n=[1-9],k=256,bs=\[1,1\],nr=\[1,1\],per=\[0,1,2,3\]")
    ok = len(re.findall(r"\): OK", out))
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    unsup = len(re.findall(r"not supported \[", out))
    print(f"MUL_MAT bf16: {ok} OK, {len(fail)} failed, {unsup} not supported")
    assert "MI355X0" in out, out[-2000:]
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert unsup == 0 and ok >= 10, (ok, unsup, out[-1500:])
