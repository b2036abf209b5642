"""What a Q8_0 K cache needs of single ops, judged by the REFERENCE's own parity harness (tests/test-backend-ops.cpp, built unmodified
into oracle/_ref) through the plugin: CPY f32 -> Q8_0 (the K store), CPY Q8_0 -> f32 (the cast of a K-shift) and MUL_MAT with a
permuted Q8_0 src0 (kq on the cache view when the attention chain is not fused).  Every case of each filter is compared with the ggml CPU
backend and none may be reported as not supported.  Each filter is run once."""
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TBO = ROOT / "oracle" / "_ref" / "test-backend-ops"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"

# the harness filters on vars(): CPY "type_src=f32,type_dst=q8_0,ne=[256,4,4,4],permute_src=[0,0,0,0],permute_dst=[0,0,0,0]" (:4029-4040, two
# shapes per type pair); MUL_MAT "type_a=q8_0,type_b=f32,m=16,n=1,k=256,bs=[2,3],nr=[1,1],per=[0,2,1,3],v=0" (:4163-4173: n = 1, 8, 16 for
# each of three permutations)
FILTERS = {
    "cpy-f32-q8_0": (("-o", "CPY", "-p", "type_src=f32,type_dst=q8_0"), 2),
    "cpy-q8_0-f32": (("-o", "CPY", "-p", "type_src=q8_0,type_dst=f32"), 2),
    "mul_mat-permuted": (("-o", "MUL_MAT", "-p", r"type_a=q8_0,type_b=f32,.*per=\[0,(2,1,3|1,3,2|3,2,1)\]"), 9),
}


def run_tbo(*args, timeout=600):
    if not TBO.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/test-backend-ops or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    p = subprocess.run([str(TBO), "test", *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(TBO.parent))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)


@pytest.mark.parametrize("name", list(FILTERS))
def test_reference_harness_passes_what_a_q8_0_k_cache_needs(name):
    args, cases = FILTERS[name]
    rc, out = run_tbo(*args)
    assert "MI355X0" in out, out[-2000:]
    ok = len(re.findall(r"\): OK", out))
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    unsup = len(re.findall(r"not supported \[", out))
    print(f"{name}: {ok} OK, {len(fail)} failed, {unsup} not supported")
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert unsup == 0, out[-3000:]
    assert ok == cases, (ok, out[-2000:])
