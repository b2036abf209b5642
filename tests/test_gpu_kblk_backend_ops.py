"""What a K cache in Q4_0, Q4_1, Q5_0 or Q5_1 needs of single ops, judged by the REFERENCE's own parity harness (tests/test-backend-ops.cpp,
built unmodified into oracle/_ref) through the plugin: CPY f32 -> type (the K store), CPY type -> f32 (the cast of a K-shift) and MUL_MAT with
a permuted src0 of the type (kq on the cache view when the attention chain is not fused; the harness permutes only its base types, Q4_0
and Q4_1 of these four).  Every case of each filter is compared with the ggml CPU backend and none may be reported as not supported.  Each
filter is run once."""
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TBO = ROOT / "oracle" / "_ref" / "test-backend-ops"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"

# the harness filters on vars(): CPY "type_src=f32,type_dst=q4_0,ne=[256,4,4,4],permute_src=[0,0,0,0],permute_dst=[0,0,0,0]" (two shapes per
# type pair); MUL_MAT "type_a=q4_0,type_b=f32,m=16,n=1,k=256,bs=[2,3],nr=[1,1],per=[0,2,1,3],v=0" (n = 1, 8, 16 for each of three permutations)
FILTERS = {}
for _t in ("q4_0", "q4_1", "q5_0", "q5_1"):
    FILTERS[f"cpy-f32-{_t}"] = (("-o", "CPY", "-p", f"type_src=f32,type_dst={_t}"), 2)
    FILTERS[f"cpy-{_t}-f32"] = (("-o", "CPY", "-p", f"type_src={_t},type_dst=f32"), 2)
for _t in ("q4_0", "q4_1"):
    FILTERS[f"mul_mat-permuted-{_t}"] = (("-o", "MUL_MAT", "-p", rf"type_a={_t},type_b=f32,.*per=\[0,(2,1,3|1,3,2|3,2,1)\]"), 9)


def run_tbo(*args, timeout=600):
    if not TBO.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/test-backend-ops or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    p = subprocess.run([str(TBO), "test", *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(TBO.parent))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)


@pytest.mark.parametrize("name", list(FILTERS))
def test_reference_harness_passes_what_such_a_k_cache_needs(name):
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
