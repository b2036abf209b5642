"""IQ1_S / IQ1_M through the reference's own parity harness (tests/test-backend-ops.cpp, built unmodified into oracle/_ref) and the
plugin, which derives the grid both formats index from the ggml it is loaded into.  Exact counts, 0 not supported and 0 failed.  Both
types are members of the harness's all_types and other_types lists (:3827, :3849), so per type
  MUL_MAT      n = 1 .. 9 at m = 16, k = 256 from the loop over all_types (:4132-4136): 9, and one case from the loop over other_types
               (:4176-4183; the block size is 256, so the first of its two cases is skipped): 10, 20 for both types
  MUL_MAT_ID   4 experts, 2 used, n = 1 and 32 from the loop over other_types (:4245-4259): 2, 4 for both
  GET_ROWS     b = 1 and 7, contiguous and a view, from the loop over all_types (:3870-3876): 4, 8 for both
Before the two types ran on the device every one of these cases was "not supported"."""
import os
import re
import subprocess
from pathlib import Path

import pytest

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parents[1]
TBO = ROOT / "oracle" / "_ref" / "test-backend-ops"
PLUGIN = ROOT / "ggml-hexagon_amd" / "libggml-mi355x.so"
N_TYPES = 2
COUNTS = {"MUL_MAT": N_TYPES * (9 + 1), "MUL_MAT_ID": N_TYPES * 2, "GET_ROWS": N_TYPES * 2 * 2}


def run_tbo(*args, timeout=600):
    if not TBO.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/test-backend-ops or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    p = subprocess.run([str(TBO), *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(TBO.parent))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)


@pytest.mark.parametrize("op,pattern", [("MUL_MAT", "type_a=(iq1_s|iq1_m)"), ("MUL_MAT_ID", "type_a=(iq1_s|iq1_m)"), ("GET_ROWS", "type=(iq1_s|iq1_m)")])
def test_iq1_cases_pass_the_reference_harness(op, pattern):
    rc, out = run_tbo("test", "-o", op, "-p", pattern)
    ok = len(re.findall(r"\): OK", out))
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    unsup = len(re.findall(r"not supported \[", out))
    print(f"{op} {pattern}: {ok} OK, {len(fail)} failed, {unsup} not supported (expected {COUNTS[op]} OK)")
    assert "MI355X0" in out, out[-2000:]
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert unsup == 0 and ok == COUNTS[op], (ok, unsup, out[-1500:])


def test_iq2_xxs_is_still_reported_as_not_supported():
    rc, out = run_tbo("test", "-o", "MUL_MAT", "-p", "type_a=iq2_xxs,")
    ok = len(re.findall(r"\): OK", out))
    unsup = len(re.findall(r"not supported \[", out))
    print(f"MUL_MAT type_a=iq2_xxs: {ok} OK, {unsup} not supported")
    assert "MI355X0" in out, out[-2000:]
    assert ok == 0 and unsup > 0, out[-1500:]
