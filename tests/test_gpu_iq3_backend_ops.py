"""IQ3_XXS / IQ3_S through the reference's own parity harness (tests/test-backend-ops.cpp, built unmodified into oracle/_ref) and the
plugin, which derives both grids from the ggml it is loaded into.  Exact counts, 0 not supported and 0 failed:
  MUL_MAT      20   n = 1 .. 9 at m = 16, k = 256 plus one case of the harness's loop over the other types, per type (:4132-4183)
  MUL_MAT_ID    4   (:4245-4259)
  GET_ROWS      8   (:3870-3876)
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


def run_tbo(*args, timeout=600):
    if not TBO.exists() or not PLUGIN.exists():
        pytest.skip("oracle/_ref/test-backend-ops or the plugin module is not built (needs the reference tree at build time)")
    env = dict(os.environ, GGML_BACKEND_PATH=str(PLUGIN))
    p = subprocess.run([str(TBO), *args], env=env, capture_output=True, text=True, timeout=timeout, cwd=str(TBO.parent))
    return p.returncode, re.sub(r"\x1b\[[0-9;]*m", "", p.stdout + p.stderr)


@pytest.mark.parametrize("op,pattern,count", [("MUL_MAT", "type_a=(iq3_xxs|iq3_s)", 20), ("MUL_MAT_ID", "type_a=(iq3_xxs|iq3_s)", 4),
                                              ("GET_ROWS", "type=(iq3_xxs|iq3_s)", 8)])
def test_iq3_cases_pass_the_reference_harness(op, pattern, count):
    rc, out = run_tbo("test", "-o", op, "-p", pattern)
    ok = len(re.findall(r"\): OK", out))
    fail = [l for l in out.splitlines() if "FAIL" in l or "ERR =" in l]
    unsup = len(re.findall(r"not supported \[", out))
    print(f"{op} {pattern}: {ok} OK, {len(fail)} failed, {unsup} not supported")
    assert "MI355X0" in out, out[-2000:]
    assert not fail, "\n".join(fail[:20])
    assert rc == 0, out[-3000:]
    assert unsup == 0 and ok == count, (ok, unsup, out[-1500:])
